"""bench.py's plain run and --dump-outputs: the line carries the headline fields and nothing that takes runs of its own
(those need --full), and two runs with the same arguments write the same outputs of their last timed step, bit for bit
— the timed steps start from the seeded state whatever the warm-up ran, and every kernel is deterministic."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, out_dir):
    env = dict(os.environ, SF_BENCH_SETTLE_MS="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SF_RANK_CPUS", "SF_BENCH_FORCE_SPAWN"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args +
                       ["--dump-outputs", out_dir], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stderr[:3000], r.stderr[-1500:])
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return line, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


# dual at one clip: 34 M parameters, so params / grads are the seeded samples; shufflenetv2: the launch-bound config,
# whose timed form (eager or hipGraph replay) is chosen by timing and may differ between the two runs
@pytest.mark.parametrize("args", [["--workload", "dual", "--batch", "1", "--steps", "3", "--warmup", "2"],
                                  ["--workload", "shufflenetv2", "--steps", "5", "--warmup", "2"]],
                         ids=["dual_b1", "shufflenetv2"])
def test_plain_run_dumps_the_same_outputs_twice(args, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()  # the children are other processes on the same GPU
    (a, da), (b, db) = _bench(args, str(tmp_path / "a")), _bench(args, str(tmp_path / "b"))
    for line in (a, b):
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line, k
        assert line["steps"] == int(args[args.index("--steps") + 1]) and line["ms_per_step"] > 0
        for k in ("cpu_baseline", "roofline", "eval_forward", "clocks", "launch_bound", "fwd_max_rel_err"):
            assert k not in line, k                                    # --full only
        assert "grad_hash" not in line["allreduce"] and line["parity_gate"].startswith("not run")
    assert sorted(da) == ["buffers", "grads", "logits", "loss", "params"]
    assert sum(v.nbytes for v in da.values()) <= 64 << 20
    for k in da:
        assert da[k].dtype == np.float32 and np.isfinite(da[k]).all(), k
        assert np.array_equal(da[k], db[k]), (k, a["config"]["launch_probe"], b["config"]["launch_probe"])
    assert abs(float(da["loss"][0]) - a["last_timed_step_loss"]) < 1e-5
    assert a["last_timed_step_loss"] == b["last_timed_step_loss"]
