#!/usr/bin/env python3
"""Gradient clipping alone, on the real parameter list of a workload through FlatGradients (default: dual, the 8x8 R50 +
CMDA model bench.py times).

Arms (the whole call, as a training loop issues it):
  HipGradClip, scale taken     max_norm drops by a tenth in front of every call (a fixed max_norm would clip once and
                               then find the norm at the limit: coefficient 1), so every call scales by about 0.9 — the
                               scale pass reads and writes every gradient; the call includes the 8-byte upload of the
                               new max_norm, as a scheduled learning rate costs the optimizers
  HipGradClip, scale skipped   max_norm far above the norm: the coefficient is 1.0f and sf_grad_scale touches nothing
  torch clip_grad_norm_        torch.nn.utils.clip_grad_norm_(params, 1.0) (foreach; multiplies every time)
and the two native calls alone on the table HipGradClip built: sf_grad_norm (partials + finish) and sf_grad_scale
with the coefficient forced below 1, with the bytes/s they achieve (norm: every gradient read once; scale: read once
and written once).
Method: every arm warmed up, then ROUNDS rounds in which the arms alternate; an arm's round is REPS calls between two
HIP events, per call; the figure is the median round, the spread its min .. max.  Clocks not pinned.
The bound: the gradient bytes once for the norm, twice more when scaling, at the 5.0 TB/s sgd_step_kernel reaches on
the same list.
usage: tools/microbench/grad_clip_bench.py [out.txt] [workload ...]"""
import contextlib
import io
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd"), os.path.join(ROOT, "tests", "golden")]
import torch  # noqa: E402
import bench  # noqa: E402
from slowfast.models.step_tail import ST_COEF, HipGradClip, grad_norm, grad_scale  # noqa: E402
from slowfast.utils.distributed import FlatGradients  # noqa: E402

ROUNDS, REPS = 9, 5
SGD_TBPS = 5.0  # sgd_step_kernel on cfg #3's list (profiles/step_tail.txt)


def alternate(arms):
    for _, fn in arms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in arms}
    for _ in range(ROUNDS):
        for name, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e-3 / REPS)
    return times


def fmt(v):
    return "%8.1f us (%7.1f .. %7.1f)" % (statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6)


def one_workload(workload, out):
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        cfg, model, batch, desc = bench.build(workload, dev)
    params = [p for p in model.parameters() if p.requires_grad]
    flat = FlatGradients(params)
    n = flat.flat.numel()
    g = torch.Generator(device="cpu").manual_seed(1)
    fill = torch.randn(n, generator=g).to(dev) * 1e-3
    flat.flat.copy_(fill)
    taken = HipGradClip(params, max_norm=1.0)
    skipped = HipGradClip(params, max_norm=1e6)

    def clip_taken():
        taken.max_norm *= 0.9
        taken.clip()

    arms = [("HipGradClip, scale taken", clip_taken), ("HipGradClip, scale skipped", skipped.clip),
            ("torch clip_grad_norm_", lambda: torch.nn.utils.clip_grad_norm_(params, 1.0))]
    times = alternate(arms)
    coef = (float(taken.coef.cpu()[0]), float(skipped.coef.cpu()[0]))
    assert 0.8 < coef[0] < 1.0 and coef[1] == 1.0, coef
    lines = ["== %s: %s; %d gradient tensors, %.2f M elements (%.1f MB), %d chunks" % (
        workload, desc, len(params), n / 1e6, n * 4 / 1e6, taken._chunks.shape[0])]
    lines.append("   the call (HIP events)            per call                       bound at %.1f TB/s" % SGD_TBPS)
    bounds = {"HipGradClip, scale taken": 3, "HipGradClip, scale skipped": 1, "torch clip_grad_norm_": 3}
    for name, _ in arms:
        lines.append("   %-30s %s   %6.1f us (%d x the gradient bytes)" % (
            name, fmt(times[name]), bounds[name] * n * 4 / (SGD_TBPS * 1e12) * 1e6, bounds[name]))
    t = {k: statistics.median(v) for k, v in times.items()}
    lines.append("   torch / HipGradClip: %.2f x with the scale pass taken, %.2f x with it skipped" % (
        t["torch clip_grad_norm_"] / t["HipGradClip, scale taken"],
        t["torch clip_grad_norm_"] / t["HipGradClip, scale skipped"]))
    # the native calls alone
    flat.flat.copy_(fill)
    tabs = (taken._table, taken._table_dev, taken._chunks, taken._chunks_dev)
    state = taken._state.clone()
    state[ST_COEF] = 0.999999
    raw = alternate([("sf_grad_norm", lambda: grad_norm(*tabs, 2, taken._partials, taken._state,
                                                        max_norm=taken._hyper_dev[0:1])),
                     ("sf_grad_scale", lambda: grad_scale(*tabs, state))])
    lines.append("   native calls alone (HIP events)  per call                       achieved")
    for name, passes in (("sf_grad_norm", 1), ("sf_grad_scale", 2)):
        lines.append("   %-30s %s   %6.2f TB/s" % (name, fmt(raw[name]),
                                                  passes * n * 4 / statistics.median(raw[name]) / 1e12))
    for ln in lines:
        print(ln, file=out, flush=True)
        if out is not sys.stdout:
            print(ln, flush=True)


def main():
    args = sys.argv[1:]
    out = open(args[0], "w") if args and args[0].endswith(".txt") else sys.stdout
    workloads = [a for a in args if not a.endswith(".txt")] or ["dual"]
    print("grad_clip_bench: torch %s on %s; %d rounds x %d calls per arm, arms alternate, median (min .. max)" % (
        torch.__version__, torch.cuda.get_device_name(0), ROUNDS, REPS), file=out, flush=True)
    print("command: python tools/microbench/grad_clip_bench.py %s" % " ".join(args), file=out, flush=True)
    for w in workloads:
        one_workload(w, out)


if __name__ == "__main__":
    main()
