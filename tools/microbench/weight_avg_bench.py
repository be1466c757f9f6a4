#!/usr/bin/env python3
"""The averaged weights alone, on the parameters and buffers of a workload (default: dual, the 8x8 R50 + CMDA model
bench.py times).

Arms:
  HipAveragedModel.update_parameters   one sf_avg_update call (the table update, then the one-thread count launch);
                                       12 bytes per averaged float element (both sides read, the average written)
  torch AveragedModel.update_parameters   get_ema_multi_avg_fn: foreach lerp over a deep copy of the module
  HipAveragedModel.swap                one sf_avg_exchange launch, 16 bytes per element (both sides read and written)
  sf_avg_update alone                  the native call on the table the object built, no host work but the call
  precise-BN averaging, one iteration  sf_avg_update mode 2 over every {accumulator, running statistic} pair, against
                                       the loop it replaced: mean += (running - mean) / (k + 1), twice per BN layer
The Hip arms alternate among themselves and torch's arms among themselves.
Method: every arm warmed up, then ROUNDS rounds in which the arms alternate; an arm's round is REPS calls between two
HIP events, per call; the figure is the median round, the spread its min .. max.  Clocks not pinned.
usage: tools/microbench/weight_avg_bench.py [out.txt] [workload ...]"""
import contextlib
import io
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd"), os.path.join(ROOT, "tests", "golden"),
                os.path.join(ROOT, "tests")]
import torch  # noqa: E402
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn  # noqa: E402
import bench  # noqa: E402
from slowfast.models import weight_avg  # noqa: E402
from slowfast.models.step_tail import carve_views  # noqa: E402
from slowfast.utils.precise_bn import get_bn_modules  # noqa: E402

ROUNDS, REPS = 9, 5
DECAY = 0.999


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
    model.train()
    ema = weight_avg.HipAveragedModel(model, decay=DECAY)
    n_float = sum(v.numel() for v in ema.averaged.values() if v.dtype == torch.float32)
    n_words = sum(v.numel() for v in ema.averaged.values() if v.dtype == torch.int64)
    ema.update_parameters()
    args = ema._args(None)
    hip = alternate([("HipAveragedModel.update_parameters", ema.update_parameters),
                     ("HipAveragedModel.swap", ema.swap),
                     ("sf_avg_update alone", lambda: weight_avg.avg_update(
                         *args, ema.mode, ema.n_averaged, hyper_host=ema._w_host, hyper=ema._w_dev))])
    # one precise-BN iteration's averaging: the native call and the loop it replaced, on the same layers
    layers = get_bn_modules(model)
    stats = [t for bn in layers for t in (bn.running_mean, bn.running_var)]
    _, acc = carve_views([t.numel() for t in stats], dev)
    table = weight_avg._PairTable("weight_avg_bench")
    pairs = [(a, t, weight_avg.KIND_AVG) for a, t in zip(acc, stats)]
    count = torch.full((), 3, dtype=torch.int64, device=dev)
    mean = [torch.zeros_like(bn.running_mean) for bn in layers]
    var = [torch.zeros_like(bn.running_var) for bn in layers]

    def torch_loop():
        with torch.no_grad():
            for i, bn in enumerate(layers):
                mean[i] += (bn.running_mean - mean[i]) / 4
                var[i] += (bn.running_var - var[i]) / 4

    pb_args = table.args(pairs)
    pb = alternate([("precise-BN: sf_avg_update mode 2", lambda: weight_avg.avg_update(
        *pb_args, weight_avg.MODE_RUNNING, count))])
    t_avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(DECAY), use_buffers=True)
    t_avg.update_parameters(model)
    tt = alternate([("torch AveragedModel.update_parameters", lambda: t_avg.update_parameters(model)),
                    ("precise-BN: torch loop", torch_loop)])
    n_stats = sum(t.numel() for t in stats)
    lines = ["== %s: %s; %d tensors, %.2f M float elements (%.1f MB) + %d int64 words, %d chunks; %d BN layers, %d "
             "statistics" % (workload, desc, len(ema.averaged), n_float / 1e6, n_float * 4 / 1e6, n_words,
                             ema._tab.chunks.shape[0], len(layers), n_stats)]
    lines.append("   (HIP events)                            per call")
    for times in (hip, tt, pb):
        for name in times:
            lines.append("   %-38s %s" % (name, fmt(times[name])))
    m = {k: statistics.median(v) for t in (hip, tt, pb) for k, v in t.items()}
    bytes_update, bytes_swap = 12 * n_float + 16 * n_words, 16 * n_float + 32 * n_words
    lines.append("   update: %.1f MB by counting (12 B per element): update_parameters %.2f TB/s, the native call alone "
                 "%.2f TB/s" % (bytes_update / 1e6, bytes_update / m["HipAveragedModel.update_parameters"] / 1e12,
                                bytes_update / m["sf_avg_update alone"] / 1e12))
    lines.append("   swap:   %.1f MB by counting (16 B per element): %.2f TB/s" % (
        bytes_swap / 1e6, bytes_swap / m["HipAveragedModel.swap"] / 1e12))
    lines.append("   torch AveragedModel.update_parameters / HipAveragedModel.update_parameters: %.2f x" % (
        m["torch AveragedModel.update_parameters"] / m["HipAveragedModel.update_parameters"]))
    lines.append("   precise-BN averaging per iteration: torch loop / sf_avg_update mode 2: %.2f x" % (
        m["precise-BN: torch loop"] / m["precise-BN: sf_avg_update mode 2"]))
    for ln in lines:
        print(ln, file=out, flush=True)
        if out is not sys.stdout:
            print(ln, flush=True)


def main():
    args = sys.argv[1:]
    out = open(args[0], "w") if args and args[0].endswith(".txt") else sys.stdout
    workloads = [a for a in args if not a.endswith(".txt")] or ["dual"]
    print("weight_avg_bench: torch %s on %s; %d rounds x %d calls per arm, arms alternate, median (min .. max)" % (
        torch.__version__, torch.cuda.get_device_name(0), ROUNDS, REPS), file=out, flush=True)
    print("command: python tools/microbench/weight_avg_bench.py %s" % " ".join(args), file=out, flush=True)
    for w in workloads:
        one_workload(w, out)


if __name__ == "__main__":
    main()
