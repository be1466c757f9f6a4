#!/usr/bin/env python3
"""The training telemetry alone, on the parameters of a workload (default: dual, the 8x8 R50 + CMDA model bench.py
times), and inside that workload's training step.

Arms:
  DeviceModelStats.record("param")   one sf_tensor_stats call (a partial per chunk, a row per tensor) behind the host's
                                     address check; every element read once, 4 bytes per element
  sf_tensor_stats alone              the native call on the tables the object built, no host work but the call
  one read of the parameters         torch.sum over ONE flat float32 tensor of the same size: what reading the bytes
                                     once costs in a single launch
  torch loop, per tensor             isfinite + count, min, max, sum, norm, count_nonzero, histc(49 linear bins): the
                                     same quantities up to the bins' shape, every result left on the device (no host
                                     sync), 8 small launches or more per tensor
  training step / step + record      bench.make_train_step's eager step, and the same step with record("grad") behind
                                     the backward and record("param") behind the optimizer
The arms of a group alternate.  Method: every arm warmed up, then ROUNDS rounds in which the arms alternate; an arm's round
is REPS calls between two HIP events, per call; the figure is the median round, the spread its min .. max.  Clocks not
pinned.
usage: tools/microbench/tensor_stats_bench.py [out.txt] [workload ...]"""
import contextlib
import io
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd"), os.path.join(ROOT, "tests", "golden"),
                os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import bench  # noqa: E402
import sfhip  # noqa: E402
from slowfast.utils import model_stats  # noqa: E402

ROUNDS, REPS = 9, 5


def alternate(arms, reps=REPS):
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
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e-3 / reps)
    return times


def fmt(v):
    return "%9.1f us (%8.1f .. %8.1f)" % (statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6)


def one_workload(workload, out):
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        cfg, model, batch, desc = bench.build(workload, dev)
    model.train()
    params = [p for p in model.parameters()]
    watch = model_stats.DeviceModelStats(model.named_parameters(), slots=8)
    watch.record("param")
    tab = watch._tabs["param"]
    n_elem = sum(p.numel() for p in params)
    flat = torch.randn((n_elem,), dtype=torch.float32, device=dev)
    keep = []

    def torch_loop():
        keep.clear()
        with torch.no_grad():
            for p in params:
                fin = torch.isfinite(p)
                keep.append((fin.numel() - fin.sum(), p.min(), p.max(), p.sum(dtype=torch.float64), p.norm(),
                             p.numel() - torch.count_nonzero(p), torch.histc(p, bins=49, min=-16.0, max=16.0)))

    native = alternate([
        ('DeviceModelStats.record("param")', lambda: watch.record("param")),
        ("sf_tensor_stats alone", lambda: sfhip.tensor_stats(tab.host, tab.dev, watch._chunks, watch._chunks_dev,
                                                             watch._ws["param"], watch.ring("param"), watch.cursor("param"))),
        ("one read of the parameters", lambda: flat.sum())])
    loop = alternate([("torch loop, per tensor", torch_loop)], reps=2)

    # inside the workload's training step
    clips = bench.synthetic_clips(cfg, batch, dev, 100)
    labels = torch.randint(0, cfg.MODEL.NUM_CLASSES, (batch,), device=dev,
                           generator=torch.Generator(device=dev).manual_seed(7))
    step, gflat, opt = bench.make_train_step(model, clips, labels)

    def watched():
        gflat.zero()
        loss = torch.nn.functional.cross_entropy(model([clips[0], clips[1]]), labels)
        loss.backward()
        gflat.all_reduce_mean()
        watch.record("grad")
        opt.step()
        gflat.rebind()
        watch.record("param")

    steps = alternate([("training step", step), ("training step + record(grad) + record(param)", watched)])

    lines = ["== %s: %s; %d tensors, %.2f M elements (%.1f MB), %d chunks, row %d x 8 B, workspace %.2f MB" % (
        workload, desc, len(watch.names), n_elem / 1e6, n_elem * 4 / 1e6, watch._chunks.shape[0], model_stats.ROW,
        watch._ws["param"].numel() * 8 / 1e6)]
    lines.append("   (HIP events)                                     per call")
    for times in (native, loop, steps):
        for name in times:
            lines.append("   %-46s %s" % (name, fmt(times[name])))
    m = {k: statistics.median(v) for t in (native, loop, steps) for k, v in t.items()}
    lines.append("   %.1f MB read once: record %.2f TB/s, the native call alone %.2f TB/s, torch.sum over one flat tensor "
                 "%.2f TB/s" % (n_elem * 4 / 1e6, n_elem * 4 / m['DeviceModelStats.record("param")'] / 1e12,
                                n_elem * 4 / m["sf_tensor_stats alone"] / 1e12,
                                n_elem * 4 / m["one read of the parameters"] / 1e12))
    lines.append("   sf_tensor_stats alone / one read of the parameters: %.2f x;  torch loop / record: %.1f x" % (
        m["sf_tensor_stats alone"] / m["one read of the parameters"],
        m["torch loop, per tensor"] / m['DeviceModelStats.record("param")']))
    a, b = m["training step"], m["training step + record(grad) + record(param)"]
    lines.append("   step with both recordings / step: %.4f x (%+.1f us); rebuilds %r" % (b / a, (b - a) * 1e6, watch.rebuilds))
    for ln in lines:
        print(ln, file=out, flush=True)
        if out is not sys.stdout:
            print(ln, flush=True)


def main():
    args = sys.argv[1:]
    out = open(args[0], "w") if args and args[0].endswith(".txt") else sys.stdout
    workloads = [a for a in args if not a.endswith(".txt")] or ["dual"]
    print("tensor_stats_bench: torch %s on %s; %d rounds x %d calls per arm, arms alternate, median (min .. max)" % (
        torch.__version__, torch.cuda.get_device_name(0), ROUNDS, REPS), file=out, flush=True)
    print("command: python tools/microbench/tensor_stats_bench.py %s" % " ".join(args), file=out, flush=True)
    for w in workloads:
        one_workload(w, out)


if __name__ == "__main__":
    main()
