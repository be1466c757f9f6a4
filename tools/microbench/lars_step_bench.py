#!/usr/bin/env python3
"""The large-batch optimizers alone, on the real parameter list of a workload through FlatGradients (default: dual, the
8x8 R50 + CMDA model bench.py times).

Arms (the whole `step()`, as a training loop issues it, the learning rate changing in front of every call so that the
hyper-parameter upload is part of it):
  HipAdam / HipAdamW            sf_adam_step / sf_adamw_step: the same traffic (p, g, m, v read, p, m, v written)
  torch AdamW foreach           torch.optim.AdamW(foreach=True)
  HipSGD                        sf_sgd_step with momentum: 5 array passes (p, g, buf read; p, buf written)
  HipLARS                       sf_lars_ratios (p and g read once more: 2 array passes) + sf_lars_sgd_step; by traffic
                                7 / 5 = 1.4 x HipSGD
  wrapper + torch SGD foreach   tests/_lars_ref.py (two norms per tensor read back on the host, as written there) around
                                torch.optim.SGD(foreach=True)
and the native calls alone on the tables those objects built (sf_adam_step, sf_adamw_step, sf_sgd_step, and HipLARS's
two: sf_lars_ratios with both of its launches, sf_lars_sgd_step), with the bytes/s they achieve: the step() figures
include the host side of the call (372 addresses compared, the hyper-parameter upload), the native ones do not.  The
Hip arms alternate among themselves and torch's arms among themselves.
Method: every arm warmed up, then ROUNDS rounds in which the arms alternate; an arm's round is REPS calls between two
HIP events, per call; the figure is the median round, the spread its min .. max.  Clocks not pinned.
usage: tools/microbench/lars_step_bench.py [out.txt] [workload ...]"""
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
from _lars_ref import LarsRef  # noqa: E402
from slowfast.models.step_tail import (HYP_ROW, LARS_HYP_ROW, ST_GUARD, HipAdam, HipAdamW, HipLARS, HipSGD,  # noqa: E402
                                       lars_ratios, lars_sgd_step)
from slowfast.utils.distributed import FlatGradients  # noqa: E402

ROUNDS, REPS = 9, 5
SGD_KW = dict(momentum=0.9, weight_decay=1e-4)
LARS_KW = dict(trust_coefficient=0.02, clip=True, eps=1e-8)


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


def scheduled(opt, base):
    """opt.step() behind a learning rate that differs from the last call's."""
    state = {"i": 0}

    def fn():
        state["i"] += 1
        lr = base * (1.0 + 0.001 * (state["i"] % 7))
        for g in opt.param_groups:
            g["lr"] = lr
        opt.step()
    return fn


def one_workload(workload, out):
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        cfg, model, batch, desc = bench.build(workload, dev)
    params = [p for p in model.parameters() if p.requires_grad]
    flat = FlatGradients(params)
    n = flat.flat.numel()
    g = torch.Generator(device="cpu").manual_seed(1)
    fill = torch.randn(n, generator=g).to(dev) * 1e-3
    p0 = [p.detach().clone() for p in params]

    def reset():
        flat.flat.copy_(fill)
        with torch.no_grad():
            for p, q in zip(params, p0):
                p.copy_(q)

    reset()
    adam, adamw = HipAdam(params, lr=1e-5, weight_decay=1e-2), HipAdamW(params, lr=1e-5, weight_decay=1e-2)
    sgd, lars = HipSGD(params, lr=1e-4, **SGD_KW), HipLARS(params, lr=1e-4, **SGD_KW, **LARS_KW)
    hip = [("HipAdam", adam, 1e-5), ("HipAdamW", adamw, 1e-5), ("HipSGD", sgd, 1e-4), ("HipLARS", lars, 1e-4)]
    th = alternate([(name, scheduled(opt, lr)) for name, opt, lr in hip])
    assert float(lars.guard.cpu()[0]) == 0.0 and bool(torch.isfinite(lars.ratios).all())
    # the native calls alone on the tables the objects built (no host work but the call itself): what the device does
    reset()

    def native(opt):
        return lambda: opt._launch(opt._table, opt._table_dev, opt._chunks, opt._chunks_dev, opt._hyper, opt._hyper_dev,
                                   None, False)
    G = len(lars.param_groups)
    k = G * HYP_ROW
    lh, ld = lars._hyper[0, k:].view(G + 1, LARS_HYP_ROW), lars._hyper_dev[0, k:].view(G + 1, LARS_HYP_ROW)
    sh, sd = lars._hyper[0, :k].view(G, HYP_ROW), lars._hyper_dev[0, :k].view(G, HYP_ROW)
    raw_arms = [("sf_adam_step", native(adam), 7), ("sf_adamw_step", native(adamw), 7), ("sf_sgd_step", native(sgd), 5),
                ("sf_lars_ratios (2 launches)",
                 lambda: lars_ratios(lars._lars_table, lars._lars_table_dev, lars._chunks, lars._chunks_dev, lh, ld,
                                     lars._partials, lars._ratios, lars._lars_state), 2),
                ("sf_lars_sgd_step",
                 lambda: lars_sgd_step(lars._table, lars._table_dev, lars._chunks, lars._chunks_dev, sh, sd, lars._ratios,
                                       guard=lars._lars_state[ST_GUARD:ST_GUARD + 1]), 5)]
    raw = alternate([(name, fn) for name, fn, _ in raw_arms])
    # torch's own path, in rounds of its own: its host-bound calls leave the GPU idle and its clocks low for whatever runs next
    reset()
    t_adamw = torch.optim.AdamW(params, lr=1e-5, weight_decay=1e-2, foreach=True)
    wrapper = LarsRef(torch.optim.SGD(params, lr=1e-4, foreach=True, **SGD_KW), **LARS_KW)
    tt = alternate([("torch AdamW foreach", scheduled(t_adamw, 1e-5)),
                    ("wrapper + torch SGD foreach", scheduled(wrapper, 1e-4))])
    lines = ["== %s: %s; %d parameter tensors, %.2f M elements (%.1f MB), %d chunks" % (
        workload, desc, len(params), n / 1e6, n * 4 / 1e6, lars._chunks.shape[0])]
    lines.append("   step() (HIP events)              per call")
    for times in (th, tt):
        for name in times:
            lines.append("   %-30s %s" % (name, fmt(times[name])))
    lines.append("   native calls alone (HIP events)  per call                       achieved")
    for name, _, passes in raw_arms:
        lines.append("   %-30s %s   %6.2f TB/s (%d array passes)" % (
            name, fmt(raw[name]), passes * n * 4 / statistics.median(raw[name]) / 1e12, passes))
    m = {k_: statistics.median(v) for t in (th, tt, raw) for k_, v in t.items()}
    lines.append("   step():  HipAdamW / HipAdam %.3f x (expected 1: the same traffic);  HipLARS / HipSGD %.3f x (expected "
                 "about 1.4: 7 array passes against 5)" % (m["HipAdamW"] / m["HipAdam"], m["HipLARS"] / m["HipSGD"]))
    lines.append("   native:  sf_adamw_step / sf_adam_step %.3f x;  (sf_lars_ratios + sf_lars_sgd_step) / sf_sgd_step %.3f x" % (
        m["sf_adamw_step"] / m["sf_adam_step"],
        (m["sf_lars_ratios (2 launches)"] + m["sf_lars_sgd_step"]) / m["sf_sgd_step"]))
    lines.append("   torch AdamW foreach / HipAdamW: %.2f x;  wrapper + torch SGD foreach / HipLARS: %.2f x" % (
        m["torch AdamW foreach"] / m["HipAdamW"], m["wrapper + torch SGD foreach"] / m["HipLARS"]))
    for ln in lines:
        print(ln, file=out, flush=True)
        if out is not sys.stdout:
            print(ln, flush=True)


def main():
    args = sys.argv[1:]
    out = open(args[0], "w") if args and args[0].endswith(".txt") else sys.stdout
    workloads = [a for a in args if not a.endswith(".txt")] or ["dual"]
    print("lars_step_bench: torch %s on %s; %d rounds x %d calls per arm, arms alternate, median (min .. max)" % (
        torch.__version__, torch.cuda.get_device_name(0), ROUNDS, REPS), file=out, flush=True)
    print("command: python tools/microbench/lars_step_bench.py %s" % " ".join(args), file=out, flush=True)
    for w in workloads:
        one_workload(w, out)


if __name__ == "__main__":
    main()
