#!/usr/bin/env python3
"""The training step's tail alone (tools/train_net.py:87-138 and :93-96): loss + top-k + NaN check + the three host
reads + zero + SGD, on the real parameter list of a workload through FlatGradients, with resident logits [N, K].

Arms (whole tail):
  torch, foreach SGD   F.cross_entropy + backward on the logits, metrics.topks_correct, math.isnan(loss.item()) and the
                       three .item() reads, FlatGradients.zero(), torch.optim.SGD (foreach) — the parent's route
  torch, fused SGD     the same with torch.optim.SGD(fused=True)
  hip tail             HipCrossEntropy + backward_direct, HipSGD.step(guard=, zero_grad=True): no host read, no zero pass
Arms (the update alone): torch foreach, torch fused, HipSGD, HipSGD with zero_grad.
Every arm sets a new learning rate in front of every call, as train_net.py:68-69 does (cosine is the default policy).
The update KERNEL's device time: REPS raw `sf_sgd_step` launches on the table HipSGD built, back to back between two
HIP events (the host issues a launch in far less than it runs), per launch; achieved bytes/s = p and buf read and
written, g read (+ g written with zero_grad) over that time.
Method: every arm warmed up, then ROUNDS rounds in which the arms alternate; an arm's round is REPS calls; "issue" is
the host clock until the last call returns, "total" until the device is idle (host clock between two device
synchronisations), both per call; the figure is the median round, the spread its min .. max.  Clocks not pinned.
Adam mode (`--adam`): the update alone on the workload's parameter list — torch.optim.Adam(foreach=True), torch.optim.Adam(
fused=True), HipAdam and HipAdam with zero_grad, a new learning rate in front of every call, same method; plus the
raw `sf_adam_step` call (step-count launch + update launch) by HIP events: p, m, v read and written, g read.
usage: tools/microbench/step_tail_bench.py [out.txt] [--adam] [workload ...]      (default: dual shufflenetv2; --adam: slowfast, the R50 parameter set)"""
import contextlib
import io
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd"), os.path.join(ROOT, "tests", "golden")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import bench  # noqa: E402
import sfhip  # noqa: E402
from slowfast.models.step_tail import HipAdam, HipCrossEntropy, HipSGD, StatsRing, adam_step, sgd_step  # noqa: E402
from slowfast.utils.distributed import FlatGradients  # noqa: E402
from slowfast.utils.meters import topks_correct  # noqa: E402

ROUNDS, REPS = 9, 5
SGD = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
ADAM = dict(lr=0.01, betas=(0.9, 0.999), weight_decay=1e-4)


def alternate(arms):
    for _, fn in arms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    issue = {n: [] for n, _ in arms}
    total = {n: [] for n, _ in arms}
    for _ in range(ROUNDS):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            issue[name].append((t1 - t0) / REPS)
            total[name].append((t2 - t0) / REPS)
    return issue, total


_LR = [0]


def new_lr(opt):
    """optim.set_lr with a value that differs from the last call's."""
    _LR[0] += 1
    lr = 0.01 * (1.0 + 0.001 * (_LR[0] % 97))
    for g in opt.param_groups:
        g["lr"] = lr


def kernel_time(opt, zero_grad, sgd_step=sgd_step):
    """Seconds per raw sf_sgd_step launch (or sf_adam_step call), one per round, by HIP events."""
    args = (opt._table, opt._table_dev, opt._chunks, opt._chunks_dev, opt._hyper, opt._hyper_dev, None, zero_grad)
    for _ in range(3):
        sgd_step(*args)
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(REPS):
            sgd_step(*args)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3 / REPS)
    return out


def fmt(v):
    return "%8.1f us (%7.1f .. %7.1f)" % (statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6)


def one_workload(workload, out):
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        cfg, model, batch, desc = bench.build(workload, dev)
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    N, K = batch, cfg.MODEL.NUM_CLASSES
    g = torch.Generator(device="cpu").manual_seed(1)
    logits = (torch.randn(N, K, generator=g) * 2).to(dev).requires_grad_(True)
    labels = torch.randint(0, K, (N,), generator=g).to(dev)
    topk = min(5, K)
    flat = FlatGradients(params)
    n = flat.flat.numel()
    fill = torch.randn(n, generator=g).to(dev) * 1e-3
    flat.flat.copy_(fill)
    opts = {"foreach": torch.optim.SGD(params, foreach=True, **SGD), "fused": torch.optim.SGD(params, fused=True, **SGD),
            "hip": HipSGD(params, **SGD)}
    loss_fun = HipCrossEntropy(topk, StatsRing(10))

    def torch_tail(opt):
        def fn():
            new_lr(opt)
            logits.grad = None
            loss = F.cross_entropy(logits, labels)
            if math.isnan(loss.item()):  # misc.check_nan_losses
                raise RuntimeError("nan")
            loss.backward()
            opt.step()
            correct = topks_correct(logits.detach(), labels, (1, topk))
            errs = [(1.0 - x / N) * 100.0 for x in correct]
            vals = (loss.item(), errs[0].item(), errs[1].item())
            flat.zero()  # the next step's zero pass
            return vals
        return fn

    def hip_tail():
        new_lr(opts["hip"])
        loss_fun(logits, labels)
        loss_fun.backward_direct(logits)
        opts["hip"].step(guard=loss_fun.guard, zero_grad=True)

    lines = ["== %s: %s; %d parameter tensors, %.2f M elements, logits [%d, %d]" % (
        workload, desc, len(params), n / 1e6, N, K)]
    # the share of the update's bytes on each load / store width, from the table HipSGD built
    opts["hip"].step()
    tab, chunks, C = opts["hip"]._table, opts["hip"]._chunks, sfhip.lib().sf_sgd_chunk_elems()
    wide = narrow = 0
    for ti, start in chunks.tolist():
        r = tab[ti].tolist()
        ln = min(C, r[3] - start)
        if all((a + 4 * start) % 16 == 0 for a in r[:3]):
            wide += ln
        else:
            narrow += ln
    first_odd = next((i for i, p in enumerate(params) if p.numel() % 4), None)
    lines.append("   update chunks: %d of %d elements; 16-byte path %.2f %% of the bytes, dword path %.2f %% (first "
                 "parameter with numel %% 4 != 0: #%s of %d)" % (len(chunks), C, 100.0 * wide / (wide + narrow),
                                                                100.0 * narrow / (wide + narrow), first_odd, len(params)))
    arms = [("torch, foreach SGD", torch_tail(opts["foreach"])), ("torch, fused SGD", torch_tail(opts["fused"])),
            ("hip tail", hip_tail)]
    issue, total = alternate(arms)
    lines.append("   whole tail                 issue (host)                        total (device idle)")
    for name, _ in arms:
        lines.append("   %-22s %s   %s" % (name, fmt(issue[name]), fmt(total[name])))
    flat.flat.copy_(fill)

    def update(opt, **kw):
        def fn():
            new_lr(opt)
            opt.step(**kw)
        return fn

    upd = [("torch foreach", update(opts["foreach"])), ("torch fused", update(opts["fused"])),
           ("HipSGD", update(opts["hip"])), ("HipSGD zero_grad", update(opts["hip"], zero_grad=True))]
    issue, total = alternate(upd)
    lines.append("   update alone (call)        issue (host)                        total (device idle)")
    for name, _ in upd:
        lines.append("   %-22s %s   %s" % (name, fmt(issue[name]), fmt(total[name])))
    lines.append("   update kernel (HIP events, raw launches)                       device time                  achieved")
    for name, z in (("sgd_step_kernel", False), ("sgd_step_kernel zero_grad", True)):
        flat.flat.copy_(fill)
        t = kernel_time(opts["hip"], z)
        lines.append("   %-58s %s   %6.2f TB/s" % (name, fmt(t), n * 4 * (6 if z else 5) / statistics.median(t) / 1e12))
    # the dword path's cost: the same list with gradients on 16 bytes everywhere (one allocation per gradient)
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    aligned = HipSGD(params, **SGD)
    aligned.step()
    t = kernel_time(aligned, False)
    lines.append("   %-58s %s   %6.2f TB/s" % ("sgd_step_kernel, every gradient on 16 bytes (own allocations)", fmt(t),
                                              n * 4 * 5 / statistics.median(t) / 1e12))
    for ln in lines:
        print(ln, file=out, flush=True)
        if out is not sys.stdout:
            print(ln, flush=True)


def adam_workload(workload, out):
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        cfg, model, batch, desc = bench.build(workload, dev)
    params = [p for p in model.parameters() if p.requires_grad]
    flat = FlatGradients(params)
    n = flat.flat.numel()
    g = torch.Generator(device="cpu").manual_seed(1)
    fill = torch.randn(n, generator=g).to(dev) * 1e-3
    flat.flat.copy_(fill)
    opts = {"foreach": torch.optim.Adam(params, foreach=True, **ADAM), "fused": torch.optim.Adam(params, fused=True, **ADAM),
            "hip": HipAdam(params, **ADAM)}

    def update(opt, **kw):
        def fn():
            new_lr(opt)
            opt.step(**kw)
        return fn

    lines = ["== %s (Adam): %s; %d parameter tensors, %.2f M elements" % (workload, desc, len(params), n / 1e6)]
    upd = [("torch foreach", update(opts["foreach"])), ("torch fused", update(opts["fused"])),
           ("HipAdam", update(opts["hip"])), ("HipAdam zero_grad", update(opts["hip"], zero_grad=True))]
    issue, total = alternate(upd)
    lines.append("   update alone (call)        issue (host)                        total (device idle)")
    for name, _ in upd:
        lines.append("   %-22s %s   %s" % (name, fmt(issue[name]), fmt(total[name])))
    lines.append("   sf_adam_step (HIP events, raw calls: step counts + update)     device time                  achieved")
    for name, z in (("adam_tick_kernel + adam_step_kernel", False), ("adam_tick_kernel + adam_step_kernel zero_grad", True)):
        flat.flat.copy_(fill)
        t = kernel_time(opts["hip"], z, adam_step)
        lines.append("   %-58s %s   %6.2f TB/s" % (name, fmt(t), n * 4 * (8 if z else 7) / statistics.median(t) / 1e12))
    for ln in lines:
        print(ln, file=out, flush=True)
        if out is not sys.stdout:
            print(ln, flush=True)


def main():
    args = [a for a in sys.argv[1:] if a != "--adam"]
    adam = "--adam" in sys.argv[1:]
    out = open(args[0], "w") if args and args[0].endswith(".txt") else sys.stdout
    workloads = [a for a in args if not a.endswith(".txt")] or (["slowfast"] if adam else ["dual", "shufflenetv2"])
    print("step_tail_bench: torch %s on %s; %d rounds x %d calls per arm, arms alternate, median (min .. max)" % (
        torch.__version__, torch.cuda.get_device_name(0), ROUNDS, REPS), file=out, flush=True)
    for w in workloads:
        (adam_workload if adam else one_workload)(w, out)


if __name__ == "__main__":
    main()
