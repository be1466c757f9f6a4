#!/usr/bin/env python3
"""sf_ctx_pool_fwd / sf_ctx_pool_bwd (ContextBlock3D's attention pooling in one pass over x) at the CMDA fusion shapes
of cfg #3 for one clip — (C, T, H, W) = (32, 32, 56, 56) and (128, 32, 14, 14) — against the composition of existing
entry points the block would otherwise be built from: sf_conv_fwd for the 1-channel mask, sf_row_softmax_fwd over the
positions, then the weighted sum through sf_gram.  An entry that refuses a step of the composition (sf_gram serves
widths in steps of 4, the mask has one channel) is named in the output; the composition's time is then the sum of the
steps that ran — a LOWER bound, since the refused step is the second read of x.
Byte model: the one-pass forward reads x once (4 * rows * C bytes); the composition reads x for the mask and again for
the weighted sum and passes three times over the logits (written, read + written by the softmax, read by the sum).
The backward reads x once and writes (or reads + writes) dx.
5 warm-up + 50 timed calls per figure between HIP events, clocks not pinned.  usage: tools/microbench/ctx_pool_bench.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import torch  # noqa: E402
import sfhip  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = [(32, 32, 56, 56), (128, 32, 14, 14)]


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def attempt(name, fn):
    """(seconds, None) of a step, or (0, reason) when its entry point refuses the shape."""
    try:
        fn()
        torch.cuda.synchronize()
    except (sfhip.SfhipError, AssertionError, RuntimeError) as e:  # (SfhipError is a RuntimeError; a size query of 0 too)
        return 0.0, "%s refused: %s" % (name, str(e).splitlines()[0][:120])
    return timed(fn), None


for C, T, H, W in SHAPES:
    rows = T * H * W
    x = sfhip.Act(torch.randn(1, T, H, W, C, device=dev))
    w = torch.randn(C, device=dev) / C ** 0.5
    b = torch.zeros(1, device=dev)
    xbytes = rows * C * 4
    t_one = timed(lambda: sfhip.ctx_pool(x, w, b))
    ctx, lse = sfhip.ctx_pool(x, w, b)
    dctx = torch.randn(1, C, device=dev)
    dx = sfhip.Act(torch.zeros(1, T, H, W, C, device=dev))
    t_bw = timed(lambda: sfhip.ctx_pool_bwd(x, w, b, lse, ctx, dctx, dx, accumulate=False))
    t_ba = timed(lambda: sfhip.ctx_pool_bwd(x, w, b, lse, ctx, dctx, dx, accumulate=True))
    # the composition
    wp = sfhip.pack_conv_weight(w.view(1, C, 1, 1, 1))
    logits = sfhip.conv(x, wp, (1, 1, 1), bias=b)                      # [1, T, H, W, 1]
    flat = sfhip.Act(logits.buf.view(1, 1, 1, 1, rows))                # the positions as one softmax row
    pcol = sfhip.Act(logits.buf.view(1, T, H, W, 1))
    steps = [("sf_conv_fwd (mask)", lambda: sfhip.conv(x, wp, (1, 1, 1), bias=b, out=logits)),
             ("sf_row_softmax_fwd", lambda: sfhip.row_softmax(flat)),
             ("sf_gram (weighted sum)", lambda: sfhip.gram(pcol, x, 1.0))]
    total, notes = 0.0, []
    parts = []
    for name, fn in steps:
        t, why = attempt(name, fn)
        total += t
        parts.append("%s %.1f us" % (name, t * 1e6) if why is None else why)
        if why:
            notes.append(why)
    print("C %d, %d positions (%.1f MB):" % (C, rows, xbytes / 1e6))
    print("  one pass  forward  %7.1f us  (%5.0f GB/s of one read of x; byte model: 1 read of x)" % (
        t_one * 1e6, xbytes / t_one / 1e9))
    print("  one pass  backward %7.1f us first writer (%5.0f GB/s of x read + dx written), %7.1f us accumulating" % (
        t_bw * 1e6, 2 * xbytes / t_bw / 1e9, t_ba * 1e6))
    print("  composition forward %s %7.1f us  (byte model: 2 reads of x + 3 passes over the logits)" % (
        ">=" if notes else "  ", total * 1e6))
    for p in parts:
        print("      " + p)
    print("  forward ratio composition / one pass: %s%.2f" % (">= " if notes else "", total / t_one))
