#!/usr/bin/env python3
"""Streaming cross-length attention (sf_xattn_fwd / sf_xattn_bwd) against the materialised path
(nonlocal_helper.materialised_attention) at the Nonlocal production shapes, 8 clips at 224^2:
  res3  N_q = 6272, N_k = 1568, d = dv = 256      res4  N_q = 1568, N_k = 392, d = dv = 512
  res3 unpooled  N_q = N_k = 6272, d = dv = 256 (--batch-unpooled clips: its score matrices are 157 MB each, twice)
Per path: forward and backward time (HIP events, --warmup untimed then the median of --reps) and the peak memory the
call allocates above its inputs.  usage: tools/microbench/xattn_bench.py [--batch 8] [--reps 5] [--warmup 2]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "efficient-slowfast_amd"))

import torch  # noqa: E402

import sfhip  # noqa: E402
from slowfast.models import engine, nonlocal_helper  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def run(name, B, thw_q, thw_k, d, path, warmup, reps):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1)
    mk = lambda thw, c: sfhip.Act((torch.randn((B,) + thw + (c,), generator=g) * 0.5).to(dev))
    theta, phi, gg = mk(thw_q, d), mk(thw_k, d), mk(thw_k, d)
    sm = float(d) ** -0.5
    attend = nonlocal_helper.dense_attention if path == "streaming" else nonlocal_helper.materialised_attention
    state = {}

    def fwd():
        state["t"] = engine.Tape()
        with torch.no_grad(), engine.taping(state["t"]):
            state["y"] = attend(theta, phi, gg, True, sm)

    def prep():
        t = state["t"]
        t.grad_of(state["y"]).buf.fill_(1e-3)
        for a in (theta, phi, gg):
            t.grad_of(a)

    def bwd():
        with torch.no_grad():
            for fn, _side in reversed(state["t"].ops):
                fn()

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fwd(); prep(); bwd()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    f = timed(fwd, warmup, reps)
    prep()
    b = timed(bwd, warmup, reps)  # gradients accumulate into the same buffers: same work every repetition
    nq = thw_q[0] * thw_q[1] * thw_q[2]
    nk = thw_k[0] * thw_k[1] * thw_k[2]
    print("%-14s B=%d Nq=%5d Nk=%5d d=%3d  %-12s fwd %8.3f ms (%.3f..%.3f)  bwd %8.3f ms (%.3f..%.3f)  peak extra "
          "%8.1f MiB" % (name, B, nq, nk, d, path, f[0], f[1], f[2], b[0], b[1], b[2], peak), flush=True)
    state.clear()
    torch.cuda.empty_cache()
    return f[0], b[0], peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batch-unpooled", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    print("device: %s; %d warm-up + %d timed repetitions per figure (median, min..max), HIP events; clocks as the "
          "machine sets them (not pinned)" % (torch.cuda.get_device_name(0), a.warmup, a.reps))
    shapes = (("res3", a.batch, (8, 28, 28), (8, 14, 14), 256), ("res4", a.batch, (8, 14, 14), (8, 7, 7), 512),
              ("res3-unpooled", a.batch_unpooled, (8, 28, 28), (8, 28, 28), 256))
    for name, B, tq, tk, d in shapes:
        r = {p: run(name, B, tq, tk, d, p, a.warmup, a.reps) for p in ("streaming", "materialised")}
        s, m = r["streaming"], r["materialised"]
        print("%-14s streaming / materialised: fwd x%.2f  bwd x%.2f  fwd+bwd x%.2f  memory x%.3f" % (
            name, s[0] / m[0], s[1] / m[1], (s[0] + s[1]) / (m[0] + m[1]), s[2] / m[2]), flush=True)


if __name__ == "__main__":
    main()
