#!/usr/bin/env python3
"""The "dot_product" Nonlocal block as SLOWFAST_NLN trains it, 8 clips at 224^2, train mode, through the public module
and the tape only (so the same file runs on any commit):
  res3  x [8, 512, 8, 28, 28],  pool (1,2,2), dim_inner 256   (N_q = 6272, N_k = 1568)
  res4  x [8, 1024, 8, 14, 14], pool (1,2,2), dim_inner 512   (N_q = 1568, N_k = 392)
One repetition = Nonlocal.run under a fresh tape plus the tape's backward (the four projections, the pool, the
attention and the final BN with their gradients).  --warmup untimed repetitions, then --reps timed ones, each between
two HIP events; median, min..max and the quartile spread.  Peak memory = torch.cuda.max_memory_allocated above what is
allocated before the first repetition (x, the parameters).
usage: tools/microbench/nonlocal_dot_bench.py [--batch 8] [--reps 30] [--warmup 5]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "efficient-slowfast_amd"))

import torch  # noqa: E402

import sfhip  # noqa: E402
from slowfast.models import engine  # noqa: E402
from slowfast.models.nonlocal_helper import Nonlocal  # noqa: E402


def run(name, B, dim, thw, dim_inner, warmup, reps):
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    blk = Nonlocal(dim, dim_inner, (1, 2, 2), instantiation="dot_product").to(dev).train()
    with torch.no_grad():
        blk.bn.weight.fill_(0.5)  # zero-initialised by default: a live scale keeps every gradient non-trivial
    g = torch.Generator(device="cpu").manual_seed(2)
    xa = sfhip.Act((torch.randn((B,) + thw + (dim,), generator=g) * 0.5).to(dev))
    dy = torch.full((B,) + thw + (dim,), 1e-3, dtype=torch.float32, device=dev)

    def step():
        t = engine.Tape()
        with torch.no_grad(), engine.taping(t):
            ya = blk.run(xa)
            t.grad_of(ya).buf.copy_(dy)
            t.grad_of(xa)
            t.backward()

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    q = statistics.quantiles(ms, n=4)
    nq = thw[0] * thw[1] * thw[2]
    print("%-5s B=%d Nq=%5d Nk=%5d d=%3d  fwd+bwd median %8.3f ms  (min %.3f, max %.3f, quartiles %.3f..%.3f)  peak "
          "extra %8.1f MiB" % (name, B, nq, nq // 4, dim_inner, statistics.median(ms), min(ms), max(ms), q[0], q[2],
                               peak), flush=True)
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    print("device: %s; %d warm-up + %d timed repetitions per shape, HIP events; clocks as the machine sets them (not "
          "pinned)" % (torch.cuda.get_device_name(0), a.warmup, a.reps), flush=True)
    run("res3", a.batch, 512, (8, 28, 28), 256, a.warmup, a.reps)
    run("res4", a.batch, 1024, (8, 14, 14), 512, a.warmup, a.reps)


if __name__ == "__main__":
    main()
