#!/usr/bin/env python3
"""Time of the fully-convolutional head's pooling kernels at the driver-monitoring shape: crop 112, 64 clips, slow res5
[64, 2, 7, 7, C], fast res5 [64, 16, 7, 7, C/8] (C = 2048 unless --channels says otherwise), window T x 3 x 3 ->
pooled [64, 1, 5, 5, C + C/8].
  forward:  sf_avgpool_win_fwd against sf_pool_fwd (the generic kernel, the only other route for this arithmetic) on the
            same views, both writing the pathway's slice of the concat buffer; the largest difference of the two
            results is printed beside the times
  backward: sf_avgpool_win_bwd, first-writer (overwrite) and accumulating, against its algorithmic bytes — dy once, dx
            written (read and written when accumulating) — at the achievable HBM rate, 6.3 TB/s
One res5 map is 51 MB and would stay in the 256 MiB Infinity Cache from launch to launch, so every timed launch works
on the next of ROT copies (ROT x 51 MB > the cache).  HEAD_POOL_ITERS launches each.
usage: tools/microbench/head_pool_bench.py [--channels C] [--batch N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import torch  # noqa: E402
import sfhip  # noqa: E402

ITERS = int(os.environ.get("HEAD_POOL_ITERS", "48"))
ROT = 8
HBM = 6.3e12


def timeit(fn, iters=ITERS):
    """fn(i) is launch i; returns microseconds per launch."""
    for i in range(ROT):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "head_pool_bench needs an MI355X"
    torch.manual_seed(0)
    N, total = a.batch, a.channels + a.channels // 8
    res = {"batch": N, "channels": [a.channels, a.channels // 8], "iters": ITERS, "rotating_copies": ROT}
    off = 0
    for tag, T, C in (("slow", 2, a.channels), ("fast", 16, a.channels // 8)):
        k = (T, 3, 3)
        xs = [sfhip.Act(torch.randn(N, T, 7, 7, C, device="cuda")) for _ in range(ROT)]
        cats = [sfhip.new_act("cuda", N, 1, 5, 5, total) for _ in range(ROT)]
        ref = sfhip.new_act("cuda", N, 1, 5, 5, total)
        sfhip.avgpool_window(xs[0], k, out=cats[0].slice(off, C))
        sfhip.pool(xs[0], k, (1, 1, 1), avg=True, out=ref.slice(off, C))
        diff = float((cats[0].buf[..., off:off + C] - ref.buf[..., off:off + C]).abs().max())
        x_bytes, y_bytes = xs[0].buf.numel() * 4, N * 25 * C * 4
        r = {"x_bytes": x_bytes, "pooled_bytes": y_bytes, "max_abs_diff_vs_pool_fwd": diff}
        r["fwd_us"] = timeit(lambda i: sfhip.avgpool_window(xs[i % ROT], k, out=cats[i % ROT].slice(off, C)))
        r["pool_fwd_us"] = timeit(lambda i: sfhip.pool(xs[i % ROT], k, (1, 1, 1), avg=True,
                                                       out=cats[i % ROT].slice(off, C)))
        r["fwd_floor_us"] = (x_bytes + y_bytes) / HBM * 1e6
        r["fwd_over_pool_fwd"] = r["fwd_us"] / r["pool_fwd_us"]
        dys = [sfhip.Act(torch.randn(N, 1, 5, 5, total, device="cuda")) for _ in range(ROT)]
        dxs = [sfhip.Act(torch.zeros_like(x.buf)) for x in xs]
        for name, over, nbytes in (("bwd_overwrite", True, y_bytes + x_bytes), ("bwd_accumulate", False,
                                                                               y_bytes + 2 * x_bytes)):
            r[name + "_us"] = timeit(lambda i: sfhip.avgpool_window_bwd(dys[i % ROT].slice(off, C), dxs[i % ROT], k,
                                                                        overwrite=over))
            r[name + "_floor_us"] = nbytes / HBM * 1e6
            r[name + "_over_floor"] = r[name + "_us"] / r[name + "_floor_us"]
        res[tag] = r
        off += C
    print(json.dumps(res))


if __name__ == "__main__":
    main()
