#!/usr/bin/env python3
"""Forward / backward time of ResNetRoIHead's kernels at the AVA shape: 8 clips at 224^2, slow res5 [8, 8, 14, 14, 2048],
fast res5 [8, 32, 14, 14, 256], 32 boxes, R = 7 (sf_roi_tpool_fwd + sf_roi_align_max_fwd per pathway; the backward is
sf_roi_align_max_bwd per pathway, which writes dL/d(res5) for every frame).  The floor is the traffic of the temporal
pool: it reads both res5 maps (154 MB), and the backward writes as much; at ~6.3 TB/s that is ~24 us each way.
ROI_ITERS launches each.
usage: tools/microbench/roi_head_bench.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import torch  # noqa: E402
import sfhip  # noqa: E402

ITERS = int(os.environ.get("ROI_ITERS", "20"))
HBM = 6.3e12


def timeit(fn, iters=ITERS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def main():
    torch.manual_seed(0)
    N, K, R, scale = 8, 32, 7, 1.0 / 16
    shapes = [(8, 2048), (32, 256)]
    xs = [sfhip.Act(torch.randn(N, T, 14, 14, C, device="cuda")) for T, C in shapes]
    g = torch.Generator().manual_seed(1)
    xy = torch.rand(K, 2, generator=g) * 160
    wh = torch.rand(K, 2, generator=g) * 120 + 16
    boxes = torch.cat([(torch.arange(K) % N).float().view(K, 1), xy, xy + wh], 1).cuda()
    total = sum(C for _, C in shapes)
    cat = sfhip.new_act("cuda", K, 1, 1, 1, total)
    args, res = [], {}

    def fwd():
        args.clear()
        off = 0
        for x in xs:
            pooled = sfhip.roi_tpool(x)
            args.append(sfhip.roi_align_max(pooled, boxes, R, scale, True, out=cat.slice(off, x.C)))
            off += x.C

    dxs = [sfhip.Act(torch.empty_like(x.buf)) for x in xs]
    dy = sfhip.Act(torch.randn(K, 1, 1, 1, total, device="cuda"))

    def bwd():
        off = 0
        for x, arg, dx in zip(xs, args, dxs):
            sfhip.roi_align_max_bwd(dy.slice(off, x.C), arg, boxes, R, scale, True, dx, accumulate=False)
            off += x.C

    fwd()
    nbytes = sum(x.buf.numel() * 4 for x in xs)
    res["fwd_us"] = timeit(fwd)
    res["bwd_us"] = timeit(bwd)
    res["tpool_us"] = timeit(lambda: [sfhip.roi_tpool(x) for x in xs])
    res["floor_us"] = nbytes / HBM * 1e6
    res["res5_bytes"] = nbytes
    res["fwd_over_floor"] = res["fwd_us"] / res["floor_us"]
    res["bwd_over_floor"] = res["bwd_us"] / res["floor_us"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
