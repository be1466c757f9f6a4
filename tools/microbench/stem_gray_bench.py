#!/usr/bin/env python3
"""Forward and weight gradient of the stems of a grayscale clip: 8 clips at 112 x 112, the Fast stem (5x7x7, 1 -> 8,
T = 16) and the Slow stem (1x7x7, 1 -> 64, T = 2).

  stem_gray_bench.py            the one-channel route: sf_ncthw1_pack, sf_stem1_fwd, sf_stem1_wgrad
  stem_gray_bench.py --padded   the padded route a one-channel tensor took before those kernels existed: channels
                                padded to 4 (sf_ncthw_to_ndhwc), the stem-trick conv (kT,7,1) over pixels of 8 floats,
                                the generic weight gradient.  Uses only calls that exist on both sides of the change,
                                so it also runs from a checkout of the earlier commit.

HIP events around ITERS back-to-back launches after WARM warm-up launches, median of 5 rounds; the layout pass is
timed on its own (the input step writes the layout directly, the model pays it only for dense tensors)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "efficient-slowfast_amd"))
import sfhip  # noqa: E402

WARM, ITERS, ROUNDS = 10, 50, 5
STEMS = [("fast 5x7x7 1->8  T16", 8, 5, 16), ("slow 1x7x7 1->64 T2 ", 64, 1, 2)]
N, S = 8, 112


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return sorted(res)[len(res) // 2]


def main():
    padded = "--padded" in sys.argv[1:]
    dev = torch.device("cuda:0")
    print("%s route, %d clips, %dx%d, us per launch (median of %d x %d)" % (
        "padded (4-channel)" if padded else "one-channel", N, S, S, ROUNDS, ITERS))
    for name, cout, kT, T in STEMS:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(N, 1, T, S, S, generator=g).to(dev)
        w = (torch.randn(cout, 1, kT, 7, 7, generator=g) * 0.1).to(dev)
        pT, ph, pw, wp = kT // 2, 3, 3, S + 6
        dz = sfhip.Act(torch.randn(N, T, S // 2, S // 2, cout, generator=g).to(dev))
        if padded:
            t_pack = timed(lambda: sfhip.from_ncthw(x, cpad=4, ph=ph, pw=pw, wp=wp))
            abuf = sfhip.from_ncthw(x, cpad=4, ph=ph, pw=pw, wp=wp).buf
            view = sfhip.Act(abuf.view(N, T, S + 2 * ph, wp // 2, 8))
            w4 = torch.zeros((cout, 4, kT, 7, 7), device=dev)
            w4[:, :1] = w
            wpk = torch.zeros((cout, kT * 7, 32), device=dev)
            wpk[:, :, :28] = w4.permute(0, 2, 3, 4, 1).reshape(cout, kT * 7, 28)
            k, s, p = (kT, 7, 1), (1, 2, 1), (pT, 0, 0)
            thw = (T, S // 2, S // 2)
            t_fwd = timed(lambda: sfhip.conv(view, wpk, k, s, p, cin=28, out_thw=thw))
            t_wg = timed(lambda: sfhip.conv_wgrad(view, dz, cout, k, s, p, (1, 1, 1), cin=28, cin_pad=32))
            mb = abuf.numel() * 4 / 1e6
        else:
            t_pack = timed(lambda: sfhip.ncthw1_pack(x, ph, pw, wp))
            buf = sfhip.ncthw1_pack(x, ph, pw, wp)
            t_fwd = timed(lambda: sfhip.stem1_fwd(buf, w, pT))
            t_wg = timed(lambda: sfhip.stem1_wgrad(buf, dz, kT, pT))
            mb = buf.numel() * 4 / 1e6
        print("%s  layout %7.1f  forward %7.1f  weight gradient %7.1f   (packed clip %.1f MB)" % (
            name, t_pack, t_fwd, t_wg, mb))


if __name__ == "__main__":
    main()
