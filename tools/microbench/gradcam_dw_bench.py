#!/usr/bin/env python3
"""sf_dwconv_dgrad_epi (epilogue backward applied while dy is gathered, no dL/dz tensor) against the two-launch form it
replaces (sf_epilogue_bwd_act into a dL/dz tensor, then sf_dwconv_dgrad), on two depthwise layers of the efficient
backbones at crop 224, slow pathway, T = 4, one clip:
  mobilenetv2_s4   the stride-1 depthwise 3x3x3 + BN + ReLU6 of an InvertedResidual of SlowFastMoibleNetV2's s4
                   (6 x 32 = 192 channels at 28 x 28: the 6x-expanded tensor, the widest of the block)
  shufflenet_s3    conv2 + bn2 (no activation: scale only) of a stride-1 Bottleneck of SlowFastShuffleNet's s3
                   (GROUPS 1: 288 / 4 = 72 channels at 14 x 14)
Per shape: microseconds per call between device synchronisations (GRADCAM_DW_ITERS calls after 10 warm ones, the two
forms alternated GRADCAM_DW_ROUNDS times), the algorithmic HBM bytes of each form and the rate they imply, and the
max-norm relative difference of the two results.  One JSON line per shape.
usage: tools/microbench/gradcam_dw_bench.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import torch  # noqa: E402

ITERS = int(os.environ.get("GRADCAM_DW_ITERS", "200"))
ROUNDS = int(os.environ.get("GRADCAM_DW_ROUNDS", "3"))
K, P = (3, 3, 3), (1, 1, 1)
# name: (N, T, H, W, C, stride, relu)
SHAPES = {"mobilenetv2_s4": (1, 4, 28, 28, 192, (1, 1, 1), 6),
          "shufflenet_s3": (1, 4, 14, 14, 72, (1, 1, 1), False)}


def timeit(fn):
    """microseconds per call."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS * 1e6


def main():
    assert torch.cuda.is_available(), "gradcam_dw_bench needs an MI355X"
    import sfhip
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    for name, (N, T, H, W, C, s, relu) in SHAPES.items():
        To, Ho, Wo = T, (H - 1) // s[1] + 1, (W - 1) // s[2] + 1
        x = sfhip.Act(torch.empty(N, T, H, W, C, device=dev))
        dy = sfhip.Act(torch.randn(N, To, Ho, Wo, C, generator=g).to(dev))
        y = sfhip.Act((torch.randn(N, To, Ho, Wo, C, generator=g) * 4).clamp(0.0, 6.0).to(dev))
        wp = torch.zeros(27, (C + 15) // 16 * 16)
        wp[:, :C] = torch.randn(27, C, generator=g)
        wp = wp.to(dev)
        scale = (torch.rand(C, generator=g) + 0.5).to(dev)
        dx_f = sfhip.Act(torch.empty(N, T, H, W, C, device=dev))
        dx_t = sfhip.Act(torch.empty(N, T, H, W, C, device=dev))
        dz = sfhip.Act(torch.empty(N, To, Ho, Wo, C, device=dev))

        def fused():
            sfhip.dwconv_dgrad_epi(x, dy, y, wp, K, s, P, dx_f, scale=scale, relu=relu, accumulate=False)

        def two_launches():  # sf_dwconv_dgrad accumulates: the zero fill is part of the form
            sfhip.epilogue_bwd(dy, y, dz, scale=scale, act=relu)
            dx_t.buf.zero_()
            sfhip.dwconv_dgrad(x, dz, wp, K, s, P, dx_t)

        tf, tt = [], []
        for _ in range(ROUNDS):
            tf.append(timeit(fused))
            tt.append(timeit(two_launches))
        out_b, in_b = 4 * dy.rows * C, 4 * x.rows * C
        bytes_f = out_b * (2 if relu else 1) + in_b
        bytes_t = out_b * (2 if relu else 1) + out_b + out_b + in_b + 2 * in_b  # + dz written and read, dx zeroed and read
        diff = float((dx_f.buf - dx_t.buf).abs().max() / dx_t.buf.abs().max())
        print(json.dumps({
            "shape": name, "N_T_H_W_C": [N, T, H, W, C], "stride": list(s), "act": int(relu), "iters": ITERS,
            "fused_us": tf, "two_launch_us": tt, "fused_over_two_launch": min(tf) / min(tt),
            "fused_bytes": bytes_f, "two_launch_bytes": bytes_t,
            "fused_GBps": bytes_f / (min(tf) * 1e-6) / 1e9, "two_launch_GBps": bytes_t / (min(tt) * 1e-6) / 1e9,
            "max_rel_diff": diff}))


if __name__ == "__main__":
    main()
