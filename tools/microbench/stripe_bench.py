#!/usr/bin/env python3
"""sf_stripe_pool_fwd, sf_stripe_add_fwd and sf_stripe_pool_bwd (Stripe_NonLocalBlock's activation-sized passes) beside
the two existing memory-bound kernels of the same kind — sf_sample_affine_fwd (one read and one write of x, the bytes
sf_stripe_add_fwd moves) and sf_tmax_mean (one read of x, the bytes the pooling moves) — at a res2-sized Slow tensor
[8, 8, 56, 56, 256] with S = 7 stripes (205.5 MB: a read and a write pass together exceed the 256 MB Infinity Cache).

Byte model, computed from the shape: pooling = one read of x; add = one read + one write; backward first-writer = one
read of dz + one write of dx, accumulating = + one read of dx.  The [N, T, S, C] vectors are 0.03 % of x and are left out.
Method: every kernel warmed up 3 times, then ROUNDS rounds in which the kernels alternate, each timed over REPS calls
between HIP events (a round of one kernel is >= 10 ms); the figure is the median round, the spread its min .. max.
Clocks not pinned.  usage: tools/microbench/stripe_bench.py [out.txt]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import torch  # noqa: E402
import sfhip  # noqa: E402

N, T, H, W, C, S = 8, 8, 56, 56, 256, 7
ROUNDS, REPS = 7, 20


def main():
    assert torch.cuda.is_available(), "stripe_bench.py measures on an MI355X: no GPU, no figure"
    dev = torch.device("cuda:0")
    x = sfhip.Act(torch.randn(N, T, H, W, C, device=dev))
    dz = sfhip.Act(torch.randn(N, T, H, W, C, device=dev))
    out = sfhip.new_act(x, N, T, H, W, C)
    v = sfhip.Act(torch.randn(N, T, S, 1, C, device=dev))
    dmm = sfhip.Act(torch.randn(N, T, S, 1, 2 * C, device=dev))
    add = torch.randn(N, C, device=dev)
    _, arg = sfhip.stripe_pool(x, S, "max")
    xb = N * T * H * W * C * 4
    kernels = [
        ("sf_tmax_mean (yardstick: 1 read)", xb, lambda: sfhip.tmax_mean(x, 1)),
        ("sf_stripe_pool_fwd mean", xb, lambda: sfhip.stripe_pool(x, S, "mean")),
        ("sf_stripe_pool_fwd meanmax", xb, lambda: sfhip.stripe_pool(x, S, "meanmax")),
        ("sf_stripe_pool_fwd sum", xb, lambda: sfhip.stripe_pool(dz, S, "sum")),
        ("sf_sample_affine_fwd (yardstick: 1 read + 1 write)", 2 * xb, lambda: sfhip.sample_affine(x, add=add, out=out)),
        ("sf_stripe_add_fwd", 2 * xb, lambda: sfhip.stripe_add(x, v, out=out)),
        ("sf_stripe_pool_bwd first writer", 2 * xb,
         lambda: sfhip.stripe_pool_bwd(out, S, dz=dz, dmean=dmm.slice(0, C), dmax=dmm.slice(C, C), arg=arg,
                                       accumulate=False)),
        ("sf_stripe_pool_bwd accumulating", 3 * xb,
         lambda: sfhip.stripe_pool_bwd(out, S, dz=dz, dmean=dmm.slice(0, C), dmax=dmm.slice(C, C), arg=arg,
                                       accumulate=True)),
    ]
    for _, _, fn in kernels:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in kernels}
    for _ in range(ROUNDS):
        for name, _, fn in kernels:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / REPS * 1e-3)
    lines = ["x [%d, %d, %d, %d, %d] fp32 = %.1f MB, S = %d; median of %d alternating rounds of %d calls (min .. max)" % (
        N, T, H, W, C, xb / 1e6, S, ROUNDS, REPS)]
    gbs = {}
    for name, nbytes, _ in kernels:
        ts = times[name]
        med = statistics.median(ts)
        gbs[name] = nbytes / med / 1e9
        lines.append("%-52s %8.1f us (%7.1f .. %7.1f)  %6.0f GB/s of %5.1f MB" % (
            name, med * 1e6, min(ts) * 1e6, max(ts) * 1e6, gbs[name], nbytes / 1e6))
    names = [k[0] for k in kernels]
    for name in names[1:4]:
        lines.append("ratio %-46s %.2f of sf_tmax_mean" % (name, gbs[name] / gbs[names[0]]))
    for name in names[5:]:
        lines.append("ratio %-46s %.2f of sf_sample_affine_fwd" % (name, gbs[name] / gbs[names[4]]))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
