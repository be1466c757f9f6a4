#!/usr/bin/env python3
"""The one-pass backward of a frozen (eval-mode) BatchNorm, sf_bn_frozen_bwd, against the two calls it replaces on such
a layer — sf_bn_bwd_reduce + sf_bn_bwd_apply fed with the running statistics — at res2's shapes for one clip (Slow:
8 x 56 x 56 x 256, Fast: 32 x 56 x 56 x 32), byte-mask form, no residual and an accumulated one.  Bytes moved per
element: two-pass 2 x (dy + z + mask) + dz = 5 + 2/16 tensor passes, one-pass dy + z + mask + dz = 3 + 1/16 (each + 2
with an accumulated residual gradient).  usage: tools/microbench/bn_frozen_bench.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import torch  # noqa: E402
import sfhip  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = [(1, 8, 56, 56, 256), (1, 32, 56, 56, 32)]


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


print("%-22s %-9s %12s %12s %8s   (us; GB/s of algorithmic bytes)" % ("shape", "residual", "reduce+apply", "one pass", "ratio"))
for shp in SHAPES:
    n, t, h, w, c = shp
    z = sfhip.Act(torch.randn(*shp, device=dev))
    z0 = z.buf.clone()
    dy = sfhip.Act(torch.randn(*shp, device=dev))
    out = sfhip.Act(torch.empty(*shp, device=dev))
    dz = sfhip.Act(torch.empty(*shp, device=dev))
    dres = sfhip.Act(torch.zeros(*shp, device=dev))
    gamma, beta = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)
    mean, var = torch.randn(c, device=dev) * 0.1, torch.rand(c, device=dev) + 0.5
    invstd = torch.rsqrt(var + 1e-5)
    scale = gamma * invstd
    mk = {}
    sfhip.affine(z, scale, beta - mean * scale, relu=True, out=out, mask=mk)
    mask = mk["bytes"]
    dg, db = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
    nbytes = z.buf.numel() * 4
    for with_res in (False, True):
        r = dres if with_res else None

        def two():  # dz to its own buffer, so every repetition reads the same z
            sfhip.bn_bwd(dy, out, z, mean, invstd, gamma, True, dres=r, dz_out=dz, mask=mask)

        def one():
            sfhip.bn_frozen_bwd(dy, out, z, mean, invstd, gamma, True, dres=r, dz_out=dz, grads=(dg, db), mask=mask)

        t2, t1 = timed(two), timed(one)
        k2, k1 = 5.125 + (4 if with_res else 0) * 0.5, 3.0625 + (2 if with_res else 0)
        print("%-22s %-9s %6.1f/%-5.0f %6.1f/%-5.0f %8.2f" % (shp, "acc" if with_res else "none", t2 * 1e6,
                                                            k2 * nbytes / t2 / 1e9, t1 * 1e6, k1 * nbytes / t1 / 1e9,
                                                            t2 / t1))
    assert torch.equal(z.buf, z0)
