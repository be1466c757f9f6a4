"""Op-level parity of the fully-convolutional head's pooling kernels — sfhip.avgpool_window (sf_avgpool_win_fwd) and
sfhip.avgpool_window_bwd (sf_avgpool_win_bwd) — through the C ABI against torch.nn.functional.avg_pool3d and its
autograd in float64 on the CPU, on the same fp32 inputs.

Views are channel slices of wider buffers as in tests/test_elementwise_views_gpu.py: inputs sit between NaN channels,
outputs between sentinel channels that must come back bit for bit, a view a kernel overwrites starts as NaN.

Bound (the one test_elementwise_views_gpu.py holds average pooling to): |got - ref| <= (taps + 2) * 2^-24 * mag per
element.  Forward: mag = sum |x_window| / taps (taps - 1 additions, the reciprocal, the product; summing the frames
first and the plane second keeps the count).  Backward: at most taps windows hold an element, so the same count with
mag = sum |dy| / taps over those windows; accumulating adds one rounding of |base| + |gradient|, which
(taps + 2) * 2^-24 * (|base| + mag) still covers.

Shapes are the smallest at which a branch can go wrong: To = 1 (one sum stored to every frame) and To = 2, unequal
Ho / Wo, a non-cubic window, window == extent, the scalar kernels (C = 6, and an offset no float4 can address), more
than one channel block with a ragged last one (C = 72 / 70) and more than one backward workgroup, and the two plane
sizes either side of the 2048-position limit of the float4 LDS plane (the larger takes sf_pool_fwd's kernel)."""
import pytest
import torch

import _elementwise_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")

# name: (N, T, H, W, C), window, x view (coff, pitch), out / dy view (coff, pitch)
CASES = {
    "head_N2T2H4W4C8_k222": ((2, 2, 4, 4, 8), (2, 2, 2), (0, 8), (0, 8)),
    "to2_T3H5W4_k233": ((2, 3, 5, 4, 8), (2, 3, 3), (0, 8), (0, 8)),
    "noncubic_k123": ((2, 2, 4, 4, 8), (1, 2, 3), (0, 8), (0, 8)),
    "window_is_extent": ((2, 2, 4, 4, 8), (2, 4, 4), (0, 8), (0, 8)),
    "scalar_C6": ((2, 2, 4, 4, 6), (2, 2, 2), (0, 6), (1, 9)),
    "scalar_C8_coff2": ((2, 2, 4, 4, 8), (2, 2, 2), (2, 12), (4, 16)),
    "slice_cs16_coff4_to_coff8_of_24": ((2, 2, 4, 4, 8), (2, 2, 2), (4, 16), (8, 24)),
    "blocks_C72": ((2, 2, 5, 4, 72), (2, 3, 2), (4, 80), (4, 80)),
    "blocks_scalar_C70": ((2, 3, 5, 4, 70), (2, 3, 2), (1, 72), (0, 70)),
    "plane_2048_lds": ((1, 2, 32, 64, 4), (2, 2, 2), (0, 4), (4, 8)),
    "plane_2112_generic": ((1, 2, 33, 64, 4), (2, 2, 2), (0, 4), (4, 8)),
}
_refs = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _gen(name):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)


def _case(name):
    """Inputs and float64 references of one case, computed once: x, dy, base (what dx holds before an accumulate),
    out / its mag, dx / its mag."""
    if name not in _refs:
        import torch.nn.functional as F
        shape, k, _, _ = CASES[name]
        g = _gen(name)
        x = torch.randn(*shape, generator=g)
        out, out_mag = R.pool_ref(x, k, (1, 1, 1), (0, 0, 0), True)
        dy = torch.randn(*out.shape, generator=g)
        base = torch.randn(*shape, generator=g)

        def pulled_back(v):
            leaf = torch.zeros(shape, dtype=torch.float64).requires_grad_(True)
            F.avg_pool3d(R.to_ncthw(leaf), k, 1).backward(R.to_ncthw(v.double()))
            return leaf.grad

        _refs[name] = dict(x=x, dy=dy, base=base, out=out, out_mag=out_mag, dx=pulled_back(dy),
                           dx_mag=pulled_back(dy.abs()))
    return _refs[name]


def _report(name, err):
    from test_backward_ops_gpu import _report as report
    report(name, err, "elementwise_report.txt")


@pytest.mark.parametrize("name", list(CASES))
def test_avgpool_window_forward(name):
    import sfhip
    dev = _dev()
    shape, k, x_view, out_view = CASES[name]
    c = _case(name)
    taps = k[0] * k[1] * k[2]
    assert tuple(c["out"].shape) == (shape[0], shape[1] - k[0] + 1, shape[2] - k[1] + 1, shape[3] - k[2] + 1, shape[4])
    xa = R.view(dev, c["x"], x_view[0], x_view[1], NAN)
    oa = R.view(dev, torch.full(c["out"].shape, NAN), out_view[0], out_view[1], R.SENTINEL)
    ret = sfhip.avgpool_window(xa, k, out=oa)
    torch.cuda.synchronize()
    assert ret is oa
    got = R.inside(oa)
    r = R.rounds(got, c["out"], c["out_mag"])
    _report("avgpool_window/" + name, r)
    print("%-36s forward %.2f roundings (bound %d)" % (name, r, taps + 2))
    assert r <= taps + 2
    assert out_view == (0, shape[4]) or R.outside_is(oa)
    assert torch.equal(R.inside(xa), c["x"])
    if name == "window_is_extent":  # E = 1: the mean over T, H, W
        assert tuple(got.shape) == (shape[0], 1, 1, 1, shape[4])
        mean = c["x"].double().mean((1, 2, 3), keepdim=True)
        assert R.rounds(got, mean, c["x"].double().abs().mean((1, 2, 3), keepdim=True)) <= taps + 2
    again = R.view(dev, torch.full(c["out"].shape, NAN), out_view[0], out_view[1], R.SENTINEL)
    sfhip.avgpool_window(xa, k, out=again)
    torch.cuda.synchronize()
    assert torch.equal(R.inside(again).view(torch.int32), got.view(torch.int32)), "two runs differ"


def test_avgpool_window_allocates_its_output():
    import sfhip
    dev = _dev()
    name = "head_N2T2H4W4C8_k222"
    c = _case(name)
    out = sfhip.avgpool_window(R.view(dev, c["x"], 4, 16, NAN), CASES[name][1])
    torch.cuda.synchronize()
    assert (out.coff, out.C, out.cs) == (0, 8, 8) and tuple(out.buf.shape) == tuple(c["out"].shape)
    assert R.rounds(R.inside(out), c["out"], c["out_mag"]) <= 10


def test_two_pathways_share_the_concat_buffer():
    """C = 8 read from (pitch 16, offset 4) into channels [8, 16) of a 24-channel sentinel buffer; a second pathway
    (C = 8, dense) then fills [0, 8).  Each call leaves the other slice and channels [16, 24) as they were."""
    import sfhip
    dev = _dev()
    a, b = _case("slice_cs16_coff4_to_coff8_of_24"), _case("head_N2T2H4W4C8_k222")
    k = (2, 2, 2)
    cat = sfhip.Act(torch.full(tuple(a["out"].shape[:4]) + (24,), R.SENTINEL).to(dev))
    sfhip.avgpool_window(R.view(dev, a["x"], 4, 16, NAN), k, out=cat.slice(8, 8))
    torch.cuda.synchronize()
    first = cat.buf.cpu()
    assert R.rounds(first[..., 8:16], a["out"], a["out_mag"]) <= 10
    rest = torch.cat([first[..., :8], first[..., 16:]], -1)
    assert torch.equal(rest.view(torch.int32), torch.full_like(rest, R.SENTINEL).view(torch.int32))
    sfhip.avgpool_window(R.view(dev, b["x"], 0, 8, NAN), k, out=cat.slice(0, 8))
    torch.cuda.synchronize()
    second = cat.buf.cpu()
    assert R.rounds(second[..., :8], b["out"], b["out_mag"]) <= 10
    assert torch.equal(second[..., 8:16].view(torch.int32), first[..., 8:16].view(torch.int32)), "first slice changed"
    tail = second[..., 16:]
    assert torch.equal(tail.view(torch.int32), torch.full_like(tail, R.SENTINEL).view(torch.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_avgpool_window_backward(name):
    """overwrite=True into a NaN-filled dx: all finite and correct; overwrite=False adds to known contents; two runs
    are bitwise equal.  dy sits in the out view's slice, dx in the x view's."""
    import sfhip
    dev = _dev()
    shape, k, x_view, out_view = CASES[name]
    c = _case(name)
    taps = k[0] * k[1] * k[2]
    dya = R.view(dev, c["dy"], out_view[0], out_view[1], NAN)
    runs = []
    for _ in range(2):
        dxa = R.view(dev, torch.full(shape, NAN), x_view[0], x_view[1], R.SENTINEL)
        ret = sfhip.avgpool_window_bwd(dya, dxa, k, overwrite=True)
        torch.cuda.synchronize()
        assert ret is dxa
        runs.append(R.inside(dxa))
        assert x_view == (0, shape[4]) or R.outside_is(dxa)
    assert bool(torch.isfinite(runs[0]).all())
    r = R.rounds(runs[0], c["dx"], c["dx_mag"])
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two runs differ"
    acc = R.view(dev, c["base"], x_view[0], x_view[1], R.SENTINEL)
    sfhip.avgpool_window_bwd(dya, acc, k, overwrite=False)
    torch.cuda.synchronize()
    r_acc = R.rounds(R.inside(acc), c["base"].double() + c["dx"], c["base"].double().abs() + c["dx_mag"])
    _report("avgpool_window_bwd/" + name, max(r, r_acc))
    print("%-36s backward %.2f / accumulate %.2f roundings (bound %d)" % (name, r, r_acc, taps + 2))
    assert r <= taps + 2 and r_acc <= taps + 2
    assert x_view == (0, shape[4]) or R.outside_is(acc)
    assert torch.equal(R.inside(dya), c["dy"])


def test_elements_past_2_to_the_31():
    """Element indices are 64-bit: 8 channels at the END of a 2^26-float pitch over 2*2*3*3 = 36 rows, so the last
    rows' elements lie past index 2^31 (the buffer is allocated, never filled: only the slice is touched)."""
    import sfhip
    dev = _dev()
    shape, k, cs = (2, 2, 3, 3, 8), (2, 2, 2), 1 << 26
    coff = cs - 8
    g = _gen("big")
    x = torch.randn(*shape, generator=g)
    ref, mag = R.pool_ref(x, k, (1, 1, 1), (0, 0, 0), True)
    big = torch.empty(shape[:4] + (cs,), dtype=torch.float32, device=dev)
    assert big.numel() > 2 ** 31
    big[..., coff:] = x.to(dev)
    out = sfhip.avgpool_window(sfhip.Act(big, coff, 8), k)
    torch.cuda.synchronize()
    assert R.rounds(R.inside(out), ref, mag) <= 10
    dy = torch.randn(*ref.shape, generator=g)
    big[..., coff:] = NAN
    sfhip.avgpool_window_bwd(sfhip.Act(dy.to(dev)), sfhip.Act(big, coff, 8), k, overwrite=True)
    torch.cuda.synchronize()
    got = big[..., coff:].cpu()
    del big
    leaf = torch.zeros(shape, dtype=torch.float64).requires_grad_(True)
    torch.nn.functional.avg_pool3d(R.to_ncthw(leaf), k, 1).backward(R.to_ncthw(dy.double()))
    leaf_mag = torch.zeros(shape, dtype=torch.float64).requires_grad_(True)
    torch.nn.functional.avg_pool3d(R.to_ncthw(leaf_mag), k, 1).backward(R.to_ncthw(dy.double().abs()))
    assert R.rounds(got, leaf.grad, leaf_mag.grad) <= 10
