"""Op-level parity of the memory-bound kernels that sit under every model — sfhip.affine (flat float4, general float4
and scalar kernels, byte mask), row_softmax / row_softmax_bwd, sigmoid_bwd, the generic pool kernel and the ECA pair
on channel slices — against float64 CPU references of the same fp32 inputs (tests/_elementwise_ref.py).

Views are channel slices of wider buffers: inputs sit between NaN channels, outputs between sentinel channels that
must come back bit for bit, and a view a kernel overwrites starts as NaN.

Bounds.  Elementwise kernels: |got - ref| <= 8 * 2^-24 * mag per element, mag = sum of |terms| added to make it (they
round at most four times per element).  Average pool: (taps + 2) * 2^-24 * sum|x_window| / taps (taps - 1 additions,
the reciprocal, the product).  Max pool and the exact-arithmetic mask cases: equality.  The __expf kernels and the long
reduction keep the tolerances test_ops_gpu.py applies to them: 2e-4 max-norm relative (row softmax, gate_apply), 1e-5
(tmax_mean)."""
import zlib

import pytest
import torch

import _elementwise_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-4
ROUNDS = 8.0
NTHW = (3, 2, 5, 7)  # 210 rows


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _report(name, err):
    """One line per case in elementwise_report.txt, beside the other op-level reports."""
    from test_backward_ops_gpu import _report as report
    report(name, err, "elementwise_report.txt")


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)


NAN = float("nan")


# ------------------------------------------------------------------------------------------------ affine
def _affine_case(name, C, x_view, out_view, res_view=None, relu=False, with_scale=True, rep=1, nsplit=1,
                 params_off=0, nthw=NTHW):
    """Run sfhip.affine on slices and compare with the fp64 reference.  *_view = (coff, pitch).  params_off: scale and
    bias start that many floats into a longer tensor."""
    import sfhip
    dev = _dev()
    g = _gen(name)
    N, T, H, W = nthw
    x = torch.randn(N, T, H, W, C, generator=g)
    res = torch.randn(N, T, H, W, C, generator=g) if res_view else None
    scale = bias = scale_d = bias_d = None
    if with_scale:
        scale = (torch.rand(nsplit * C, generator=g) + 0.5) * (torch.randint(0, 2, (nsplit * C,), generator=g) * 2 - 1)
        bias = torch.randn(nsplit * C, generator=g)
        if relu == 6:  # spread the pre-activation over both clamps
            scale, bias = scale * 3, bias * 3 + 2
        pad = torch.full((params_off,), NAN)
        scale_d = torch.cat([pad, scale, pad]).to(dev)[params_off:params_off + nsplit * C]
        bias_d = torch.cat([pad, bias, pad]).to(dev)[params_off:params_off + nsplit * C]
        assert scale_d.data_ptr() % 16 == (4 * params_off) % 16 and bias_d.data_ptr() % 16 == (4 * params_off) % 16
    xa = R.view(dev, x, x_view[0], x_view[1], NAN)
    ra = R.view(dev, res, res_view[0], res_view[1], NAN) if res_view else None
    oa = R.view(dev, torch.full((N, T * rep, H, W, C), NAN), out_view[0], out_view[1], R.SENTINEL)
    ret = sfhip.affine(xa, scale_d, bias_d, res=ra, relu=relu, rep=rep, out=oa, nsplit=nsplit)
    torch.cuda.synchronize()
    assert ret is oa
    ref, mag = R.affine_ref(x, scale, bias, res, relu, rep, nsplit)
    got = R.inside(oa)
    r = R.rounds(got, ref, mag)
    _report("affine/" + name, r)
    assert r <= ROUNDS, (name, r)
    assert R.outside_is(oa), name
    assert torch.equal(R.inside(xa), x), "the input view changed"


# C, res view or None, activation, with scale — x at coff 4 of pitch C + 8, out at coff 8 of pitch C + 12
FLAT_CASES = [
    (4, False, False, True), (4, True, True, True), (4, False, 6, True),
    (12, False, True, True), (12, True, 6, True), (12, True, False, True), (12, True, True, False),
    (64, False, 6, True), (64, True, True, True), (64, True, False, False),
]


@pytest.mark.parametrize("C,res,relu,with_scale", FLAT_CASES,
                         ids=["C%d_%s_act%s_%s" % (c, "res" if r else "nores", int(a), "scale" if s else "addinto")
                              for c, r, a, s in FLAT_CASES])
def test_affine_flat_float4(C, res, relu, with_scale):
    """S = 1, rep = 1, every view 16-byte addressable: C / 4 = 1, 3 (division) and 16 (shift); 210, 630 and 3360
    float4 — one partial 1024-element block, and three full blocks with a ragged tail."""
    assert 210 * (C // 4) in (210, 630, 3360)
    _affine_case("flat/C%d_res%d_act%d_scale%d" % (C, res, int(relu), with_scale), C, (4, C + 8), (8, C + 12),
                 (4, C + 4) if res else None, relu, with_scale)


GENERAL_CASES = {
    "rep2": dict(rep=2, res_view=(4, 16), relu=True),
    "nsplit2_N3": dict(nsplit=2),
    "rep2_nsplit3": dict(rep=2, nsplit=3, res_view=(4, 16), relu=True),
    "params_4_mod_16": dict(params_off=1, relu=6),
}


@pytest.mark.parametrize("name", list(GENERAL_CASES))
def test_affine_general_float4(name):
    """C = 12 on float4-addressable slices, each of the four ways that keep the flat kernel out: a T repeat, scale /
    bias blocks by n % nsplit (N = 3, nsplit = 2: samples 0 and 2 take block 0, sample 1 block 1), both, and scale /
    bias pointers at 4 mod 16."""
    assert NTHW[0] == 3
    _affine_case("general/" + name, 12, (4, 20), (8, 24), **GENERAL_CASES[name])


SCALAR_CASES = {
    "C7": dict(C=7, x_view=(4, 15), out_view=(8, 19), res_view=(4, 11), relu=True),
    "C12_xcoff3": dict(C=12, x_view=(3, 20), out_view=(8, 24), relu=6),
    "C5_rep3": dict(C=5, x_view=(0, 5), out_view=(1, 9), rep=3, res_view=(2, 8), relu=True, nsplit=3),
}


@pytest.mark.parametrize("name", list(SCALAR_CASES))
def test_affine_scalar(name):
    _affine_case("scalar/" + name, **SCALAR_CASES[name])


def test_affine_scalar_out_cmul():
    """C = 10 scattered with a channel multiplier of 2 into channels 1, 3, .., 19 of a 24-wide zero buffer."""
    import sfhip
    dev = _dev()
    g = _gen("cmul")
    N, T, H, W = NTHW
    C = 10
    x, res = torch.randn(N, T, H, W, C, generator=g), torch.randn(N, T, H, W, C, generator=g)
    scale, bias = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    full = torch.zeros(N, T, H, W, 24, device=dev)
    sfhip.affine(R.view(dev, x, 2, 13, NAN), scale.to(dev), bias.to(dev), res=R.view(dev, res, 1, 12, NAN), relu=True,
                 out=sfhip.Act(full, 1, 19), out_cmul=2)
    torch.cuda.synchronize()
    ref, mag = R.affine_ref(x, scale, bias, res, True)
    full = full.cpu()
    r = R.rounds(full[..., 1:20:2], ref, mag)
    _report("affine/scalar/C10_cmul2", r)
    assert r <= ROUNDS
    assert bool((full[..., 0::2].contiguous().view(torch.int32) == 0).all())
    assert bool((full[..., 20:].contiguous().view(torch.int32) == 0).all())


def _exact_inputs(g, shape_x, C):
    """Quarter-integers in [-4, 4] and scales in {0.5, 1, -1, 2}: x * scale + bias + res is exact in fp32 with or
    without fma contraction."""
    q = lambda *s: torch.randint(-16, 17, s, generator=g).float() * 0.25
    scale = torch.tensor([0.5, 1.0, -1.0, 2.0])[torch.randint(0, 4, (C,), generator=g)]
    return q(*shape_x), scale, q(C), q(*shape_x)


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [True, 6], ids=["relu", "relu6"])
@pytest.mark.parametrize("C", [12, 64])
def test_affine_byte_mask(C, relu, with_res):
    import sfhip
    dev = _dev()
    N, T, H, W = NTHW
    x, scale, bias, res = _exact_inputs(_gen("mask%d" % C), (N, T, H, W, C), C)
    if not with_res:
        res = None
    pre, _ = R.affine_ref(x, scale, bias, res, False)
    ref = R.act_ref(pre, relu)
    assert bool((pre == 0).any()), "the boundary y == 0 is not hit"
    if relu == 6:
        assert bool((pre == 6).any()), "the boundary y == 6 is not hit"
    xa = R.view(dev, x, 4, C + 8, NAN)
    ra = R.view(dev, res, 4, C + 4, NAN) if with_res else None
    oa = R.view(dev, torch.full((N, T, H, W, C), NAN), 8, C + 12, R.SENTINEL)
    mask = {}
    sfhip.affine(xa, scale.to(dev), bias.to(dev), res=ra, relu=relu, out=oa, mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(R.inside(oa).double(), ref)
    assert R.outside_is(oa)
    assert "bytes" in mask and mask["bytes"].dtype == torch.uint8
    want = R.mask_ref(pre, relu)
    assert mask["bytes"].shape == want.shape
    assert torch.equal(mask["bytes"].cpu(), want)


def test_affine_byte_mask_declined_for_scalar_view():
    """C = 7 cannot take the flat float4 kernel: the dict comes back without 'bytes' and the output is still right."""
    import sfhip
    dev = _dev()
    N, T, H, W = NTHW
    C = 7
    x, scale, bias, res = _exact_inputs(_gen("mask7"), (N, T, H, W, C), C)
    ref = R.act_ref(R.affine_ref(x, scale, bias, res, False)[0], True)
    oa = R.view(dev, torch.full((N, T, H, W, C), NAN), 8, C + 12, R.SENTINEL)
    mask = {}
    sfhip.affine(R.view(dev, x, 4, C + 8, NAN), scale.to(dev), bias.to(dev), res=R.view(dev, res, 4, C + 4, NAN),
                 relu=True, out=oa, mask=mask)
    torch.cuda.synchronize()
    assert mask == {}
    assert torch.equal(R.inside(oa).double(), ref)
    assert R.outside_is(oa)


# ------------------------------------------------------------------------------------------------ row softmax
SOFTMAX_C = [1, 18, 63, 64, 65, 200]
SOFTMAX_SHAPE = (2, 1, 3, 3)  # 18 rows: four full workgroups of 4 wavefronts and one with two idle ones
SOFTMAX_CASES = ([(c, s, False) for c in SOFTMAX_C for s in (1.0, 0.125)] +
                 [(c, s, True) for c in SOFTMAX_C if c >= 18 for s in (1.0, 0.125)])


@pytest.mark.parametrize("C,scale,plant", SOFTMAX_CASES,
                         ids=["C%d_s%g%s" % (c, s, "_plant88" if p else "") for c, s, p in SOFTMAX_CASES])
def test_row_softmax_fwd(C, scale, plant):
    """plant: one entry per row sits 88 / scale above the row's largest — exp overflows unless the maximum is
    subtracted first."""
    import sfhip
    dev = _dev()
    g = _gen("smax%d" % C)
    x = torch.randn(*SOFTMAX_SHAPE, C, generator=g) * 20 / scale
    if plant:
        rows = x.view(-1, C)
        top = rows.max(1).values
        for r in range(rows.shape[0]):
            rows[r, (r * 37 + C - 1) % C] = top[r] + 88 / scale
    a = R.view(dev, x, 3, C + 5, R.SENTINEL)
    assert a.rows == 18
    ret = sfhip.row_softmax(a, scale)
    torch.cuda.synchronize()
    assert ret is a
    got = R.inside(a)
    ref = torch.softmax(scale * x.double(), -1)
    assert bool(torch.isfinite(got).all())
    err = R.rel(got, ref)
    _report("row_softmax/fwd_C%d_s%g%s" % (C, scale, "_plant88" if plant else ""), err)
    assert err < TOL
    assert R.outside_is(a)


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("C", SOFTMAX_C)
def test_row_softmax_bwd(C, scale):
    import sfhip
    dev = _dev()
    g = _gen("smaxb%d" % C)
    p = torch.softmax(torch.randn(*SOFTMAX_SHAPE, C, generator=g, dtype=torch.float64) * 2, -1).float()
    dp = torch.randn(*SOFTMAX_SHAPE, C, generator=g)
    pa = R.view(dev, p, 3, C + 5, NAN)
    da = R.view(dev, dp, 4, C + 8, R.SENTINEL)
    assert pa.rows == 18
    ret = sfhip.row_softmax_bwd(pa, da, scale)
    torch.cuda.synchronize()
    assert ret is da
    got = R.inside(da)
    assert bool(torch.isfinite(got).all())
    ref = R.softmax_bwd_ref(p, dp, scale)
    if C == 1:  # p == 1: dp - <p, dp> is exactly zero
        assert bool((got == 0).all())
    err = R.rel(got, ref) if C > 1 else float(got.abs().max())
    _report("row_softmax/bwd_C%d_s%g" % (C, scale), err)
    assert err < TOL
    assert R.outside_is(da)
    assert torch.equal(R.inside(pa), p), "p changed"


# ------------------------------------------------------------------------------------------------ sigmoid backward
@pytest.mark.parametrize("accumulate", [True, False], ids=["accumulate", "overwrite"])
@pytest.mark.parametrize("shape", [(1,), (255,), (256,), (257,), (5, 80)], ids=["n1", "n255", "n256", "n257", "n400"])
def test_sigmoid_bwd(shape, accumulate):
    import sfhip
    dev = _dev()
    n = 1
    for s in shape:
        n *= s
    g = _gen("sig%d" % n)
    y = torch.sigmoid(torch.randn(n, generator=g, dtype=torch.float64) * 4).float()
    zeros, ones = ([0, n // 2], [n - 1, 254]) if n >= 255 else ([], [])
    for i in zeros:
        y[i] = 0.0
    for i in ones:
        y[i] = 1.0
    dy = torch.randn(n, generator=g)
    base = torch.randn(n, generator=g) if accumulate else None
    pad = 3  # dx is a window of a longer sentinel tensor (and sits at 12 mod 16 bytes)
    full = torch.full((n + 2 * pad,), R.SENTINEL)
    full[pad:pad + n] = base if accumulate else NAN
    full = full.to(dev)
    dx = full[pad:pad + n].view(shape)
    ret = sfhip.sigmoid_bwd(y.view(shape).to(dev), dy.view(shape).to(dev), dx, accumulate=accumulate)
    torch.cuda.synchronize()
    assert ret is dx
    full = full.cpu()
    got = full[pad:pad + n]
    ref, mag = R.sigmoid_bwd_ref(y, dy, base)
    r = R.rounds(got, ref, mag)
    _report("sigmoid_bwd/n%d_%s" % (n, "acc" if accumulate else "ovw"), r)
    assert r <= ROUNDS
    for i in zeros + ones:  # a saturated output passes no gradient at all
        assert float(got[i]) == (float(base[i]) if accumulate else 0.0), i
    edge = torch.cat([full[:pad], full[pad + n:]])
    assert torch.equal(edge.view(torch.int32), torch.full_like(edge, R.SENTINEL).view(torch.int32))


# ------------------------------------------------------------------------------------------------ pool, generic kernel
POOL_NTHW = (2, 4, 13, 12)
POOL_K, POOL_S, POOL_P = (3, 3, 3), (1, 2, 2), (1, 1, 1)
POOL_VIEWS = {  # C, x view, out view
    "float4_C8_coff4_pitch20": (8, (4, 20), (4, 16)),
    "scalar_C6_dense": (6, (0, 6), (1, 9)),
    "scalar_C8_coff2": (8, (2, 12), (4, 16)),
}
_pool_inputs = {}


def _pool_input(name):
    if name not in _pool_inputs:
        _pool_inputs[name] = torch.randn(*POOL_NTHW, POOL_VIEWS[name][0], generator=_gen("pool" + name))
    return _pool_inputs[name]


def _pool_out(dev, ref, out_view):
    return R.view(dev, torch.full(ref.shape, NAN), out_view[0], out_view[1], R.SENTINEL)


@pytest.mark.parametrize("avg", [False, True], ids=["max", "avg"])
@pytest.mark.parametrize("name", list(POOL_VIEWS))
def test_pool_generic_views(name, avg):
    """Padded (3,3,3)/(1,2,2)/(1,1,1) windows: max exactly, average over the full window (count_include_pad=True)."""
    import sfhip
    dev = _dev()
    C, x_view, out_view = POOL_VIEWS[name]
    x = _pool_input(name)
    ref, mag = R.pool_ref(x, POOL_K, POOL_S, POOL_P, avg)
    assert tuple(ref.shape) == (2, 4, 7, 6, C)
    xa = R.view(dev, x, x_view[0], x_view[1], NAN)
    oa = _pool_out(dev, ref, out_view)
    ret = sfhip.pool(xa, POOL_K, POOL_S, POOL_P, avg=avg, out=oa)
    torch.cuda.synchronize()
    assert ret is oa
    got = R.inside(oa)
    if avg:
        taps = POOL_K[0] * POOL_K[1] * POOL_K[2]
        r = R.rounds(got, ref, mag)  # mag = sum |x_window| / taps
        _report("pool/avg_" + name, r)
        assert r <= taps + 2
    else:
        assert torch.equal(got.double(), ref)
    assert R.outside_is(oa)
    assert torch.equal(R.inside(xa), x)


@pytest.mark.parametrize("avg", [False, True], ids=["max", "avg"])
def test_pool_float4_out_reserve(avg):
    """The float4 slice again, the output allocated by pool() itself with out_reserve=(4, 4)."""
    import sfhip
    dev = _dev()
    name = "float4_C8_coff4_pitch20"
    x = _pool_input(name)
    ref, mag = R.pool_ref(x, POOL_K, POOL_S, POOL_P, avg)
    out = sfhip.pool(R.view(dev, x, 4, 20, NAN), POOL_K, POOL_S, POOL_P, avg=avg, out_reserve=(4, 4))
    torch.cuda.synchronize()
    assert (out.coff, out.C, out.cs) == (4, 8, 16) and tuple(out.buf.shape[:4]) == tuple(ref.shape[:4])
    got = R.inside(out)
    if avg:
        r = R.rounds(got, ref, mag)
        _report("pool/avg_reserve_" + name, r)
        assert r <= POOL_K[0] * POOL_K[1] * POOL_K[2] + 2
    else:
        assert torch.equal(got.double(), ref)


def test_pool_want_arg_declined_for_scalar_view():
    import sfhip
    dev = _dev()
    name = "scalar_C6_dense"
    x = _pool_input(name)
    ref, _ = R.pool_ref(x, POOL_K, POOL_S, POOL_P, False)
    oa = _pool_out(dev, ref, (1, 9))
    ret = sfhip.pool(R.view(dev, x, 0, 6, NAN), POOL_K, POOL_S, POOL_P, out=oa, want_arg=True)
    torch.cuda.synchronize()
    assert isinstance(ret, tuple) and len(ret) == 2 and ret[0] is oa and ret[1] is None
    assert torch.equal(R.inside(oa).double(), ref)
    assert R.outside_is(oa)


# ------------------------------------------------------------------------------------------------ ECA on slices
@pytest.mark.parametrize("alpha", [4, 8])
@pytest.mark.parametrize("C,x_view,out_view", [(32, (4, 40), (4, 40)), (3, (3, 8), (2, 7))],
                         ids=["C32_coff4_pitch40", "C3_coff3_pitch8"])
def test_eca_on_slices(C, x_view, out_view, alpha):
    import sfhip
    dev = _dev()
    g = _gen("eca%d" % C)
    N, T, H, W = 2, 8, 7, 9
    x = torch.randn(N, T, H, W, C, generator=g)
    w3 = torch.randn(3, generator=g)
    scale, bias = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    pooled_ref, ref = R.eca_ref(x, alpha, w3, scale, bias)
    xa = R.view(dev, x, x_view[0], x_view[1], NAN)
    oa = R.view(dev, torch.full(ref.shape, NAN), out_view[0], out_view[1], R.SENTINEL)
    pooled = sfhip.tmax_mean(xa, alpha)
    ret = sfhip.gate_apply(xa, alpha, pooled, w3=w3.to(dev), scale=scale.to(dev), bias=bias.to(dev), relu=True, out=oa)
    torch.cuda.synchronize()
    assert ret is oa and tuple(pooled.shape) == (N, C)
    e1, e2 = R.rel(pooled.cpu(), pooled_ref), R.rel(R.inside(oa), ref)
    _report("eca_slices/C%d_a%d pooled" % (C, alpha), e1)
    _report("eca_slices/C%d_a%d out" % (C, alpha), e2)
    assert e1 < 1e-5 and e2 < TOL
    assert bool(torch.isfinite(R.inside(oa)).all())
    assert R.outside_is(oa)
    assert torch.equal(R.inside(xa), x)
