"""sf_epilogue_bwd_act and sf_dwconv_dgrad_epi (csrc/gradcam.hip) through the binding, against float64 restatements
written here: activation codes none / ReLU / ReLU6 with y drawn from a grid that holds exact zeros and sixes, the
un-shuffling gather (groups 2 and 3), the residual gradient stored and accumulated, a T-repeat, depthwise strides
(1,1,1) and (1,2,2) over odd H and W, overwrite into NaN and accumulate, on channel slices with a pitch above C and a
non-zero offset (float4 form: C 8 and 12 at offset 4; scalar form: C 3, 6, 70 and an unaligned slice of 8).

Tolerance 1e-5, max-norm relative: each output is a sum of at most 27 fp32 products of exactly masked terms, one
multiplication by scale and one accumulate — about 30 roundings of 6e-8 on terms of the output's own magnitude.  Where
sf_epilogue_bwd_act coincides with sf_epilogue_bwd (groups 1, no activation or ReLU) the two must agree bit for bit, and
two runs of either entry must too."""
import zlib

import pytest
import torch
import torch.nn.functional as F

import _elementwise_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
NAN = float("nan")
N, T, H, W = 2, 2, 5, 5
CHANNELS = (3, 6, 8, 12, 70)
ACTS = (False, True, 6)
# exact zeros and sixes and values on both sides of each: no rounding decides the mask
Y_GRID = torch.tensor([-1.5, -0.25, 0.0, 0.0, 0.25, 3.0, 5.75, 6.0, 6.0, 6.25, 8.0])


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)


def _report(name, err):
    from test_backward_ops_gpu import _report as report
    report(name, err, "gradcam_report.txt")


def _grid(shape, g):
    y = Y_GRID[torch.randint(0, Y_GRID.numel(), shape, generator=g)]
    assert int((y == 0).sum()) > 0 and int((y == 6).sum()) > 0
    return y


def _mask(y, act):
    if act == 6:
        return ((y > 0) & (y < 6)).double()
    return (y > 0).double() if act else torch.ones_like(y, dtype=torch.float64)


def _geom(C, aligned=True):
    """(offset, pitch) of a slice with room on both sides; aligned: offset and pitch multiples of 4."""
    return (4, (C + 3) // 4 * 4 + 8) if aligned else (3, C + 5)


# ------------------------------------------------------------------------------------------------ sf_epilogue_bwd_act
def _epi_ref(dy, y, scale, act, rep, groups, base, rbase):
    """float64 (dz, dres): dz channel g * C/G + j takes dy * m(y) at channel j * G + g."""
    C = dy.shape[-1]
    terms = (dy.double() * _mask(y, act)).view(N, T, rep, H, W, C)
    cz = torch.arange(C)
    src = (cz % (C // groups)) * groups + cz // (C // groups)
    dz = terms.sum(2)[..., src]
    if scale is not None:
        dz = dz * scale.double()
    dres = terms[:, :, 0]
    if base is not None:
        dz = dz + base.double()
    if rbase is not None:
        dres = dres + rbase.double()
    return dz, dres


def _epi_run(dev, C, act, groups, rep, with_dres, acc, aligned=True, via_act=True, with_scale=True):
    import sfhip
    g = _gen("epi_eff_%d_%d" % (C, rep))
    dy = torch.randn(N, T * rep, H, W, C, generator=g)
    y = _grid((N, T * rep, H, W, C), g)
    scale = torch.randn(C, generator=g) * 1.5
    dz0 = torch.randn(N, T, H, W, C, generator=g)
    dr0 = torch.randn(N, T, H, W, C, generator=g)
    off, pitch = _geom(C, aligned)
    dya = R.view(dev, dy, off, pitch, R.SENTINEL)
    ya = R.view(dev, y, off, pitch, R.SENTINEL)
    dza = R.view(dev, dz0 if acc else torch.full_like(dz0, NAN), off, pitch, R.SENTINEL)
    dra = R.view(dev, dr0 if acc else torch.full_like(dr0, NAN), off, pitch, R.SENTINEL) if with_dres else None
    sc = scale.to(dev) if with_scale else None
    if via_act:
        sfhip.epilogue_bwd(dya, ya, dza, scale=sc, act=act, groups=groups, rep=rep, dz_accumulate=acc, dres=dra,
                           dres_accumulate=acc)
    else:
        sfhip.epilogue_bwd(dya, ya, dza, scale=sc, relu=act, rep=rep, dz_accumulate=acc, dres=dra, dres_accumulate=acc)
    torch.cuda.synchronize()
    assert R.outside_is(dza) and R.outside_is(dya) and R.outside_is(ya)
    assert torch.equal(R.inside(dya), dy) and torch.equal(R.inside(ya), y), "an input changed"
    assert dra is None or R.outside_is(dra)
    ref = _epi_ref(dy, y, scale if with_scale else None, act, rep, groups, dz0 if acc else None,
                   dr0 if (acc and with_dres) else None)
    return R.inside(dza), (R.inside(dra) if with_dres else None), ref


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_epilogue_bwd_act(C, act):
    dev = _dev()
    variants = [(G, 1, False, acc) for G in (1, 2, 3) if C % G == 0 for acc in (False, True)]
    variants += [(1, 1, True, False), (1, 1, True, True), (1, 2, False, False), (1, 2, False, True)]
    for groups, rep, with_dres, acc in variants:
        name = "epilogue_bwd_act/C%d_act%d_g%d_rep%d_r%d_a%d" % (C, int(act), groups, rep, with_dres, acc)
        dz, dres, (rz, rr) = _epi_run(dev, C, act, groups, rep, with_dres, acc)
        e = R.rel(dz, rz)
        _report(name + "/dz", e)
        assert bool(torch.isfinite(dz).all()) and e <= TOL, (name, e)
        if with_dres:
            er = R.rel(dres, rr)
            _report(name + "/dres", er)
            assert bool(torch.isfinite(dres).all()) and er <= TOL, (name, er)
        again, dres2, _ = _epi_run(dev, C, act, groups, rep, with_dres, acc)
        assert torch.equal(dz, again) and (dres is None or torch.equal(dres, dres2)), name


@pytest.mark.parametrize("act", ACTS)
def test_epilogue_bwd_act_scalar_form_on_an_unaligned_slice(act):
    """C = 8 at offset 3 of a pitch-13 buffer: the scalar kernels, with and without a scale."""
    dev = _dev()
    for groups, with_scale in ((1, True), (2, True), (2, False)):
        dz, _, (rz, _) = _epi_run(dev, 8, act, groups, 1, False, False, aligned=False, with_scale=with_scale)
        e = R.rel(dz, rz)
        _report("epilogue_bwd_act/unaligned_act%d_g%d_s%d" % (int(act), groups, with_scale), e)
        assert e <= TOL, (act, groups, e)


@pytest.mark.parametrize("act", (False, True))
@pytest.mark.parametrize("C", (8, 70))
def test_epilogue_bwd_act_is_bitwise_sf_epilogue_bwd_where_they_coincide(C, act):
    dev = _dev()
    for rep, with_dres, acc in ((1, False, False), (1, True, False), (1, True, True), (2, False, True)):
        new = _epi_run(dev, C, act, 1, rep, with_dres, acc, via_act=True)
        old = _epi_run(dev, C, act, 1, rep, with_dres, acc, via_act=False)
        assert torch.equal(new[0], old[0]), (C, act, rep, with_dres, acc)
        assert new[1] is None or torch.equal(new[1], old[1])


def test_mask_edges_pass_nothing():
    """dy = 1 everywhere: the result IS the mask — y == 0 and y == 6 pass no gradient, under the shuffle too."""
    import sfhip
    dev = _dev()
    C, G = 12, 3
    y = _grid((N, T, H, W, C), _gen("edges"))
    cz = torch.arange(C)
    src = (cz % (C // G)) * G + cz // (C // G)
    for act in (True, 6):
        for groups in (1, G):
            dza = R.view(dev, torch.full((N, T, H, W, C), NAN), 4, 24, R.SENTINEL)
            sfhip.epilogue_bwd(R.view(dev, torch.ones_like(y), 4, 24, R.SENTINEL), R.view(dev, y, 4, 24, R.SENTINEL),
                               dza, act=act, groups=groups)
            torch.cuda.synchronize()
            want = _mask(y, act).float()
            assert torch.equal(R.inside(dza), want[..., src] if groups > 1 else want), (act, groups)


# ------------------------------------------------------------------------------------------------ sf_dwconv_dgrad_epi
def _dw_ref(dy, y, w, scale, act, stride, base):
    """float64 dx [N, T, H, W, C]: autograd of F.conv3d(groups = C) with dL/dz = scale * dy * m(y)."""
    C = dy.shape[-1]
    dz = dy.double() * _mask(y, act)
    if scale is not None:
        dz = dz * scale.double()
    x = torch.zeros(N, C, T, H, W, dtype=torch.float64, requires_grad=True)
    z = F.conv3d(x, w.double(), None, stride, 1, 1, C)
    assert tuple(z.shape) == (N, C) + tuple(dy.shape[1:4])
    z.backward(dz.permute(0, 4, 1, 2, 3))
    dx = x.grad.permute(0, 2, 3, 4, 1)
    return dx + base.double() if base is not None else dx


def _dw_run(dev, C, act, stride, acc, aligned=True, with_scale=True):
    import sfhip
    g = _gen("dw_eff_%d_%d" % (C, stride[1]))
    To, Ho, Wo = T, (H - 1) // stride[1] + 1, (W - 1) // stride[2] + 1
    dy = torch.randn(N, To, Ho, Wo, C, generator=g)
    y = _grid((N, To, Ho, Wo, C), g)
    w = torch.randn(C, 1, 3, 3, 3, generator=g)
    scale = torch.randn(C, generator=g) * 1.5
    dx0 = torch.randn(N, T, H, W, C, generator=g)
    off, pitch = _geom(C, aligned)
    wpitch = (C + 15) // 16 * 16  # [taps][pad16(C)], as the engine's packed depthwise weights
    wp = torch.zeros(27, wpitch)
    wp[:, :C] = sfhip.pack_dw_weight(w)
    dya = R.view(dev, dy, off, pitch, R.SENTINEL)
    ya = R.view(dev, y, off, pitch, R.SENTINEL)
    dxa = R.view(dev, dx0 if acc else torch.full_like(dx0, NAN), off, pitch, R.SENTINEL)
    x_like = sfhip.Act(torch.empty(N, T, H, W, C, device=dev))
    ret = sfhip.dwconv_dgrad_epi(x_like, dya, ya if act else None, wp.to(dev), (3, 3, 3), stride, (1, 1, 1), dxa,
                                 scale=scale.to(dev) if with_scale else None, relu=act, accumulate=acc)
    torch.cuda.synchronize()
    assert ret is dxa and R.outside_is(dxa) and R.outside_is(dya) and R.outside_is(ya)
    assert torch.equal(R.inside(dya), dy) and torch.equal(R.inside(ya), y), "an input changed"
    return R.inside(dxa), _dw_ref(dy, y, w, scale if with_scale else None, act, stride, dx0 if acc else None)


@pytest.mark.parametrize("stride", [(1, 1, 1), (1, 2, 2)])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_dwconv_dgrad_epi(C, act, stride):
    dev = _dev()
    for acc in (False, True):
        name = "dwconv_dgrad_epi/C%d_act%d_s%d_a%d" % (C, int(act), stride[1], acc)
        dx, ref = _dw_run(dev, C, act, stride, acc)
        e = R.rel(dx, ref)
        _report(name, e)
        assert bool(torch.isfinite(dx).all()), name  # overwrite: every element of the NaN-filled slice was written
        assert e <= TOL, (name, e)
        again, _ = _dw_run(dev, C, act, stride, acc)
        assert torch.equal(dx, again), name


@pytest.mark.parametrize("stride", [(1, 1, 1), (1, 2, 2)])
def test_dwconv_dgrad_epi_scalar_form_and_no_scale(stride):
    """C = 8 at offset 3 of a pitch-13 buffer (scalar kernel), and scale = NULL (means 1) on both forms."""
    dev = _dev()
    for act, aligned, with_scale in ((6, False, True), (False, False, False), (True, True, False)):
        dx, ref = _dw_run(dev, 8, act, stride, False, aligned=aligned, with_scale=with_scale)
        e = R.rel(dx, ref)
        _report("dwconv_dgrad_epi/C8_act%d_s%d_al%d_sc%d" % (int(act), stride[1], aligned, with_scale), e)
        assert bool(torch.isfinite(dx).all()) and e <= TOL, (act, aligned, with_scale, e)


@pytest.mark.parametrize("stride", [(1, 1, 1), (1, 2, 2)])
def test_dwconv_dgrad_epi_equals_the_two_launch_form(stride):
    """sf_epilogue_bwd_act into a dL/dz tensor, then sf_dwconv_dgrad: the form the fused entry replaces."""
    import sfhip
    dev = _dev()
    C = 8
    g = _gen("dw_two_%d" % stride[1])
    To, Ho, Wo = T, (H - 1) // stride[1] + 1, (W - 1) // stride[2] + 1
    dy = sfhip.Act(torch.randn(N, To, Ho, Wo, C, generator=g).to(dev))
    y = sfhip.Act(_grid((N, To, Ho, Wo, C), g).to(dev))
    wp = torch.zeros(27, 16)
    wp[:, :C] = torch.randn(27, C, generator=g)
    wp = wp.to(dev)
    scale = (torch.randn(C, generator=g) * 1.5).to(dev)
    x_like = sfhip.Act(torch.empty(N, T, H, W, C, device=dev))
    fused = sfhip.Act(torch.full((N, T, H, W, C), NAN, device=dev))
    sfhip.dwconv_dgrad_epi(x_like, dy, y, wp, (3, 3, 3), stride, (1, 1, 1), fused, scale=scale, relu=6, accumulate=False)
    dz = sfhip.Act(torch.empty(N, To, Ho, Wo, C, device=dev))
    sfhip.epilogue_bwd(dy, y, dz, scale=scale, act=6)
    two = sfhip.Act(torch.zeros(N, T, H, W, C, device=dev))
    sfhip.dwconv_dgrad(x_like, dz, wp, (3, 3, 3), stride, (1, 1, 1), two)
    torch.cuda.synchronize()
    e = R.rel(fused.buf.cpu(), two.buf.cpu().double())
    _report("dwconv_dgrad_epi/vs_two_launches_s%d" % stride[1], e)
    assert e <= TOL, e
