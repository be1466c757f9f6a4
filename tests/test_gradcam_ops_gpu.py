"""The Grad-CAM kernels (csrc/gradcam.hip) through the binding, against float64 restatements written here:
sf_epilogue_bwd on channel slices (float4 and scalar paths, T-repeat, ReLU mask boundary, overwrite / accumulate,
neighbours untouched), sf_head_act_mean_bwd against torch autograd in float64, sf_cam_weights / sf_cam_map against the
arithmetic of the reference's gradcam_video.py:159-179.

Bounds.  One fp32 rounding moves a value by at most U = 2^-24 of its magnitude.  sf_epilogue_bwd: the masked products
are exact, the repeat sum has rep - 1 additions, then one multiplication by scale and, when accumulating, one addition:
|err| <= (rep + 1) * U * sum|terms|.  The CAM sums: (#additions + 1) * U * sum|terms| (one division or fused
multiply-add rounding per term beside the additions).  sf_head_act_mean_bwd keeps the 2e-4 max-norm relative tolerance
tests/test_elementwise_views_gpu.py applies to the row-softmax backward (its TOL)."""
import itertools
import zlib

import pytest
import torch

import _elementwise_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-4  # tests/test_elementwise_views_gpu.py::TOL (row softmax forward / backward)
U = R.U


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)


def _report(name, err):
    from test_backward_ops_gpu import _report as report
    report(name, err, "gradcam_report.txt")


# ------------------------------------------------------------------------------------------------ sf_epilogue_bwd
NTHW = (1, 2, 3, 5)  # dz's [N, T, H, W]
EPI_CASES = [(C, rep, relu, scale, dres, acc)
             for C in (8, 5) for rep in (1, 4) for relu in (False, True) for scale in (False, True)
             for dres in (False, True) for acc in (False, True) if not (dres and rep != 1)]


def _epi_inputs(name, C, rep):
    """dy, y [N, T*rep, H, W, C] with y exactly 0 on a planted tenth of the elements (and negative on about half of
    the rest), scale [C], and the previous contents of dz / dres for the accumulate runs."""
    g = _gen(name)
    N, T, H, W = NTHW
    shp = (N, T * rep, H, W, C)
    dy = torch.randn(*shp, generator=g)
    y = torch.randn(*shp, generator=g)
    y[torch.rand(*shp, generator=g) < 0.1] = 0.0
    assert 0 < int((y == 0).sum()) < y.numel() // 4
    scale = torch.randn(C, generator=g) * 1.5
    dz0 = torch.randn(N, T, H, W, C, generator=g)
    dres0 = torch.randn(N, T, H, W, C, generator=g)
    return dy, y, scale, dz0, dres0


def _epi_ref(dy, y, scale, relu, rep, dz0, dres0, acc):
    """float64: (dz, its magnitude, dres, its magnitude)."""
    N, T, H, W = NTHW
    C = dy.shape[-1]
    m = (y > 0).double() if relu else torch.ones_like(y, dtype=torch.float64)
    terms = (dy.double() * m).view(N, T, rep, H, W, C)
    s = scale.double() if scale is not None else torch.ones(C, dtype=torch.float64)
    dz, mag = terms.sum(2) * s, terms.abs().sum(2) * s.abs()
    dres, rmag = terms[:, :, 0], terms[:, :, 0].abs()
    if acc:
        dz, mag = dz + dz0.double(), mag + dz0.double().abs()
        dres, rmag = dres + dres0.double(), rmag + dres0.double().abs()
    return dz, mag, dres, rmag


@pytest.mark.parametrize("C,rep,relu,with_scale,with_dres,acc", EPI_CASES)
def test_epilogue_bwd(C, rep, relu, with_scale, with_dres, acc):
    import sfhip
    dev = _dev()
    name = "epi_C%d_rep%d_relu%d_s%d_r%d_a%d" % (C, rep, relu, with_scale, with_dres, acc)
    dy, y, scale, dz0, dres0 = _epi_inputs("epi%d_%d" % (C, rep), C, rep)
    dya = R.view(dev, dy, 4, 16, R.SENTINEL)
    ya = R.view(dev, y, 4, 16, R.SENTINEL)
    # overwrite: the slice starts as NaN and every element must be written
    dza = R.view(dev, dz0 if acc else torch.full_like(dz0, float("nan")), 4, 16, R.SENTINEL)
    dra = R.view(dev, dres0 if acc else torch.full_like(dres0, float("nan")), 4, 16, R.SENTINEL) if with_dres else None
    sc = scale.to(dev) if with_scale else None
    ret = sfhip.epilogue_bwd(dya, ya, dza, scale=sc, relu=relu, rep=rep, dz_accumulate=acc, dres=dra,
                             dres_accumulate=acc)
    torch.cuda.synchronize()
    assert ret is dza
    dz, mag, dres, rmag = _epi_ref(dy, y, scale if with_scale else None, relu, rep, dz0, dres0, acc)
    r = R.rounds(R.inside(dza), dz, mag)
    _report("epilogue_bwd/%s/dz_rounds" % name, r)
    assert r <= rep + 1, (name, r)
    assert R.outside_is(dza)
    if with_dres:
        rr = R.rounds(R.inside(dra), dres, rmag)
        _report("epilogue_bwd/%s/dres_rounds" % name, rr)
        assert rr <= rep + 1, (name, rr)
        assert R.outside_is(dra)
    assert torch.equal(R.inside(dya), dy) and torch.equal(R.inside(ya), y), "an input changed"
    assert R.outside_is(dya) and R.outside_is(ya)


def test_epilogue_bwd_mask_is_strictly_positive():
    """y == 0 passes no gradient (> 0, not >= 0), with dy = 1 everywhere so that every planted zero shows."""
    import sfhip
    dev = _dev()
    _, y, _, dz0, _ = _epi_inputs("epi8_1", 8, 1)
    dya = R.view(dev, torch.ones_like(y), 4, 16, R.SENTINEL)
    ya = R.view(dev, y, 4, 16, R.SENTINEL)
    dza = R.view(dev, torch.full_like(dz0, float("nan")), 4, 16, R.SENTINEL)
    sfhip.epilogue_bwd(dya, ya, dza, relu=True)
    torch.cuda.synchronize()
    assert torch.equal(R.inside(dza), (y > 0).float())


# ------------------------------------------------------------------------------------------------ sf_head_act_mean_bwd
@pytest.mark.parametrize("act", ["softmax", "sigmoid"])
@pytest.mark.parametrize("P,K", list(itertools.product((1, 18), (3, 400))))
def test_head_act_mean_bwd(act, P, K):
    import sfhip
    dev = _dev()
    B = 2
    g = _gen("head%d_%d" % (P, K))
    logits = torch.randn(B, P, K, generator=g) * 3
    dout = torch.randn(B, K, generator=g)
    lead = logits.double().requires_grad_(True)
    probs = torch.softmax(lead, -1) if act == "softmax" else torch.sigmoid(lead)
    (probs.mean(1) * dout.double()).sum().backward()
    code = sfhip.ACT_SOFTMAX if act == "softmax" else sfhip.ACT_SIGMOID
    la = sfhip.Act(logits.view(B, P, 1, 1, K).to(dev))
    base = torch.randn(B, P, K, generator=g)
    for acc in (False, True):
        dl = sfhip.Act((base if acc else torch.full_like(base, float("nan"))).view(B, P, 1, 1, K).to(dev))
        sfhip.head_act_mean_bwd(la, dout.to(dev), code, dl, accumulate=acc)
        torch.cuda.synchronize()
        got = dl.buf.cpu().view(B, P, K).double() - (base.double() if acc else 0.0)
        err = float((got - lead.grad).abs().max() / lead.grad.abs().max())
        _report("head_act_mean_bwd/%s_P%d_K%d_acc%d" % (act, P, K, acc), err)
        assert err < TOL, (act, P, K, acc, err)
    # the forward it differentiates is sf_head_act_mean
    out = sfhip.head_act_mean(la, code).cpu().double()
    assert float((out - probs.detach().mean(1)).abs().max() / probs.detach().mean(1).abs().max()) < TOL


# ------------------------------------------------------------------------------------------------ CAM kernels
CAM_CASES = list(itertools.product((1, 4), ((7, 7), (3, 5)), (8, 5)))


def _cam_inputs(T, hw, C):
    """A, G [N, T, H, W, C]; G's frame (n=1, t=T-1) is zero, so its weights vanish and its map is the constant 1."""
    g = _gen("cam%d_%d_%d" % (T, hw[0], C))
    N = 2
    A = torch.randn(N, T, hw[0], hw[1], C, generator=g) * 2
    G = torch.randn(N, T, hw[0], hw[1], C, generator=g)
    G += torch.randn(N, T, 1, 1, C, generator=g) * 2.0  # weights of order one: a planted spread of the maps
    G[1, T - 1] = 0.0
    return A, G


def _cam_ref(A, w32):
    """float64 restatement of gradcam_video.py:159-179 from the fp32 activations and the fp32 weights the kernel gets:
    (raw map, its magnitude, normalised map, per-frame range)."""
    Ab = A.double().mean(1)                                            # [N, H, W, C]
    Amag = A.double().abs().mean(1)
    prod = w32.double()[:, :, None, None, :] * Ab[:, None]             # [N, T, H, W, C]
    raw = (1.0 + prod.sum(-1)).clamp_min(0.0)
    mag = 1.0 + (w32.double().abs()[:, :, None, None, :] * Amag[:, None]).sum(-1)
    lo = raw.amin((2, 3), keepdim=True)
    rng = raw.amax((2, 3), keepdim=True) - lo
    norm = torch.where(rng > 0, (raw - lo) / rng.clamp_min(1e-300), torch.zeros_like(raw))
    return raw, mag, norm, rng.view(raw.shape[0], raw.shape[1])


@pytest.mark.parametrize("T,hw,C", CAM_CASES)
def test_cam_weights_and_map(T, hw, C):
    import sfhip
    dev = _dev()
    A, G = _cam_inputs(T, hw, C)
    N, HW = A.shape[0], hw[0] * hw[1]
    ga = R.view(dev, G, 4, C + 9, R.SENTINEL)
    aa = R.view(dev, A, 3, C + 7, R.SENTINEL)
    w = sfhip.cam_weights(ga)
    cam, raw = sfhip.cam_map(aa, w, want_raw=True)
    w2 = sfhip.cam_weights(ga)
    cam2, raw2 = sfhip.cam_map(aa, w2, want_raw=True)
    only = sfhip.cam_map(aa, w)
    torch.cuda.synchronize()
    assert tuple(w.shape) == (N, T, C) and tuple(cam.shape) == (N, T) + hw == tuple(raw.shape)
    assert torch.equal(w, w2) and torch.equal(cam, cam2) and torch.equal(raw, raw2) and torch.equal(cam, only)
    assert R.outside_is(ga) and R.outside_is(aa) and torch.equal(R.inside(ga), G) and torch.equal(R.inside(aa), A)
    # weights: HW - 1 additions and one division
    wref = G.double().mean((2, 3))
    wmag = G.double().abs().mean((2, 3))
    rw = R.rounds(w.cpu(), wref, wmag)
    _report("cam/weights_T%d_%dx%d_C%d_rounds" % (T, hw[0], hw[1], C), rw)
    assert rw <= HW, rw
    assert bool((w.cpu()[1, T - 1] == 0).all())
    # map before normalisation: T - 1 additions and a division for Abar, C fused multiply-adds onto the 1
    ref_raw, mag, ref_norm, rng = _cam_ref(A, w.cpu())
    rr = R.rounds(raw.cpu(), ref_raw, mag)
    _report("cam/raw_T%d_%dx%d_C%d_rounds" % (T, hw[0], hw[1], C), rr)
    assert rr <= (T - 1) + C + 1, rr
    # normalised maps: the planted spread keeps every non-degenerate frame's range >= 1; one frame is constant
    flat = rng.view(-1)
    assert int((flat == 0).sum()) == 1 and float(rng[1, T - 1]) == 0.0
    assert bool((flat[flat > 0] >= 1.0).all()), flat
    e = float((cam.cpu().double() - ref_norm).abs().max())
    _report("cam/norm_T%d_%dx%d_C%d_abs" % (T, hw[0], hw[1], C), e)
    assert e <= 1e-5, e
    assert bool((cam.cpu()[1, T - 1] == 0).all()), "a zero-range frame gives zeros"
    assert float(cam.min()) >= 0.0 and float(cam.max()) <= 1.0
