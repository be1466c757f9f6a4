"""sf_ctx_pool_fwd / _bwd and sf_sample_affine_fwd / _bwd (csrc/ctx_pool.hip) through the binding against the float64
restatements of tests/_ctx_ref.py, at 1e-5 relative L2 per output (the bound and the comparison form of
test_frozen_bn_ops_gpu.py for one-pass memory-bound kernels).

Shapes: C in {3, 8, 30, 32} (3 and 30 take the scalar kernels); positions per sample 1, 63, 165 (two workgroups of a
ragged run) and 300 (three workgroups: sf_ctx_pool_parts says so, the partial merge runs); N in {1, 3}; channel-slice
views at a non-zero offset of a wider pitch, NaN around every input slice and a sentinel around every output slice;
a base one float off 16-byte alignment; logits spanning about +-80; accumulate against first-writer forms held to
prior + fresh exactly; db exactly 0; two runs of everything with the same bits."""
import numpy as np
import pytest
import torch

import _ctx_ref
from _conv_ref import shifted_view
from _elementwise_ref import SENTINEL, inside, outside_is, view

pytestmark = pytest.mark.gpu
TOL = 1e-5
NAN = float("nan")
DIMS = {1: (1, 1, 1), 63: (1, 7, 9), 165: (3, 5, 11), 300: (3, 10, 10)}
# C -> (pitch, offset): float4-addressable slices for 8 / 32, scalar ones for 3 / 30
VIEWS = {3: (8, 2), 8: (16, 4), 30: (36, 3), 32: (40, 4)}
_REF = {}


def _case(C, rows, N, wscale=1.0):
    """Seeded operands and their float64 results, computed once per shape and left unchanged."""
    key = (C, rows, N, wscale)
    if key not in _REF:
        g = torch.Generator().manual_seed(1000 * C + 10 * rows + N)
        T, H, W = DIMS[rows]
        d = dict(x=torch.randn(N, T, H, W, C, generator=g), w=torch.randn(C, generator=g) * wscale / C ** 0.5,
                 b=torch.randn(1, generator=g), dctx=torch.randn(N, C, generator=g),
                 prior=torch.randn(N, T, H, W, C, generator=g), mul=torch.randn(N, C, generator=g) + 1.5,
                 add=torch.randn(N, C, generator=g), dy=torch.randn(N, T, H, W, C, generator=g),
                 dw_prior=torch.randn(C, generator=g))
        d["ctx"], d["lse"] = _ctx_ref.ctx_pool_ref(d["x"], d["w"], d["b"])
        d["dx"], d["dw"], d["db"] = _ctx_ref.ctx_pool_bwd_ref(d["x"], d["w"], d["b"], d["dctx"])
        _REF[key] = d
    return _REF[key]


def _views(d, C, how):
    """(make(vals, fill) -> Act) for the view kind `how`: 'slice' (offset in a wider pitch), 'dense', 'shifted'."""
    dev = torch.device("cuda")
    if how == "dense":
        return lambda v, fill: view(dev, v, 0, C, fill)
    pitch, coff = VIEWS[C]
    if how == "shifted":
        return lambda v, fill: shifted_view(dev, v, coff, pitch, fill)[0]
    return lambda v, fill: view(dev, v, coff, pitch, fill)


def _pool_roundtrip(d, C, how, check_outside=True):
    """Forward, first-writer backward and accumulating backward of one case; returns every output on the CPU."""
    import sfhip
    dev = torch.device("cuda")
    mk = _views(d, C, how)
    x = mk(d["x"], NAN)                               # NaN in every channel the view does not own
    w, b = d["w"].to(dev), d["b"].to(dev)
    ctx, lse = sfhip.ctx_pool(x, w, b)
    dctx = d["dctx"].to(dev)
    ctx64, lse64 = d["ctx"].float().to(dev), d["lse"].float().to(dev)  # the backward is held on exact forward results
    dx_w = mk(torch.full_like(d["x"], 7.0), SENTINEL)  # first writer: every element of the slice is overwritten
    db = torch.full((1,), 5.0, device=dev)
    dw = sfhip.ctx_pool_bwd(x, w, b, lse64, ctx64, dctx, dx_w, accumulate=False, db=db)
    dx_a = mk(d["prior"], SENTINEL)
    dw_a = d["dw_prior"].to(dev).clone()
    sfhip.ctx_pool_bwd(x, w, b, lse64, ctx64, dctx, dx_a, accumulate=True, dw=dw_a, dw_accumulate=True)
    dx_n = mk(torch.full_like(d["x"], 7.0), SENTINEL)  # activation gradient only (the eval-mode tape)
    assert sfhip.ctx_pool_bwd(x, w, b, lse64, ctx64, dctx, dx_n, accumulate=False, want_dw=False) is None
    torch.cuda.synchronize()
    if check_outside and how != "dense":
        assert outside_is(dx_w) and outside_is(dx_a) and outside_is(dx_n), "a channel outside the dx slice changed"
        assert bool(torch.isnan(x.buf[..., :x.coff]).all()) and bool(torch.isnan(x.buf[..., x.coff + C:]).all())
    assert torch.equal(inside(x), d["x"]), "the input was written"
    return dict(ctx=ctx.cpu(), lse=lse.cpu(), dx_w=inside(dx_w), dw=dw.cpu(), db=db.cpu(), dx_a=inside(dx_a),
                dw_a=dw_a.cpu(), dx_n=inside(dx_n))


def _check_pool(d, got, tol=TOL):
    errs = dict(ctx=_ctx_ref.rel_l2(got["ctx"], d["ctx"]), lse=_ctx_ref.rel_l2(got["lse"], d["lse"]),
                dx=_ctx_ref.rel_l2(got["dx_w"], d["dx"]), dw=_ctx_ref.rel_l2(got["dw"], d["dw"]),
                dw_acc=_ctx_ref.rel_l2(got["dw_a"], d["dw_prior"].double() + d["dw"]))
    print("ctx_pool errors", errs)
    for v in got.values():
        assert bool(torch.isfinite(v).all())
    assert all(e <= tol for e in errs.values()), errs
    assert float(d["db"].abs().max()) < 1e-12           # the float64 derivative agrees: shift invariance
    assert got["db"].numpy().tobytes() == np.zeros(1, np.float32).tobytes(), "db is not exactly 0"
    # accumulate == prior + fresh, exactly; the activation-only form writes the same bits
    assert torch.equal(got["dx_a"], d["prior"] + got["dx_w"]), "accumulate is not prior + fresh"
    assert torch.equal(got["dx_n"], got["dx_w"])
    assert torch.equal(got["dw_a"], d["dw_prior"] + got["dw"]), "dw accumulate is not prior + fresh"


@pytest.mark.parametrize("rows", sorted(DIMS))
@pytest.mark.parametrize("C", sorted(VIEWS))
def test_ctx_pool_slices_match_fp64_own_their_memory_and_repeat(C, rows):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sfhip
    assert sfhip.lib().sf_ctx_pool_parts(300) >= 3 and sfhip.lib().sf_ctx_pool_parts(165) == 2
    for N in (1, 3):
        d = _case(C, rows, N)
        got = _pool_roundtrip(d, C, "slice")
        _check_pool(d, got)
        again = _pool_roundtrip(d, C, "slice")
        for k in got:
            assert torch.equal(got[k], again[k]), ("two runs differ", k)


@pytest.mark.parametrize("C", sorted(VIEWS))
def test_ctx_pool_dense_and_misaligned_views(C):
    """A dense view, and a base one float off 16-byte alignment (pitch and offset may be multiples of 4: only the
    pointer check sends it to the scalar kernels) — the same results within the bound; for C = 8 / 32 the misaligned
    run must not take the float4 kernels, so its reduction order — and possibly its last bits — differ."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    for rows in (63, 300):
        d = _case(C, rows, 3)
        _check_pool(d, _pool_roundtrip(d, C, "dense"))
        _check_pool(d, _pool_roundtrip(d, C, "shifted"))


@pytest.mark.parametrize("C", [30, 32])
def test_ctx_pool_logits_spanning_80(C):
    """w scaled so that the logits span about +-80: exp of a raw logit would overflow fp32 sums; the online max-rescale
    (and the partial merge: 300 positions = 3 workgroups) keeps every output finite and within the bound."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = _case(C, 300, 3, wscale=28.0)
    l = (d["x"].double().reshape(3, -1, C) @ d["w"].double()) + d["b"].double()
    assert float(l.max()) > 60.0 and float(l.min()) < -60.0, (float(l.min()), float(l.max()))
    _check_pool(d, _pool_roundtrip(d, C, "slice"))


def _affine_roundtrip(d, C, how, use_mul, use_add):
    import sfhip
    dev = torch.device("cuda")
    mk = _views(d, C, how)
    x, dy = mk(d["x"], NAN), mk(d["dy"], NAN)
    mul = d["mul"].to(dev) if use_mul else None
    add = d["add"].to(dev) if use_add else None
    out = mk(torch.full_like(d["x"], 7.0), SENTINEL)
    sfhip.sample_affine(x, mul=mul, add=add, out=out)
    dx_w = mk(torch.full_like(d["x"], 7.0), SENTINEL)
    dmul, dadd = sfhip.sample_affine_bwd(dy, dx_w, x=x, mul=mul, accumulate=False, want_dmul=True, want_dadd=True)
    dx_a = mk(d["prior"], SENTINEL)
    only = sfhip.sample_affine_bwd(dy, dx_a, mul=mul, accumulate=True, want_dadd=True)  # x is not read
    dx_n = mk(torch.full_like(d["x"], 7.0), SENTINEL)
    none = sfhip.sample_affine_bwd(dy, dx_n, mul=mul, accumulate=False)
    torch.cuda.synchronize()
    assert only[0] is None and none == (None, None)
    if how != "dense":
        assert outside_is(out) and outside_is(dx_w) and outside_is(dx_a) and outside_is(dx_n)
    assert torch.equal(inside(x), d["x"]) and torch.equal(inside(dy), d["dy"]), "an input was written"
    return dict(out=inside(out), dx_w=inside(dx_w), dmul=dmul.cpu(), dadd=dadd.cpu(), dx_a=inside(dx_a),
                dadd2=only[1].cpu(), dx_n=inside(dx_n))


@pytest.mark.parametrize("rows", sorted(DIMS))
@pytest.mark.parametrize("C", sorted(VIEWS))
def test_sample_affine_matches_fp64_owns_its_memory_and_repeats(C, rows):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    for N in (1, 3):
        d = _case(C, rows, N)
        for use_mul, use_add in ((True, True), (True, False), (False, True)):
            for how in ("slice", "shifted") if (N == 3 and use_mul and use_add) else ("slice",):
                got = _affine_roundtrip(d, C, how, use_mul, use_add)
                mul, add = (d["mul"] if use_mul else None), (d["add"] if use_add else None)
                out = _ctx_ref.sample_affine_ref(d["x"], mul, add)
                dx, dmul, dadd = _ctx_ref.sample_affine_bwd_ref(d["dy"], d["x"], mul)
                errs = dict(out=_ctx_ref.rel_l2(got["out"], out), dx=_ctx_ref.rel_l2(got["dx_w"], dx),
                            dmul=_ctx_ref.rel_l2(got["dmul"], dmul), dadd=_ctx_ref.rel_l2(got["dadd"], dadd))
                print("sample_affine errors", how, errs)
                assert all(e <= TOL for e in errs.values()), errs
                assert torch.equal(got["dx_a"], d["prior"] + got["dx_w"]), "accumulate is not prior + fresh"
                assert torch.equal(got["dx_n"], got["dx_w"]) and torch.equal(got["dadd2"], got["dadd"])
                again = _affine_roundtrip(d, C, how, use_mul, use_add)
                for k in got:
                    assert torch.equal(got[k], again[k]), ("two runs differ", k)


def test_sample_affine_in_place():
    """out may alias x element for element."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sfhip
    d = _case(32, 300, 3)
    dev = torch.device("cuda")
    x = view(dev, d["x"], 4, 40, SENTINEL)
    fresh = sfhip.sample_affine(view(dev, d["x"], 4, 40, NAN), mul=d["mul"].to(dev), add=d["add"].to(dev))
    sfhip.sample_affine(x, mul=d["mul"].to(dev), add=d["add"].to(dev), out=x)
    torch.cuda.synchronize()
    assert outside_is(x) and torch.equal(inside(x), inside(fresh))
