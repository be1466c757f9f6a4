"""sf_stripe_pool_fwd, sf_stripe_add_fwd and sf_stripe_pool_bwd (csrc/stripe_pool.hip) through the binding against the
float64 restatements of tests/_nlblock_ref.py, at 1e-5 relative L2 per output (TOL of test_ctx_ops_gpu.py); the positions
of the maxima must equal the restatement's exactly.

Shapes: C in {3, 8, 70} (8 takes the float4 kernels, 3 and 70 the scalar ones, 70 in two channel chunks) and 264 (the
float4 kernels in two chunks); frames of 6 x 5 (stripes of 30, 15 and 5 positions: fewer than position lanes) and of
4 x 70 (280, 140 and 70 positions: more than one workgroup pass in the pooling, more than one workgroup per stripe in
the add / backward); S in {1, 2, H}; dense views and channel slices at a non-zero offset of a wider pitch.  Every
buffer sits between guard floats and holds a sentinel (NaN for inputs) in every channel its view does not own: all of
it must survive.  Equal maxima planted within and across the position lanes go to the first position; accumulate is
prior + fresh exactly; NULL dz / dmean / dmax in every combination; two runs of everything give the same bits.
Observed on an MI355X: at most 7.9e-8 over all outputs."""
import itertools

import pytest
import torch

import _nlblock_ref as R
from _elementwise_ref import SENTINEL, inside, outside_is

pytestmark = pytest.mark.gpu
TOL = 1e-5
NAN = float("nan")
GUARD = 64  # floats in front of and behind every buffer (a multiple of 4: the buffer stays 16-byte aligned)
DIMS = {"6x5": (2, 2, 6, 5), "4x70": (1, 2, 4, 70)}
# C -> (pitch, offset): float4-addressable slices for 8 / 264, scalar ones for 3 / 70
VIEWS = {3: (8, 2), 8: (16, 4), 70: (76, 3), 264: (272, 4)}
MODES = ("mean", "max", "meanmax", "sum")
_REF = {}


def _guarded(vals, coff, pitch, fill, dtype=torch.float32):
    """Act over channels [coff, coff + C) of a [.., pitch] buffer cut out of an allocation with GUARD elements of `fill`
    on either side; every channel outside the view holds `fill` too.  -> (Act, allocation)."""
    import sfhip
    C = vals.shape[-1]
    shape = tuple(vals.shape[:-1]) + (pitch,)
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype)
    flat[GUARD:GUARD + n].view(shape)[..., coff:coff + C] = vals
    flat = flat.cuda()
    buf = flat[GUARD:GUARD + n].view(shape)
    assert buf.data_ptr() % 16 == 0
    return sfhip.Act(buf, coff, C), flat


def _guards_hold(flat, fill=SENTINEL):
    g = torch.cat([flat[:GUARD], flat[-GUARD:]]).cpu()
    return bool(torch.isnan(g).all()) if fill != fill else torch.equal(g, torch.full_like(g, fill))


def _owned_only(act, flat, fill=SENTINEL):
    """Nothing outside the view changed: the guards, and (for a slice) the other channels of the pitch."""
    if not _guards_hold(flat, fill):
        return False
    if act.cs == act.C:
        return True
    if fill != fill:
        return bool(torch.isnan(act.buf[..., :act.coff]).all()) and bool(torch.isnan(act.buf[..., act.coff + act.C:]).all())
    return outside_is(act, fill)


def _case(C, dims, S):
    """Seeded operands and their float64 results, computed once per shape and left unchanged."""
    key = (C, dims, S)
    if key not in _REF:
        N, T, H, W = DIMS[dims]
        g = torch.Generator().manual_seed(100000 * S + 100 * C + H)
        d = dict(x=torch.randn(N, T, H, W, C, generator=g), dz=torch.randn(N, T, H, W, C, generator=g),
                 prior=torch.randn(N, T, H, W, C, generator=g), v=torch.randn(N, T, S, 1, C, generator=g),
                 dmean=torch.randn(N, T, S, 1, C, generator=g), dmax=torch.randn(N, T, S, 1, C, generator=g))
        d["pool"] = {m: R.stripe_pool_ref(d["x"], S, m) for m in MODES}
        d["add"] = R.stripe_add_ref(d["x"], d["v"].reshape(N, T, S, C))
        _REF[key] = d
    return _REF[key]


def _mk(C, how):
    pitch, coff = (C, 0) if how == "dense" else VIEWS[C]
    return lambda vals, fill: _guarded(vals, coff, pitch, fill)


def _forward(d, C, S, how):
    """The four pools and the add of one case -> every output on the CPU; asserts owned memory."""
    import sfhip
    mk = _mk(C, how)
    x, xflat = mk(d["x"], NAN)
    N, T = d["x"].shape[:2]
    got = {}
    for mode in MODES:
        cout = 2 * C if mode == "meanmax" else C
        pitch, coff = (cout, 0) if how == "dense" else (cout + 12, 8)
        out, oflat = _guarded(torch.full((N, T, S, 1, cout), 3.0), coff, pitch, SENTINEL)
        res, arg = sfhip.stripe_pool(x, S, mode, out=out)
        torch.cuda.synchronize()
        assert res is out and _owned_only(out, oflat), (mode, "memory outside the output slice changed")
        assert (arg is None) == (mode in ("mean", "sum"))
        got[mode] = inside(out).reshape(N, T, S, cout)
        if arg is not None:
            assert arg.dtype == torch.int32 and tuple(arg.shape) == (N, T, S, C)
            got[mode + "/arg"] = arg.cpu()
    v, vflat = mk(d["v"], NAN)
    z, zflat = mk(torch.full_like(d["x"], 3.0), SENTINEL)
    assert sfhip.stripe_add(x, v, out=z) is z
    torch.cuda.synchronize()
    assert _owned_only(z, zflat) and _owned_only(x, xflat, NAN) and _owned_only(v, vflat, NAN)
    assert torch.equal(inside(x), d["x"]) and torch.equal(inside(v), d["v"]), "an input was written"
    got["add"] = inside(z)
    return got


def _check_forward(d, got, S):
    for mode in MODES:
        ref, arg = d["pool"][mode]
        e = R.rel_l2(got[mode], ref)
        print("stripe_pool %-8s S=%d rel L2 %.3e" % (mode, S, e))
        assert bool(torch.isfinite(got[mode]).all()) and e <= TOL, (mode, e)
        if arg is not None:
            assert torch.equal(got[mode + "/arg"].long(), arg), (mode, "positions of the maxima differ")
    e = R.rel_l2(got["add"], d["add"])
    print("stripe_add S=%d rel L2 %.3e" % (S, e))
    assert e <= TOL, e
    c = got["mean"].shape[-1]
    assert torch.equal(got["meanmax"][..., :c], got["mean"]) and torch.equal(got["meanmax"][..., c:], got["max"])
    assert torch.equal(got["meanmax/arg"], got["max/arg"])


def _backward(d, C, S, how, use, arg):
    """First-writer and accumulating backward with the terms named in `use` -> (dx_w, dx_a) on the CPU."""
    import sfhip
    mk = _mk(C, how)
    terms, flats = {}, []
    for name in ("dz", "dmean", "dmax"):
        terms[name] = None
        if name in use:
            terms[name], f = mk(d[name], NAN)
            flats.append((terms[name], f))
    dev_arg = arg.to(torch.int32).cuda() if "dmax" in use else None
    dx_w, wflat = mk(torch.full_like(d["x"], 3.0), SENTINEL)  # first writer: every element of the slice is overwritten
    dx_a, aflat = mk(d["prior"], SENTINEL)
    sfhip.stripe_pool_bwd(dx_w, S, arg=dev_arg, accumulate=False, **terms)
    sfhip.stripe_pool_bwd(dx_a, S, arg=dev_arg, accumulate=True, **terms)
    torch.cuda.synchronize()
    assert _owned_only(dx_w, wflat) and _owned_only(dx_a, aflat), "memory outside the dx slice changed"
    for a, f in flats:
        assert _owned_only(a, f, NAN)
    return inside(dx_w), inside(dx_a)


COMBOS = [c for k in range(4) for c in itertools.combinations(("dz", "dmean", "dmax"), k)]


@pytest.mark.parametrize("dims", sorted(DIMS))
@pytest.mark.parametrize("C", sorted(VIEWS))
def test_stripe_kernels_match_fp64_own_their_memory_and_repeat(C, dims):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    H = DIMS[dims][2]
    assert len(COMBOS) == 8
    for S in (1, 2, H):
        d = _case(C, dims, S)
        N, T = d["x"].shape[:2]
        arg = d["pool"]["max"][1]
        for how in ("dense", "slice"):
            got = _forward(d, C, S, how)
            _check_forward(d, got, S)
            again = _forward(d, C, S, how)
            for k in got:
                assert torch.equal(got[k], again[k]), ("two runs differ", k)
            for use in COMBOS if how == "slice" else (("dz", "dmean", "dmax"), ()):
                kw = {k: d[k].reshape(N, T, S, C) if k != "dz" else d[k] for k in use}
                ref = R.stripe_pool_bwd_ref(d["x"].shape, S, arg=arg, **kw)
                dx_w, dx_a = _backward(d, C, S, how, use, arg)
                e = R.rel_l2(dx_w, ref)
                print("stripe_pool_bwd %-22s S=%d rel L2 %.3e" % ("+".join(use) or "nothing", S, e))
                assert bool(torch.isfinite(dx_w).all()) and e <= TOL, (use, e)
                if not use:
                    assert not bool(dx_w.any()), "accumulate == 0 with no term must write zeros"
                assert torch.equal(dx_a, d["prior"] + dx_w), "accumulate is not prior + fresh"
                w2, a2 = _backward(d, C, S, how, use, arg)
                assert torch.equal(w2, dx_w) and torch.equal(a2, dx_a), "two runs differ"


@pytest.mark.parametrize("C", sorted(VIEWS))
def test_equal_maxima_go_to_the_first_position(C):
    """Equal values planted in a stripe of 280 positions: in one position lane (l and l + 256 / CB) and across lanes,
    early and late; one channel constant over the whole stripe (position 0); one channel whose maximum is its last
    position.  The forward's positions and the backward's routing must be the restatement's."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sfhip
    N, T, H, W = DIMS["4x70"]
    g = torch.Generator().manual_seed(77 + C)
    x = torch.randn(N, T, H, W, C, generator=g).clamp(-3.0, 3.0)
    flat = x.view(N, T, H * W, C)
    for pos in (279, 7, 263, 135, 8):          # 7 and 263 share a lane for every CB (256 apart); 8 is its neighbour
        flat[:, :, pos, 0] = 9.0
    flat[0, 0, :, 1] = 1.25                     # constant: the first position
    flat[:, :, 279, 2] = 11.0                   # the last position
    flat[:, 1, 140:, C - 1] = flat[:, 1, :140, C - 1]  # the two half-frame stripes of S = 2 hold the same values
    for S in (1, 2):
        ref, arg = R.stripe_pool_ref(x, S, "max")
        if S == 1:
            assert arg[0, 0, 0, :3].tolist() == [7, 0, 279]
        for how in ("dense", "slice"):
            xa, _ = _mk(C, how)(x, NAN)
            out, got = sfhip.stripe_pool(xa, S, "max")
            dmax = torch.randn(N, T, S, 1, C, generator=g)
            dx, dflat = _mk(C, how)(torch.full_like(x, 3.0), SENTINEL)
            sfhip.stripe_pool_bwd(dx, S, dmax=_mk(C, how)(dmax, NAN)[0], arg=got, accumulate=False)
            torch.cuda.synchronize()
            assert torch.equal(got.cpu().long(), arg), "a tie did not go to the first position"
            assert torch.equal(inside(out).reshape(N, T, S, C).double(), ref)  # a maximum is one of the inputs: exact
            want = R.stripe_pool_bwd_ref(x.shape, S, dmax=dmax.reshape(N, T, S, C), arg=arg)
            assert torch.equal(inside(dx).double(), want) and _owned_only(dx, dflat)
            assert int((inside(dx) != 0).sum()) <= N * T * S * C  # one position per (stripe, channel), no more


def test_the_add_may_alias_its_input():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sfhip
    d = _case(8, "4x70", 2)
    x, flat = _guarded(d["x"], 4, 16, SENTINEL)
    v, _ = _guarded(d["v"], 4, 16, NAN)
    fresh = sfhip.stripe_add(_guarded(d["x"], 4, 16, NAN)[0], v)
    sfhip.stripe_add(x, v, out=x)
    torch.cuda.synchronize()
    assert _owned_only(x, flat) and torch.equal(inside(x), inside(fresh))
    assert fresh.cs == fresh.C == 8
