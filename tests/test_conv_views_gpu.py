"""Op-level parity and owned memory of the conv family — sfhip.conv, conv_dgrad, conv_wgrad and sf_conv_wgrad_finish
on channel slices of wider buffers — against float64 CPU references of the same fp32 inputs (tests/_conv_ref.py).

Views.  Every activation is a slice (buffer, coff, C, pitch).  Inputs sit between NaN channels and must come back
unchanged (whole buffer, compared as int32 so the NaNs compare); outputs sit between sentinel channels that must come
back bit for bit; a view a kernel overwrites starts as NaN, one it accumulates into as a seeded base.  Each case runs
  aligned      input (coff 4, pitch C + 12), output (coff 8, pitch C + 12), residual (coff 4, pitch C + 8)
  misaligned   input (coff 3, pitch C + 5),  output (coff 1, pitch C + 3),  residual (coff 2, pitch C + 3)
and, beyond those two, with only the input or only the output misaligned (the kernels decide the vector width of their
loads and of their stores separately: a misaligned input under an aligned output is the LDS-tiled kernel's float4
epilogue, the reverse its scalar epilogue under float4 loads) and, for the shapes the bf16-piece and per-wavefront
kernels take by shape, `shifted`: the aligned offsets and pitches in a buffer that starts one float into its allocation.
The misaligned pitches are visible in the descriptor, so the shape-only planners already decline them; `shifted` is the
one view whose refusal happens at RUN time (conv_igemm.hip, "a shape they take by shape but refused at run time"), with
the workspace the shape-only planner sized.

Bound.  |got - ref| <= (K + 8) * 2^-24 * mag per element, mag = the sum of |terms| added into it, K = the number of
products (taps * Cin forward, taps * Cout data gradient, N * To * Ho * Wo weight gradient, S for the split sum): the
worst case of an fp32 sum in any order, see _conv_ref.py.  Elements with mag == 0 must be exact.  The max-norm 2e-4
of test_backward_ops_gpu.py stays as a second assertion.  The worst element of every case is appended to
conv_views_report.txt, beside the other op-level reports, in units of 2^-24 * mag.

Routes.  Each case names the kernel its aligned run is meant for.  Where an exported planner tells routes apart the test
asserts on it (sf_conv_rows_parts, sf_conv_pw_ws_floats, sf_conv_bx_ws_floats, sf_conv_fwd_ws_floats,
sf_conv_wgrad_splits, sf_conv_wgrad_bx_ws_floats / _splits); the rest follows from the *_takes / *_plan predicates
quoted beside the case.  Kernels that are off by default for a shape are forced with sf_conv_tune, as their own tests do."""
import ctypes

import pytest
import torch

import _conv_ref as C
import _elementwise_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-4
NAN = float("nan")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _report(name, err):
    """One line per case in conv_views_report.txt, beside the other op-level reports."""
    from test_backward_ops_gpu import _report as report
    report(name, err, "conv_views_report.txt")


@pytest.fixture
def tune():
    import sfhip
    L = sfhip.lib()
    yield L
    for knob, v in ((0, 1), (1, -1), (2, 0), (4, 1), (6, 1), (7, 1), (9, 1), (10, 1), (11, -1), (12, 0), (20, 1),
                    (21, 1), (22, 1), (23, -1)):
        L.sf_conv_tune(knob, v)


def _case(name, cin, cout, k, s, p, nthw, **kw):
    d = dict(name=name, cin=cin, cout=cout, k=k, s=s, p=p, nthw=nthw, res=False, act=False, tune=(), route="")
    d.update(kw)
    return d


ONE = (1, 1, 1)

# views: name -> ((input coff, extra pitch), (output coff, extra pitch), (residual coff, extra pitch), shifted)
VIEWS = {
    "aligned": ((4, 12), (8, 12), (4, 8), False),
    "misaligned": ((3, 5), (1, 3), (2, 3), False),
    "in_misaligned": ((3, 5), (8, 12), (4, 8), False),
    "out_misaligned": ((4, 12), (1, 3), (2, 3), False),
    "shifted": ((4, 12), (8, 12), (4, 8), True),
}

# ---------------------------------------------------------------------------------------------------- forward
# route: the kernel of the ALIGNED run.  With a misaligned input pitch every specialised kernel declines (rows / small /
# pw / bx / wave all require in_cs % 4 == 0 and in_coff % 4 == 0) and the LDS-tiled implicit GEMM of conv_igemm.hip runs
# with scalar loads; with only the output misaligned rows / small / wave decline (out_cs % 4) and it runs with float4
# loads and the scattered epilogue.  K = taps * Cin <= 1200 everywhere.
FWD_CASES = [
    # conv_rows.hip, window form (crows_plan: stride 1 "same", 3x1x1, 8 <= C, one side <= 32, M >= 1024; level 2 =
    # sf_conv_tune(22, 2) because To = 1 keeps the ring form out): M = 5115 = 39 stages of 128 + 123
    _case("rows_t3_8_16", 8, 16, (3, 1, 1), ONE, (1, 0, 0), (5, 1, 33, 31), res=True, act=True, tune=((22, 2),),
          route="rows"),
    # conv_rows.hip, 1x3x3 window with its halo (level 2 also lifts the 8 -> 8 exclusion); M = 1150
    _case("rows_s3_8_8", 8, 8, (1, 3, 3), ONE, (0, 1, 1), (1, 2, 23, 25), tune=((22, 2),), route="rows"),
    # conv_small.hip (sf_conv_small_takes: 8 -> 8 spatial, M = 4480 >= 4096; conv_rows declines at its default level)
    _case("small_s3_8_8", 8, 8, (1, 3, 3), ONE, (0, 1, 1), (2, 4, 20, 28), res=True, act=True, route="small"),
    # conv_wave.hip, plain persistent form (1x1x1, nk = 4 <= 5, Cout >= 32); M = 576 < 2048 keeps conv_pw_bx out
    _case("wave_plain_64_256", 64, 256, ONE, ONE, (0, 0, 0), (2, 2, 12, 12), act=6, route="wave"),
    # conv_pw_bx_kernel (pw_plan: 1x1x1, Cin % 16 == 0, Cin, Cout >= 64, M = 2116 >= 2048 = 8 tiles of 256 + 68 rows;
    # its time model keeps so small a layer on the f32 kernels: sf_conv_tune(21, 2))
    _case("pw_64_256", 64, 256, ONE, ONE, (0, 0, 0), (2, 2, 23, 23), res=True, act=True, tune=((21, 2),), route="pw"),
    # strided pointwise: pw_plan wants stride 1, bx_plan nk = 18 < 32 -> conv_wave.hip with strided row addresses, M = 98
    _case("wave_pw_s2_288_512", 288, 512, ONE, (1, 2, 2), (0, 0, 0), (1, 2, 14, 14), act=True, route="wave"),
    # Cout = 64 < 128 keeps conv_bx out -> conv_wave.hip, border taps; M = 392
    _case("wave_s3_64_64", 64, 64, (1, 3, 3), ONE, (0, 1, 1), (1, 2, 14, 14), res=True, act=True, route="wave"),
    # conv_bx.hip (bx_plan: Cin % 16 == 0, Cout >= 128, nk = 36 >= 32, M = 2112 >= 2048 = 8 tiles of 256 + 64 rows; its
    # win / lose rule keeps so small a layer on conv_wave: sf_conv_tune(7, 2))
    _case("bx_s3_64_128", 64, 128, (1, 3, 3), ONE, (0, 1, 1), (1, 2, 33, 32), tune=((7, 2),), route="bx"),
    # conv_wave.hip, temporal borders, K split across the workgroup's wavefronts; M = 392
    _case("wave_t3_128_64", 128, 64, (3, 1, 1), ONE, (1, 0, 0), (2, 4, 7, 7), res=True, act=True, route="wave"),
    # Cin = 27: no float4 anywhere -> conv_igemm_kernel<.., 1>, 256 x 16 tile; M = 200
    _case("igemm_scalar_27_16", 27, 16, ONE, ONE, (0, 0, 0), (2, 4, 5, 5), act=True, route="igemm"),
    # strided in T and H with odd extents, Cout = 40 = 2.5 column blocks of 16; M = 100 (conv_wave when aligned)
    _case("wave_s2t_24_40", 24, 40, (3, 3, 1), (2, 2, 1), (1, 1, 0), (1, 7, 9, 5), res=True, act=True, route="wave"),
    # M = 8 <= 16: sf_conv_wave_takes declines, gemv_rows_kernel (float4 input) / the LDS-tiled kernel (scalar input)
    _case("gemv_256_40", 256, 40, ONE, ONE, (0, 0, 0), (2, 1, 2, 2), route="gemv"),
    # Cout = 72 = 4.5 column blocks of 16 / 1.125 of 64; M = 297
    _case("wave_s3_16_72", 16, 72, (1, 3, 3), ONE, (0, 1, 1), (1, 3, 9, 11), res=True, act=True, route="wave"),
    # K = 1152 (nk = 72 >= 48) into 64 channels over 6 row tiles of 128 (M = 765): conv_wave when aligned; with a
    # misaligned INPUT nothing takes the shape and sf_conv_fwd_ws_floats plans split-K partial tiles (splitk_factor > 1)
    _case("splitk_s3_128_64", 128, 64, (1, 3, 3), ONE, (0, 1, 1), (1, 3, 15, 17), act=True, route="wave"),
]
SHIFTED_FWD = ("wave_plain_64_256", "pw_64_256", "bx_s3_64_128", "wave_t3_128_64", "rows_t3_8_16", "small_s3_8_8")
FWD_RUNS = [(c, v) for c in FWD_CASES for v in VIEWS if v != "shifted" or c["name"] in SHIFTED_FWD]

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _fwd_reference(case):
    def make():
        t = C.conv_inputs(case)
        res = t["res"] if case["res"] else None
        ref, mag = C.conv_ref(t["x"], t["w"], t["bias"], t["scale"], res, case["act"], case["s"], case["p"])
        return t, ref, mag
    return _cached(("fwd", case["name"]), make)


def _make_view(dev, vals, spec, fill, shifted):
    """-> (Act, the allocation in front of which one more float is checked, or None)."""
    coff, extra = spec
    if shifted:
        return C.shifted_view(dev, vals, coff, vals.shape[-1] + extra, fill)
    return R.view(dev, vals, coff, vals.shape[-1] + extra, fill), None


def _snapshot(act):
    return act.buf.clone()


def _unchanged(act, snap):
    return torch.equal(act.buf.view(torch.int32), snap.view(torch.int32))


def _front_ok(alloc, fill):
    if alloc is None:
        return True
    want = torch.tensor([fill], dtype=torch.float32)
    return torch.equal(alloc[:1].cpu().view(torch.int32), want.view(torch.int32))


def _apply_tune(L, case):
    for knob, v in case["tune"]:
        assert L.sf_conv_tune(knob, v) == 0


def _check(tag, got, ref, mag, K):
    """The three numeric assertions of a case: finite, the rounding bound (exact where nothing is added), max-norm."""
    assert bool(torch.isfinite(got).all()), tag + ": non-finite output inside the view"
    r = R.rounds(got, ref, mag)
    _report(tag, r)
    print("%-60s worst %.3f of %.0f allowed (units of 2^-24 * mag)" % (tag, r, C.bound(K)))
    assert r <= C.bound(K), (tag, r, C.bound(K))
    assert R.rel(got, ref) < TOL, (tag, R.rel(got, ref))


def _fwd_route(L, d, case, view, nws_expected=None):
    """What the exported planners say about the descriptor of this run."""
    by = ctypes.byref(d)
    rows, pw, bx = L.sf_conv_rows_parts(by), L.sf_conv_pw_ws_floats(by, 1), L.sf_conv_bx_ws_floats(by, 0, 1)
    nws = L.sf_conv_fwd_ws_floats(by)
    route = case["route"]
    if view in ("aligned", "shifted"):
        assert (rows > 0) == (route == "rows"), (case["name"], rows)
        assert (pw > 0) == (route == "pw"), (case["name"], pw)
        assert (bx > 0) == (route == "bx"), (case["name"], bx)
        if route in ("pw", "bx"):
            assert nws > 0      # weight planes (+ partial tiles): what a run-time refusal hands the generic kernel
        else:
            assert nws == 0     # no split-K partials: conv_wave / gemv / the one-pass LDS-tiled kernel
    elif view in ("misaligned", "in_misaligned"):
        assert rows == 0 and pw == 0 and bx == 0, case["name"]  # every specialised kernel reads float4 rows
        M = d.N * d.To * d.Ho * d.Wo
        if case["name"] == "splitk_s3_128_64":
            assert nws > 0 and nws % (M * d.Cout) == 0 and nws // (M * d.Cout) > 1, nws
        else:
            assert nws == 0, (case["name"], nws)


@pytest.mark.parametrize("case,view", FWD_RUNS, ids=["%s-%s" % (c["name"], v) for c, v in FWD_RUNS])
def test_conv_forward_views(case, view, tune):
    import sfhip
    dev = _dev()
    t, ref, mag = _fwd_reference(case)
    xin, xout, xres, shifted = VIEWS[view]
    _apply_tune(tune, case)
    xa, xalloc = _make_view(dev, t["x"], xin, NAN, shifted)
    ra = ralloc = None
    if case["res"]:
        ra, ralloc = _make_view(dev, t["res"], xres, NAN, shifted)
    oa, oalloc = _make_view(dev, torch.full(ref.shape, NAN), xout, R.SENTINEL, shifted)
    wp = sfhip.pack_conv_weight(t["w"].to(dev))
    scale, bias = t["scale"].to(dev), t["bias"].to(dev)
    d = sfhip._conv_desc(xa, ref.shape[1:4], oa.cs, oa.coff, case["cout"], case["k"], case["s"], case["p"],
                         cin_pad=wp.shape[2], act=sfhip._act(case["act"]), res=ra)
    _fwd_route(tune, d, case, view)
    xs, rs, ws = _snapshot(xa), (_snapshot(ra) if ra else None), wp.clone()
    ret = sfhip.conv(xa, wp, case["k"], case["s"], case["p"], scale=scale, bias=bias, relu=case["act"], res=ra, out=oa)
    torch.cuda.synchronize()
    assert ret is oa
    tag = "fwd/%s/%s" % (case["name"], view)
    assert R.outside_is(oa) and _front_ok(oalloc, R.SENTINEL), tag + ": a store outside the output view"
    k = case["k"]
    _check(tag, R.inside(oa), ref, mag, k[0] * k[1] * k[2] * case["cin"])
    assert _unchanged(xa, xs) and (ra is None or _unchanged(ra, rs)) and torch.equal(wp, ws), tag + ": an input changed"
    assert _front_ok(xalloc, NAN) and _front_ok(ralloc, NAN)


# ---------------------------------------------------------------------------------------------------- data gradient
# dz is read from a slice (the input view), dx is a slice (the output view; when accumulating it is also the residual).
# K = taps * Cout.  modes: accumulate values to run.
DGRAD_CASES = [
    # stride 1 — the transposed descriptor goes through the same dispatch as a forward conv of Cout -> Cin channels
    _case("rows_t3_8_16", 8, 16, (3, 1, 1), ONE, (1, 0, 0), (5, 1, 33, 31), tune=((22, 2),), route="rows",
          modes=(True, False)),
    _case("small_s3_8_8", 8, 8, (1, 3, 3), ONE, (0, 1, 1), (2, 4, 20, 28), route="small", modes=(True, False)),
    _case("wave_t3_128_64", 128, 64, (3, 1, 1), ONE, (1, 0, 0), (2, 4, 7, 7), route="wave", modes=(True, False)),
    _case("wave_s3_64_64", 64, 64, (1, 3, 3), ONE, (0, 1, 1), (1, 2, 14, 14), route="wave", modes=(True, False)),
    # dx has 27 channels: scalar stores whatever the view
    _case("igemm_scalar_27_16", 27, 16, ONE, ONE, (0, 0, 0), (2, 4, 5, 5), route="igemm", modes=(True, False)),
    # strided.  accumulate=False into a SLICE: sfhip.conv_dgrad may not zero the buffer, so it takes the transposed
    # gather (d.transposed with a stride: conv_wave and conv_bx decline, conv_igemm_kernel predicates the taps that do
    # not divide).  accumulate=True: one dense conv per residue class with a scattered store (os_* > 1) into the slice
    _case("s3_s2_128_128", 128, 128, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 2, 14, 14), route="gather",
          modes=(False, True)),
    _case("k5_s2_48_32", 48, 32, (1, 5, 5), (1, 2, 2), (0, 2, 2), (2, 2, 13, 11), route="gather", modes=(False, True)),
    # 1x1x1 stride 2: three of four residue classes get no tap — exact zeros, not the NaNs the slice held
    _case("pw_s2_64_128", 64, 128, ONE, (1, 2, 2), (0, 0, 0), (1, 2, 14, 14), route="gather", modes=(False,)),
    _case("k7_s4_32_64", 32, 64, (7, 1, 1), (4, 1, 1), (3, 0, 0), (1, 16, 6, 6), route="gather", modes=(False,)),
    _case("s2t_24_40", 24, 40, (3, 3, 1), (2, 2, 1), (1, 1, 0), (1, 7, 9, 5), route="gather", modes=(False, True)),
]
DGRAD_VIEWS = ("aligned", "misaligned", "in_misaligned", "out_misaligned")
DGRAD_RUNS = [(c, v, a) for c in DGRAD_CASES for v in DGRAD_VIEWS for a in c["modes"]]


def _dgrad_reference(case, accumulate):
    def make():
        t = C.conv_inputs(case)
        ref, mag = C.dgrad_ref(t["dz"], t["w"], t["x"].shape, case["s"], case["p"],
                               base=t["base_dx"] if accumulate else None)
        return t, ref, mag
    return _cached(("dgrad", case["name"], accumulate), make)


@pytest.mark.parametrize("case,view,accumulate", DGRAD_RUNS,
                         ids=["%s-%s-%s" % (c["name"], v, "acc" if a else "write") for c, v, a in DGRAD_RUNS])
def test_conv_dgrad_views(case, view, accumulate, tune):
    import sfhip
    dev = _dev()
    t, ref, mag = _dgrad_reference(case, accumulate)
    xin, xout, _, shifted = VIEWS[view]
    _apply_tune(tune, case)
    dza, _ = _make_view(dev, t["dz"], xin, NAN, shifted)
    dxa, _ = _make_view(dev, t["base_dx"] if accumulate else torch.full(ref.shape, NAN), xout, R.SENTINEL, shifted)
    wtp = sfhip.pack_conv_weight(t["w"].transpose(0, 1).contiguous().to(dev))
    strided = max(case["s"]) > 1
    if not strided and view == "aligned":
        d = sfhip._conv_desc(dza, (dxa.T, dxa.H, dxa.W), dxa.cs, dxa.coff, case["cin"], case["k"], case["s"], case["p"],
                             cin_pad=wtp.shape[2], res=dxa if accumulate else None, transposed=1)
        rows = tune.sf_conv_rows_parts(ctypes.byref(d))
        assert (rows > 0) == (case["route"] == "rows"), (case["name"], rows)
        assert tune.sf_conv_fwd_ws_floats(ctypes.byref(d)) == 0
    zs, ws = _snapshot(dza), wtp.clone()
    ret = sfhip.conv_dgrad(dza, wtp, dxa, case["k"], case["s"], case["p"], out=dxa, accumulate=accumulate)
    torch.cuda.synchronize()
    assert ret is dxa
    tag = "dgrad/%s/%s/%s" % (case["name"], view, "acc" if accumulate else "write")
    assert R.outside_is(dxa), tag + ": a store outside the dx view"
    k = case["k"]
    got = R.inside(dxa)
    _check(tag, got, ref, mag, k[0] * k[1] * k[2] * case["cout"])
    if case["name"] == "pw_s2_64_128":
        untapped = torch.ones(ref.shape[1:4], dtype=torch.bool)
        untapped[:, ::2, ::2] = False
        assert bool((mag[:, untapped] == 0).all()) and bool((mag[:, ~untapped] > 0).all())
        assert bool((got[:, untapped] == 0.0).all()), tag + ": a residue class no tap reaches is not exactly zero"
    assert _unchanged(dza, zs) and torch.equal(wtp, ws), tag + ": an input changed"


# ---------------------------------------------------------------------------------------------------- weight gradient
# x and dz are both slices.  K = N * To * Ho * Wo.  route: the kernel of the aligned run; `planner`: how the test tells —
#   wave          sf_conv_wgrad_splits changes when the kernel is switched off (sf_conv_tune(10, 0))
#   rows          by predicate (rows_plan): on these small shapes its split count coincides with the LDS-tiled plan's,
#                 so switching it off (sf_conv_tune(20, 0)) may not move the planner; where it does, rows is the route
#   tiled         the count changes with neither switch (neither kernel takes the shape)
#   bx            sf_conv_wgrad_bx_ws_floats > 0 and sf_conv_wgrad_bx_splits > 0
WGRAD_CASES = [
    # conv_wgrad_rows.hip (rows_plan: stride 1 "same", 1x3x3, 8 <= C, one side <= 32, float4 x rows); Cin = 8 < cin_pad 16.
    # M = K = 4480 is the shape the route's own tests use; the next case keeps K <= 1200
    _case("rows_s3_8_8", 8, 8, (1, 3, 3), ONE, (0, 1, 1), (2, 4, 20, 28), route="rows"),
    _case("rows_s3_8_8_k1120", 8, 8, (1, 3, 3), ONE, (0, 1, 1), (1, 2, 20, 28), route="rows"),
    # conv_wgrad_wave.hip (wg_plan: both sides >= 64, M = 1176 >= 1024, Wo >= 4): 1x2 blocks, 5 tiles, 3 splits
    _case("wave_s3_64_64", 64, 64, (1, 3, 3), ONE, (0, 1, 1), (3, 2, 14, 14), route="wave"),
    # M = 784 < 1024: wg_plan declines -> conv_wgrad_kernel<64, 64>
    _case("tiled_s3_64_64", 64, 64, (1, 3, 3), ONE, (0, 1, 1), (2, 2, 14, 14), route="tiled"),
    # M = 392: conv_wgrad_kernel<64, 128> (wgrad_tile: 128 on the side that has 128 channels)
    _case("tiled_t3_128_64", 128, 64, (3, 1, 1), ONE, (1, 0, 0), (2, 4, 7, 7), route="tiled"),
    # 1x1x1, 8 -> 24: conv_wgrad_rows when x is float4-addressable, else conv_wgrad_small_kernel<32, 16>; cin_pad 16
    _case("rows_pw_8_24", 8, 24, ONE, ONE, (0, 0, 0), (2, 4, 9, 9), route="rows"),
    # Cin = 27 < cin_pad 32: conv_wgrad_small_kernel<16, 32>, scalar loads
    _case("small_odd_27_16", 27, 16, ONE, ONE, (0, 0, 0), (2, 4, 5, 5), route="tiled"),
]
WGRAD_VIEWS = {
    # name -> (x view, dz view)
    "aligned": ((4, 12), (8, 12)),
    "misaligned": ((3, 5), (1, 3)),
    # x float4-addressable, dz not: the rows / wave / bx kernels take the shape and refuse the call at run time, the
    # LDS-tiled kernel runs with the split count THEIR plan gave (and scalar loads: vec4 is false for dz alone)
    "dz_misaligned": ((4, 12), (1, 3)),
}
WGRAD_RUNS = [(c, v) for c in WGRAD_CASES for v in WGRAD_VIEWS]


def _wgrad_reference(case):
    def make():
        t = C.conv_inputs(case)
        ref, mag = C.wgrad_ref(t["x"], t["dz"], t["w"].shape, case["s"], case["p"])
        return t, ref, mag
    return _cached(("wgrad", case["name"]), make)


def _wgrad_desc(sfhip, xa, dza, case, cin_pad):
    return sfhip._conv_desc(xa, (dza.T, dza.H, dza.W), 0, 0, case["cout"], case["k"], case["s"], case["p"],
                            cin=case["cin"], cin_pad=cin_pad)


def _wgrad_route(L, d, case, view):
    by = ctypes.byref(d)
    s_on = L.sf_conv_wgrad_splits(by)
    assert L.sf_conv_tune(20, 0) == 0
    s_norows = L.sf_conv_wgrad_splits(by)
    assert L.sf_conv_tune(20, 1) == 0 and L.sf_conv_tune(10, 0) == 0
    s_nowave = L.sf_conv_wgrad_splits(by)
    assert L.sf_conv_tune(10, 1) == 0
    bx = L.sf_conv_wgrad_bx_ws_floats(by, 0, 0)
    route = case["route"] if view != "misaligned" else "tiled"   # every specialised plan wants float4 x rows
    assert s_on > 0
    assert s_on == s_norows or route == "rows", (case["name"], view, s_on, s_norows)
    # (a bx shape is also a conv_wgrad_wave shape: that plan serves it when sf_conv_wgrad_bx refuses the call)
    assert (s_on != s_nowave) == (route in ("wave", "bx")), (case["name"], view, s_on, s_nowave)
    assert (bx > 0) == (route == "bx"), (case["name"], view, bx)
    if route == "bx":
        assert L.sf_conv_wgrad_bx_splits(by) > 0
    return s_on


def _run_wgrad(case, view, tune, reference):
    """Packed gradient and finish_into on a seeded destination, for one case and view."""
    import sfhip
    dev = _dev()
    t, ref, mag = reference
    xv, zv = WGRAD_VIEWS[view]
    _apply_tune(tune, case)
    xa = R.view(dev, t["x"], xv[0], case["cin"] + xv[1], NAN)
    dza = R.view(dev, t["dz"], zv[0], case["cout"] + zv[1], NAN)
    cin_pad = sfhip._pad16(case["cin"])
    assert case["cin"] <= cin_pad
    _wgrad_route(tune, _wgrad_desc(sfhip, xa, dza, case, cin_pad), case, view)
    xs, zs = _snapshot(xa), _snapshot(dza)
    n, to, ho, wo, _ = t["dz"].shape
    K = n * to * ho * wo
    tag = "wgrad/%s/%s" % (case["name"], view)
    dwp = sfhip.conv_wgrad(xa, dza, case["cout"], case["k"], case["s"], case["p"])
    torch.cuda.synchronize()
    assert tuple(dwp.shape) == (case["cout"], case["k"][0] * case["k"][1] * case["k"][2], cin_pad)
    assert bool((dwp[:, :, case["cin"]:] == 0).all()), tag + ": packed padding channels must be exactly zero"
    _check(tag + "/packed", sfhip.unpack_conv_weight_grad(dwp, t["w"].shape).cpu(), ref, mag, K)
    # finish_into: accumulate onto a seeded gradient that sits between sentinels in its allocation
    numel = t["w"].numel()
    alloc = torch.full((numel + 128,), R.SENTINEL)
    alloc[64:64 + numel] = t["base_dw"].reshape(-1)
    alloc = alloc.to(dev)
    dst = alloc[64:64 + numel].view(t["w"].shape)
    assert sfhip.conv_wgrad(xa, dza, case["cout"], case["k"], case["s"], case["p"],
                            finish_into=(dst, case["cin"], 0)) is None
    torch.cuda.synchronize()
    edge = torch.cat([alloc[:64], alloc[64 + numel:]]).cpu()
    assert torch.equal(edge.view(torch.int32), torch.full_like(edge, R.SENTINEL).view(torch.int32)), \
        tag + ": a store outside the gradient"
    _check(tag + "/finish", dst.cpu(), ref + t["base_dw"].double(), mag + t["base_dw"].double().abs(), K)
    assert _unchanged(xa, xs) and _unchanged(dza, zs), tag + ": an input changed"
    return xa, dza, dwp


@pytest.mark.parametrize("case,view", WGRAD_RUNS, ids=["%s-%s" % (c["name"], v) for c, v in WGRAD_RUNS])
def test_conv_wgrad_views(case, view, tune):
    import sfhip
    xa, dza, dwp = _run_wgrad(case, view, tune, _wgrad_reference(case))
    if case["name"] in ("rows_s3_8_8_k1120", "wave_s3_64_64"):  # the fixed summation order
        again = sfhip.conv_wgrad(xa, dza, case["cout"], case["k"], case["s"], case["p"])
        torch.cuda.synchronize()
        assert torch.equal(dwp, again), "a second identical call must be bit-identical"


# conv_bx.hip's weight gradient (bxw_plan: Cin % 8 == 0 = cin_pad, Cout >= 128 and % 8 == 0, taps * Cin >= 512,
# M >= 2048, then its win / lose rule against conv_wgrad_wave at the DEFAULT level).  A sweep of the exported planner
# over Cin 64 .. 1024, Cout 128 .. 1024, the four window shapes and M in steps of 256 puts the cheapest accepted shapes
# at ~3.4 G products: 384 -> 128 channels under a 3x3x3 window from M = 2560 on.
WGRAD_BX_CASE = _case("bx_k27_384_128", 384, 128, (3, 3, 3), ONE, (1, 1, 1), (1, 4, 25, 26), route="bx")


@pytest.mark.parametrize("view", list(WGRAD_VIEWS))
def test_conv_wgrad_bx_views(view, tune):
    """The bf16-piece weight gradient at its default level, on the smallest shape its planner accepts (above).  Its
    M >= 2048 floor puts K = M = 2600 above the 1200 of the other cases; a single dropped product, mag / K, is still
    six times the bound of 2608 roundings.  `dz_misaligned` is the run-time refusal of sf_conv_wgrad_bx (SF_EALIGN ->
    sf_conv_wgrad with conv_wgrad_wave's split count and the LDS-tiled kernel)."""
    _run_wgrad(WGRAD_BX_CASE, view, tune, _wgrad_reference(WGRAD_BX_CASE))


# ---------------------------------------------------------------------------------------------------- finish kernels
# sf_conv_wgrad_finish on a seeded partial [S, Cout, taps, cin_pad]; K = S.  Padding columns hold the sentinel: they
# must be dropped, not added to a neighbour.
def _fin(name, S, cout, taps, cin_pad, cin, fold_kw=0):
    return dict(name="%s_S%d" % (name, S), S=S, cout=cout, taps=taps, cin_pad=cin_pad, cin=cin, fold_kw=fold_kw)


FINISH_CASES = (
    # wgrad_finish_flat_kernel<64> (<= 65 536 elements, S <= 32): 4 split groups; S = 32 is one eight-deep trip, no tail
    [_fin("flat64", S, 16, 9, 32, 27) for S in (1, 5, 32)] +
    # wgrad_finish_flat_kernel<16> (S > 32): 16 split groups, eight-deep trips from S = 113 on — 33 and 100 are tails
    # only, 150 is one trip and a tail in every group
    [_fin("flat16", S, 16, 9, 32, 27) for S in (33, 100, 150)] +
    # wgrad_finish_kernel: 19 * 27 * 128 = 65 664 elements; Cin = 100 = a full 64-channel tile and one of 36 columns;
    # S = 19 is one trip of the 16-stride loop and a tail in groups 0 .. 2
    [_fin("tiled", S, 19, 27, 128, 100) for S in (3, 19)] +
    # wgrad_finish_stem_kernel: packed channel = (kw, ci), 7 x 3 of 32 real
    [_fin("stem", 4, 8, 35, 32, 3, fold_kw=7)]
)
FINISH_RUNS = [(c, a) for c in FINISH_CASES for a in (0, 1)]


@pytest.mark.parametrize("case,accumulate", FINISH_RUNS,
                         ids=["%s-%s" % (c["name"], "acc" if a else "write") for c, a in FINISH_RUNS])
def test_wgrad_finish_kernels(case, accumulate):
    import sfhip
    dev = _dev()
    t = C.finish_inputs(case)
    ref, mag = C.finish_ref(t["part"], case["cin"], case["fold_kw"], t["base"] if accumulate else None)
    elems = case["cout"] * case["taps"] * case["cin_pad"]
    assert (elems > 65536) == case["name"].startswith("tiled")
    numel = t["base"].numel()
    alloc = torch.full((numel + 128,), R.SENTINEL)
    alloc[64:64 + numel] = t["base"] if accumulate else NAN
    alloc = alloc.to(dev)
    dst = alloc[64:64 + numel]
    part = t["part"].to(dev)
    snap = part.clone()
    sfhip._call("sf_conv_wgrad_finish", sfhip._ptr(part), case["S"], case["cout"], case["taps"], case["cin_pad"],
                case["cin"], case["fold_kw"], sfhip._ptr(dst), accumulate)
    torch.cuda.synchronize()
    tag = "finish/%s/%s" % (case["name"], "acc" if accumulate else "write")
    edge = torch.cat([alloc[:64], alloc[64 + numel:]]).cpu()
    assert torch.equal(edge.view(torch.int32), torch.full_like(edge, R.SENTINEL).view(torch.int32)), \
        tag + ": a store outside the destination"
    _check(tag, dst.cpu().view(ref.shape), ref, mag, case["S"])
    assert torch.equal(part, snap)


# ---------------------------------------------------------------------------------------------------- Python pre-sum
# sfhip.conv_wgrad(..., finish_into=...) sums the partials with a tree sum first when S > 128 and the packed weight has
# more than 65 536 elements.  Which plans can give that: the LDS-tiled and per-wavefront plans give S <= 768 / tiles and
# a weight that large has at least 6 tiles of 128 x 128 (S <= 128) unless Cin % 4 != 0 keeps conv_wgrad_wave out, and
# then S > 128 splits of >= 256 positions need > 80 MB of activations; conv_wgrad_rows' window form gives S <= 640 /
# blocks with at most 32 x 32 x taps elements per block (<= 36 864 at S > 128).  The ring over t (tring_plan) is the one
# plan whose split count does not shrink with the weight: S = N * ceil(H * W / 64) * nseg.  The smallest such shape is
# 32 -> 684 channels, 3x1x1, T = 2, H * W = 8200: 129 splits, 65 664 elements, 47 MB of activations.
PRESUM_CASE = _case("presum_t3_32_684", 32, 684, (3, 1, 1), ONE, (1, 0, 0), (1, 2, 82, 100), route="rows")


def test_conv_wgrad_python_presum(tune):
    """S = 129 > 128 and 684 * 3 * 32 = 65 664 > 65 536 partial elements: the tree sum in front of the finish kernel.
    K = M = 16 400 here (the split count needs the positions), so the bound is 16 408 roundings; the case is about the
    branch being taken and summing every split once."""
    import sfhip
    dev = _dev()
    case = PRESUM_CASE
    t, ref, mag = _wgrad_reference(case)
    xa = R.view(dev, t["x"], 4, case["cin"] + 12, NAN)
    dza = R.view(dev, t["dz"], 8, case["cout"] + 12, NAN)
    d = _wgrad_desc(sfhip, xa, dza, case, 32)
    S = tune.sf_conv_wgrad_splits(ctypes.byref(d))
    assert S > 128 and case["cout"] * 3 * 32 > 65536 and tune.sf_conv_wgrad_bx_ws_floats(ctypes.byref(d), 0, 0) == 0, S
    base = t["base_dw"]
    dst = base.clone().to(dev)
    sfhip.conv_wgrad(xa, dza, case["cout"], case["k"], case["s"], case["p"], finish_into=(dst, case["cin"], 0))
    torch.cuda.synchronize()
    n, to, ho, wo, _ = t["dz"].shape
    _check("wgrad/%s/presum" % case["name"], dst.cpu(), ref + base.double(), mag + base.double().abs(),
           n * to * ho * wo)
