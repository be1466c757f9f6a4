"""Op-level parity and owned memory of the attention family — sf_attn_fwd_ws, sfhip.attention_bwd (sf_attn_bwd_fused
and the two-kernel sf_attn_bwd) — on channel slices of wider buffers, against the float64 CPU reference of the same
fp32 inputs (tests/_attn_ref.py).  The dispatch picks a kernel by C, by C % 4, by every stride and pointer being
float4-addressable and by whether a workspace was passed; the tables below walk every branch of it, the fallback
kernels included (tools/isa_audit.py lists them), and name the kernel each run is meant for with the predicate that
sends it there.

Shapes.  B = 2 and two position counts: N = 35 = (1, 5, 7), one partial tile in every kernel, and N = 333 = (3, 3, 37),
ragged in every tiling in use (128-query tiles: two and one of 77; 64-key tiles: five and one of 13; 32-key tiles at
d = 128; 16-query wavefronts; the 128- and 64-key backward blocks).

Views.  q, k, v are slices of one qkv buffer, as the model builds them; x, out, dz, dq and the dk | dv pair are slices
of wider buffers (r4 = rounded up to a multiple of 4, so that `aligned` pitches stay float4-addressable when C % 4 != 0)
  aligned         qkv (coff 4, pitch r4(3C) + 12), x / dz (coff 4, pitch r4(C) + 8), out / dq (coff 8, pitch r4(C) + 12),
                  dk | dv (coff 4, pitch r4(2C) + 12)
  misaligned      qkv (coff 3, pitch 3C + 5), x / dz (coff 2, pitch C + 3), out / dq (coff 1, pitch C + 3),
                  dk | dv (coff 3, pitch 2C + 5)
  out_misaligned  aligned, but out (forward) resp. dk | dv (backward) as in `misaligned`
  shifted         the aligned layout in buffers that start one float into their allocation: pitches and offsets look
                  float4-addressable, the refusal happens on the pointer at run time
Inputs sit between NaN channels and must come back unchanged (whole buffer, compared as int32); outputs start as NaN
between sentinel channels that must come back bit for bit; o_save and lse_save are narrowed out of sentinel-padded
allocations whose padding is checked the same way.

Bounds, against the fp64 reference only.  5 <= C <= 64 (unit-scale inputs): those of test_attention_bx_gpu.py, which
states that the f32-MFMA kernels meet them too — o_save and z max error <= 5e-6 of the reference's max, o_save rms
<= 6e-7, gradients max <= 2e-5 and rms <= 1e-6.  C <= 4 and C > 64 (q, k scaled by 0.7): the max-norm 2e-4 of
test_backward_ops_gpu.py::test_attention_backward.  lse_save: 1e-3 absolute in log2 units (test_ops_gpu.py).  dvec is
held to the gradient bound of its family and the sum of the returned dvec (in float64, times nothing else) to the
same max-norm figure against dgamma.  Every measured figure is appended to attn_views_report.txt.

Measured on an MI355X (worst over the cases of a group): forward o max 1.6e-6 / rms 1.4e-7, z 7.7e-7 for 5 <= C <= 64
(f32-MFMA fallbacks and bf16 kernels alike), o 2.7e-6 at d = 128, lse 1.7e-5; fused backward families 5 / 6 gradients
4.3e-6 / 4.5e-6 max, 2.7e-7 / 3.5e-7 rms; two-kernel backward 7.0e-6 max, 5.3e-7 rms (C = 64); C <= 4 and C = 100
2.0e-6 max."""
import pytest
import torch

import _attn_ref as A
import _conv_ref as C
import _elementwise_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
B = 2
SHAPES = {35: (1, 5, 7), 333: (3, 3, 37)}
LSE_TOL = 1e-3
LOOSE = 2e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _report(name, err):
    """One line per measured figure in attn_views_report.txt, beside the other op-level reports."""
    from test_backward_ops_gpu import _report as report
    report(name, err, "attn_views_report.txt")


@pytest.fixture
def attn_knobs():
    """sf_attn_tune is process-wide: every test that forces sweep parts hands the planner back."""
    import sfhip
    L = sfhip.lib()
    yield L
    L.sf_attn_tune(0, 0)
    L.sf_attn_tune(1, 0)


def _r4(c):
    return (c + 3) // 4 * 4


def _layout(view, c):
    """name -> (coff, pitch) of every buffer of a run, and whether the buffers start one float into their allocation."""
    al = dict(qkv=(4, _r4(3 * c) + 12), x=(4, _r4(c) + 8), out=(8, _r4(c) + 12), dkv=(4, _r4(2 * c) + 12))
    mis = dict(qkv=(3, 3 * c + 5), x=(2, c + 3), out=(1, c + 3), dkv=(3, 2 * c + 5))
    if view == "misaligned":
        return mis, False
    if view == "out_misaligned":
        return dict(al, out=mis["out"], dkv=mis["dkv"]), False
    assert view in ("aligned", "shifted"), view
    return al, view == "shifted"


def _mk(dev, vals, spec, fill, shifted):
    """-> (Act, the allocation in front of which one more float is checked, or None)."""
    if shifted:
        return C.shifted_view(dev, vals, spec[0], spec[1], fill)
    return R.view(dev, vals, spec[0], spec[1], fill), None


def _front_ok(alloc, fill):
    if alloc is None:
        return True
    want = torch.tensor([fill], dtype=torch.float32)
    return torch.equal(alloc[:1].cpu().view(torch.int32), want.view(torch.int32))


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


PAD = 64


def _padded(dev, numel, shift=0):
    """A NaN tensor of `numel` floats narrowed out of an allocation that holds the sentinel around it; shift = 1 puts
    it one float off the 16-byte boundary."""
    alloc = torch.full((numel + 2 * PAD + shift,), R.SENTINEL, dtype=torch.float32)
    alloc[PAD + shift:PAD + shift + numel] = NAN
    alloc = alloc.to(dev)
    t = alloc.narrow(0, PAD + shift, numel)
    assert t.data_ptr() % 16 == 4 * shift
    return alloc, t


def _padding_ok(alloc, t):
    lo = (t.data_ptr() - alloc.data_ptr()) // 4
    edge = torch.cat([alloc[:lo], alloc[lo + t.numel():]]).cpu()
    return edge.numel() >= 2 * PAD and _same_bits(edge, torch.full_like(edge, R.SENTINEL))


def _float4_addressable(c, *acts):
    """The dispatch's own question (`vec4` in attn_fwd_impl / sf_attn_bwd_fused), asked of the views a run built — so
    that a case provably is the one its comment says: C % 4 == 0, every pitch and offset a multiple of 4, every
    buffer 16-byte aligned."""
    return c % 4 == 0 and all(a.cs % 4 == 0 and a.coff % 4 == 0 and a.buf.data_ptr() % 16 == 0 for a in acts)


_CACHE = {}


def _reference(c, n):
    """(inputs, fp64 reference) of a (C, N) pair: computed once, shared by every view and mode, never modified."""
    key = (c, n)
    if key not in _CACHE:
        t = A.attn_inputs("c%d_n%d" % (c, n), B, SHAPES[n], c)
        _CACHE[key] = (t, A.attn_ref(t))
    return _CACHE[key]


def _check(tag, what, got, ref, c, grad=False):
    """Finite, then the family's bound: (max, rms) for 5 <= C <= 64, the max-norm 2e-4 outside it."""
    assert bool(torch.isfinite(got).all()), "%s: non-finite %s inside the view" % (tag, what)
    mx, rms = A.errs(got, ref)
    _report("%s %s max" % (tag, what), mx)
    _report("%s %s rms" % (tag, what), rms)
    print("%-70s %-5s max %.3e rms %.3e" % (tag, what, mx, rms))
    if A.tight(c):
        max_tol, rms_tol = (2e-5, 1e-6) if grad else (5e-6, 6e-7 if what == "o" else None)
    else:
        max_tol, rms_tol = LOOSE, None
    assert mx <= max_tol, (tag, what, mx, max_tol)
    assert rms_tol is None or rms <= rms_tol, (tag, what, rms, rms_tol)


# ---------------------------------------------------------------------------------------------------- forward
def _forward(dev, c, n, view, affine, alpha, o_shift=0):
    """One sf_attn_fwd_ws call on the views of (c, n, view).  -> dict of the views, snapshots and saved tensors."""
    import sfhip
    t, _ = _reference(c, n)
    thw = SHAPES[n]
    lay, shifted = _layout(view, c)
    qkv, qalloc = _mk(dev, t["qkv"], lay["qkv"], NAN, shifted)
    x, xalloc = _mk(dev, t["x"], lay["x"], NAN, shifted)
    out, oalloc = _mk(dev, torch.full((B, thw[0] * alpha, thw[1], thw[2], c), NAN), lay["out"], R.SENTINEL, shifted)
    o_alloc, o_save = _padded(dev, B * n * c, o_shift)
    l_alloc, lse_save = _padded(dev, B * n)
    gamma = t["gamma"].to(dev)
    scale = t["scale"].to(dev) if affine else None
    bias = t["bias"].to(dev) if affine else None
    q, k, v = qkv.slice(0, c), qkv.slice(c, c), qkv.slice(2 * c, c)
    ws = torch.empty((sfhip.lib().sf_attn_fwd_ws_floats(B, n, c),), dtype=torch.float32, device=dev)
    assert ws.numel() > 0
    snaps = (qkv.buf.clone(), x.buf.clone())
    sfhip._call("sf_attn_fwd_ws", sfhip._slice_base(q), q.cs, sfhip._slice_base(k), k.cs, sfhip._slice_base(v), v.cs,
                sfhip._slice_base(x), x.cs, sfhip._ptr(gamma), sfhip._ptr(scale), sfhip._ptr(bias),
                sfhip.ACT_RELU if affine else sfhip.ACT_NONE, out.ptr(), out.cs, out.coff, B, thw[0], thw[1], thw[2],
                c, alpha, sfhip._ptr(o_save), sfhip._ptr(lse_save), sfhip._ptr(ws))
    torch.cuda.synchronize()
    return dict(qkv=qkv, q=q, k=k, v=v, x=x, out=out, gamma=gamma, o=o_save.view(B, n, c), lse=lse_save.view(B, n),
                o_alloc=o_alloc, l_alloc=l_alloc, allocs=(qalloc, xalloc, oalloc), snaps=snaps)


def _check_forward(tag, c, n, run, affine, alpha):
    t, ref = _reference(c, n)
    out = run["out"]
    qalloc, xalloc, oalloc = run["allocs"]
    assert R.outside_is(out) and _front_ok(oalloc, R.SENTINEL), tag + ": a store outside the output view"
    assert _padding_ok(run["o_alloc"], run["o"]), tag + ": a store outside o_save"
    assert _padding_ok(run["l_alloc"], run["lse"]), tag + ": a store outside lse_save"
    assert _same_bits(run["qkv"].buf, run["snaps"][0]) and _same_bits(run["x"].buf, run["snaps"][1]), \
        tag + ": an input changed"
    assert _front_ok(qalloc, NAN) and _front_ok(xalloc, NAN)
    _check(tag, "o", run["o"].cpu(), ref["o"], c)
    lse = run["lse"].cpu()
    assert bool(torch.isfinite(lse).all()), tag + ": non-finite lse"
    lerr = float((lse.double() - ref["lse"]).abs().max())
    _report(tag + " lse abs", lerr)
    assert lerr <= LSE_TOL, (tag, lerr)
    got = R.inside(out)
    zref = A.epilogue_ref(ref["y"], SHAPES[n], t["scale"] if affine else None, t["bias"] if affine else None, affine,
                          alpha)
    _check(tag, "z", got, zref, c)
    frames = got.contiguous().view(B, SHAPES[n][0], alpha, -1)
    for r in range(1, alpha):  # the alpha copies of a row are the same bits
        assert _same_bits(frames[:, :, r].contiguous(), frames[:, :, 0].contiguous()), tag + ": T-upsample copies differ"


# (C, view, o_save shift) -> the kernel the run is meant for.  attn_fwd_impl (attn_flash.hip):
#   vec4 = C % 4 == 0 && q_cs % 4 == 0 && k_cs % 4 == 0 && v_cs % 4 == 0 && x_cs % 4 == 0 && out_cs % 4 == 0 &&
#          out_coff % 4 == 0 && sf_aligned16(q) && sf_aligned16(k) && sf_aligned16(v) && sf_aligned16(x) &&
#          sf_aligned16(out)
# `misaligned` fails it on every pitch, `out_misaligned` on out_cs / out_coff alone, `shifted` on the pointers alone.
FWD_CASES = [
    # sf_attn_lane_try (attn_lane.hip): "if (!vec4 || a.C != 4) return 1" (1 = refused) — taken: attn_lane_kernel
    (4, "aligned", 0, "lane"),
    # refused by !vec4 -> attn_small.hip "if (C <= 4) return launch<4>(a, vec4, stream)": attn_small_kernel<4, 1>
    (4, "misaligned", 0, "small4_scalar"),
    (4, "shifted", 0, "small4_scalar"),
    # refused by "(a.o_save && !sf_aligned16(a.o_save))" with vec4 true: attn_small_kernel<4, 4>, scalar o_save stores
    (4, "aligned", 1, "small4_vec4"),
    # "if (C > 4 && C <= 8 && C % 4 == 0 && vec4 && ws)": attn_fwd_bxp_kernel, packed bf16 planes
    (8, "aligned", 0, "bxp"),
    # !vec4 -> "if (C <= 16) return sf_attn_small_dispatch(..)" -> "if (C <= 8) return launch<8>(a, vec4, stream)" with
    # vec4 false: attn_small_kernel<8, 1>
    (8, "misaligned", 0, "small8_scalar"),
    (8, "shifted", 0, "small8_scalar"),
    # "return launch<16>(a, vec4, stream)": attn_small_kernel<16, 4> / <16, 1>; C = 12 leaves channels 12 .. 15 padded
    (12, "aligned", 0, "small16_vec4"),
    (12, "misaligned", 0, "small16_scalar"),
    (16, "aligned", 0, "small16_vec4"),
    (16, "misaligned", 0, "small16_scalar"),
    # "if (C <= 32) return launch<32>(a, vec4, s)" -> "if (vec4 && a.bx_planes)": attn_fwd_bx_kernel<32>
    (32, "aligned", 0, "bx32"),
    # !vec4 -> "else hipLaunchKernelGGL((attn_fwd_kernel<CP, 1, STALE>), ..)": attn_fwd_kernel<32, 1, true>
    (32, "misaligned", 0, "fwd32_scalar"),
    (32, "out_misaligned", 0, "fwd32_scalar"),
    (32, "shifted", 0, "fwd32_scalar"),
    # "if (C <= 64) return launch<64>(a, vec4, s)" -> "if (vec4 && a.bx_planes)" (bx_planes: cp == 64 && C > 32):
    # attn_fwd_bx2_kernel, 48 = a full and a half 32-channel block
    (48, "aligned", 0, "bx2"),
    (48, "misaligned", 0, "fwd64_scalar"),    # attn_fwd_kernel<64, 1, true>
    (48, "out_misaligned", 0, "fwd64_scalar"),
    (48, "shifted", 0, "fwd64_scalar"),
    # aligned pitches, but "C % 4 == 0" fails: attn_fwd_kernel<32, 1>, <64, 1>, <128, 1> with a per-channel tail
    # (102 = three 32-channel tiles and 6 channels: the last float4 of a row is half real)
    (30, "aligned", 0, "fwd32_scalar"),
    (50, "aligned", 0, "fwd64_scalar"),
    (102, "aligned", 0, "fwd128_scalar"),
    # 100 % 4 == 0, so aligned views keep float4: attn_fwd_kernel<128, 4, false> with C < CP, "if (c0 >= C) continue"
    (100, "aligned", 0, "fwd128_vec4"),
    # "return launch<128>(a, vec4, s)": attn_fwd_kernel<128, 4, false> / <128, 1, false>, 32-key tiles
    (128, "aligned", 0, "fwd128_vec4"),
    (128, "misaligned", 0, "fwd128_scalar"),
]
# every N with scale / bias / ReLU and alpha = 2; N = 35 also bare (no affine, alpha = 1: the form the tape records)
FWD_RUNS = [(c, v, s, kern, n, mode) for c, v, s, kern in FWD_CASES for n, mode in ((35, "affine"), (35, "bare"),
                                                                                    (333, "affine"))]


def _fwd_id(c, v, s, kern, n, mode):
    return "c%d-%s%s-n%d-%s-%s" % (c, v, "-oshift" if s else "", n, mode, kern)


@pytest.mark.parametrize("c,view,o_shift,kern,n,mode", FWD_RUNS, ids=[_fwd_id(*r) for r in FWD_RUNS])
def test_attention_forward_views(c, view, o_shift, kern, n, mode):
    dev = _dev()
    affine, alpha = (True, 2) if mode == "affine" else (False, 1)
    run = _forward(dev, c, n, view, affine, alpha, o_shift)
    assert _float4_addressable(c, run["qkv"], run["x"], run["out"]) == (view == "aligned" and c % 4 == 0)
    assert kern.endswith("scalar") == (view != "aligned" or c % 4 != 0)
    if view == "shifted":  # only the pointer says no
        assert all(a.cs % 4 == 0 and a.coff % 4 == 0 for a in (run["qkv"], run["x"], run["out"]))
    assert (run["o"].data_ptr() % 16 != 0) == bool(o_shift)
    _check_forward("fwd/%s/c%d/n%d/%s%s/%s" % (kern, c, n, view, "+oshift" if o_shift else "", mode), c, n, run,
                   affine, alpha)


# sf_attn_tune(1, 3) at N = 333: three key parts ("if (p.zs > 1)" in attn_fwd_finish parks the unnormalised (O^T, m, l)
# of each part) and attn_fwd_merge_kernel with cp = 32 / 64 / 128 — for C = 30, 50, 100 its "if (c0 >= C) return" and
# the per-channel "(c0 + e) < C" tail (102: inside a float4); parts of 2 + 2 + 2 64-key tiles resp. 4 + 4 + 3 32-key
# tiles at d = 128.  C = 100 on aligned views is the float4 kernel under the same merge.
FWD_FORCED = [(30, "aligned", "fwd32_scalar"), (50, "aligned", "fwd64_scalar"), (100, "aligned", "fwd128_vec4"),
              (102, "aligned", "fwd128_scalar"), (32, "misaligned", "fwd32_scalar"),
              (128, "misaligned", "fwd128_scalar")]


@pytest.mark.parametrize("c,view,kern", FWD_FORCED, ids=["c%d-%s-%s" % r for r in FWD_FORCED])
def test_attention_forward_views_forced_parts(c, view, kern, attn_knobs):
    dev = _dev()
    assert attn_knobs.sf_attn_tune(1, 3) == 0
    run = _forward(dev, c, 333, view, True, 2)
    assert _float4_addressable(c, run["qkv"], run["x"], run["out"]) == kern.endswith("vec4")
    _check_forward("fwd/%s+merge/c%d/n333/%s/z3" % (kern, c, view), c, 333, run, True, 2)


# ---------------------------------------------------------------------------------------------------- backward
def _backward(dev, c, n, view, workspace, tag):
    """Forward of the same case (bare, as the tape records it), then sfhip.attention_bwd on its o and lse."""
    import sfhip
    t, ref = _reference(c, n)
    thw = SHAPES[n]
    lay, shifted = _layout(view, c)
    fview = "aligned" if view == "out_misaligned" else view
    run = _forward(dev, c, n, fview, False, 1)
    dz, zalloc = _mk(dev, t["dz"], lay["x"], NAN, shifted)
    dq, dqalloc = _mk(dev, torch.full((B,) + thw + (c,), NAN), _layout(fview, c)[0]["out"], R.SENTINEL, shifted)
    dkv, dkvalloc = _mk(dev, torch.full((B,) + thw + (2 * c,), NAN), lay["dkv"], R.SENTINEL, shifted)
    dk, dv = dkv.slice(0, c), dkv.slice(c, c)
    snaps = (run["qkv"].buf.clone(), dz.buf.clone(), run["o_alloc"].clone(), run["l_alloc"].clone())
    dvec = sfhip.attention_bwd(run["q"], run["k"], run["v"], dz, run["o"], run["lse"], run["gamma"], dq, dk, dv,
                               workspace=workspace)
    torch.cuda.synchronize()
    assert R.outside_is(dq) and _front_ok(dqalloc, R.SENTINEL), tag + ": a store outside the dq view"
    assert R.outside_is(dkv) and _front_ok(dkvalloc, R.SENTINEL), tag + ": a store outside the dk | dv views"
    assert _same_bits(run["qkv"].buf, snaps[0]) and _same_bits(dz.buf, snaps[1]) and _front_ok(zalloc, NAN) and \
        _same_bits(run["o_alloc"], snaps[2]) and _same_bits(run["l_alloc"], snaps[3]), tag + ": an input changed"
    got = R.inside(dkv)
    for what, g in (("dq", R.inside(dq)), ("dk", got[..., :c]), ("dv", got[..., c:])):
        _check(tag, what, g.reshape(B, n, c), ref[what], c, grad=True)
    _check(tag, "dvec", dvec.cpu().view(B, n), ref["dvec"], c, grad=True)
    dg = float(dvec.cpu().double().sum())
    gerr = abs(dg - float(ref["dgamma"])) / abs(float(ref["dgamma"]))
    _report(tag + " dgamma rel", gerr)
    assert gerr <= (2e-5 if A.tight(c) else LOOSE), (tag, dg, float(ref["dgamma"]))
    return run, dz, dq, dkv


# C -> sf_attn_bwd_variant on 16-byte aligned views (10 * family + wavefronts per workgroup), and what a view that is
# not float4-addressable falls to.  sf_attn_bwd_fused (attn_bwd.hip):
#    4  14  "if (C <= 16) return sf_attn_small_fused_dispatch(..)" -> "if (C <= 4)": attn_small_fused44_kernel<4>,
#           scalar loads whatever the view
#    7  14  "else if (C <= 8)": attn_small_fused44_kernel<8> with a per-channel tail
#    8  24  "if (C > 4 && C <= 8 && C % 4 == 0 && (q_cs % 4 == 0) && .. && sf_aligned16(dv))": attn_bwd_bxp_kernel<4>;
#           any view that fails it -> family 1, attn_small_fused44_kernel<8>
#   12  14  "else": attn_small_fused_kernel<16>, channels 12 .. 15 padded
#   28  34  "if (C <= 32) { const bool vec4 = (C % 4 == 0) && (q_cs % 4 == 0) && .. && sf_aligned16(dv); if (vec4)":
#   32  34  attn_bwd_bx_kernel<4>; else "return launch_fused<32, FUSED_KEYS_32 / 32>(a, ws, ..)" = family 5,
#           attn_bwd_fused_kernel<32, 4> + attn_dq_reduce_tiled_kernel
#   48  44  the same vec4 test, "if (vec4) return launch_fused_bx2(..)"; else "return launch_fused<64, 4>(a, ws, ..)"
#           = family 6, attn_bwd_fused_kernel<64, 4>
#   30  54  C % 4 != 0: family 5 on any view (C < CP = 32 in the dQ reduction)
#   50  64  C % 4 != 0: family 6 on any view (C < CP = 64)
#  100  74  "if (C > 64)": attn_bwd_dq_kernel<128> + attn_bwd_dkv_kernel<128> through the fused entry
FUSED_VARIANT = {4: 14, 7: 14, 8: 24, 12: 14, 28: 34, 32: 34, 48: 44, 30: 54, 50: 64, 100: 74}
FUSED_FALLBACK = {8: "family1", 28: "family5", 32: "family5", 48: "family6"}
FUSED_RUNS = ([(c, v) for c in FUSED_VARIANT for v in ("aligned", "misaligned")] +
              # the vec4 test names dk / dv (dk_cs, dv_cs, sf_aligned16(dk), sf_aligned16(dv)) and every pointer: these
              # must leave the bf16 kernels for families 1, 5 and 6 as well
              [(c, v) for c in (8, 32, 48) for v in ("out_misaligned", "shifted")])
FUSED_RUNS = [(c, v, n) for c, v in FUSED_RUNS for n in SHAPES]


def _family(c, view):
    return "family%d" % (FUSED_VARIANT[c] // 10) if view == "aligned" else FUSED_FALLBACK.get(
        c, "family%d" % (FUSED_VARIANT[c] // 10))


@pytest.mark.parametrize("c,view,n", FUSED_RUNS, ids=["c%d-%s-n%d" % r for r in FUSED_RUNS])
def test_attention_backward_fused_views(c, view, n):
    import sfhip
    dev = _dev()
    L = sfhip.lib()
    assert L.sf_attn_bwd_fused_ws_floats(B, n, c) > 0
    if view == "aligned":
        assert L.sf_attn_bwd_variant(B, n, c) == FUSED_VARIANT[c]
    run, dz, dq, dkv = _backward(dev, c, n, view, True, "bwd/%s/c%d/n%d/%s" % (_family(c, view), c, n, view))
    # (dq is not part of the test: attn_dq_reduce_tiled_kernel stores it scalar whatever the view)
    assert _float4_addressable(c, run["qkv"], dz, dkv) == (view == "aligned" and c % 4 == 0)
    if view == "out_misaligned":
        assert _float4_addressable(c, run["qkv"], dz, dq) and not _float4_addressable(c, dkv)


# workspace=False: sf_attn_bwd, "if (C <= 16) return sf_attn_small_bwd_dispatch(..)" -> attn_small_dq_kernel /
# attn_small_dkv_kernel<4 | 8 | 16>; "if (C <= 32) return launch<32>(a, which, s); if (C <= 64) return launch<64>(..);
# return launch<128>(..)" -> attn_bwd_dq_kernel / attn_bwd_dkv_kernel<32 | 64 | 128>.  Scalar loads and stores on any
# view; 30 and 100 leave padded channels in the 32- and 128-channel tiles.
TWO_KERNEL = {4: "small4", 8: "small8", 16: "small16", 30: "dq_dkv32", 32: "dq_dkv32", 64: "dq_dkv64", 100: "dq_dkv128"}
TWO_RUNS = [(c, v, n) for c in TWO_KERNEL for v in ("aligned", "misaligned") for n in SHAPES]


@pytest.mark.parametrize("c,view,n", TWO_RUNS, ids=["c%d-%s-n%d" % r for r in TWO_RUNS])
def test_attention_backward_two_kernel_views(c, view, n):
    dev = _dev()
    _backward(dev, c, n, view, False, "bwd2/%s/c%d/n%d/%s" % (TWO_KERNEL[c], c, n, view))


# sf_attn_tune(1, 3) at N = 333: three query parts.  "if (p.zs > 1)" at the end of attn_bwd_fused_kernel parks dK / dV
# partials [B][zs][N][CP] that attn_dq_reduce_kernel sums with "if (c + e < C)" (C < CP for 30, 50 and 48), dQ goes
# through attn_dq_reduce_tiled_kernel; parts of 2 + 2 + 2 64-query tiles (CP = 32) resp. 4 + 4 + 3 32-query tiles
# (CP = 64).  C = 100 is beyond the issue's list: the d = 128 two-kernel form with parts ("a.dqp = ws; .."), the one
# caller of attn_dq_reduce_kernel for dQ with C < CP = 128.
BWD_FORCED = [(30, "aligned", "family5"), (50, "aligned", "family6"), (32, "misaligned", "family5"),
              (48, "misaligned", "family6"), (100, "aligned", "family7")]


@pytest.mark.parametrize("c,view,fam", BWD_FORCED, ids=["c%d-%s-%s" % r for r in BWD_FORCED])
def test_attention_backward_fused_views_forced_parts(c, view, fam, attn_knobs):
    dev = _dev()
    assert attn_knobs.sf_attn_tune(1, 3) == 0
    _backward(dev, c, 333, view, True, "bwd/%s+parts/c%d/n333/%s/z3" % (fam, c, view))
