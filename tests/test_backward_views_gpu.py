"""Op-level parity of the kernels of csrc/backward.hip — BN backward reduce and apply, max-pool backward, the ECA
backward trio, the generic depthwise backward, rowdot / axpy / bcast_add / act_bwd / gather_add — against float64
closed-form references of the same fp32 inputs (tests/_backward_ref.py), on channel-slice views, at the smallest shapes
that reach every branch of the launchers.  Every case declares the route it is meant to reach;
test_backward_ref_cpu.py checks the tables below against the restated launch predicates without a GPU.

Views: inputs are channel slices of wider buffers whose other channels hold NaN; outputs are slices between SENTINEL
channels that must come back bit for bit; a view a kernel overwrites starts as NaN, one it accumulates into starts
from a random base; inputs must be unchanged afterwards.  Kinds: dense, a4 / a8 (coff 4 / 8 of pitch C + 12: float4
addressable), m3 (coff 3 of pitch C + 12) and mp (coff 4 of pitch C + 5): the last two force the scalar kernels.

Bounds.  Elementwise outputs: |got - ref| <= k * 2^-24 * mag, mag = sum of |terms| added to make the element, k = the
roundings the kernel makes on the longest path to an element, + 3:
  BN dz     9 + (rep - 1): xhat 2, xhat*dgamma 1, *inv_m 1 and inv_m's own rounding 1, the two subtractions 2,
            gamma*invstd 1, the final product 1; rep - 1 additions make g                                  -> 12 + (rep - 1)
  BN dres   accumulated: rep - 1 additions in g + 1 into the base -> rep + 3; first writer, rep = 1: exact
  max pool  accumulated: W - 1 additions of the W = prod ceil(k / s) windows over an element + 1 into the base -> W + 3;
            first writer: W + 2; windows that do not overlap: exact
  ECA dx    product, sum with dpool, sum into dx: 3                                                          -> 6
  dw dgrad  n taps: each term is rounded once as a product and at most n times by the running sum and the add into
            dx                                                                                               -> n + 4
  axpy / bcast_add 2 -> 5; act_bwd / gather_add accumulated 1 -> 4, overwriting: exact
  ECA gate  a = w (*) pooled makes 5 roundings relative to amag = sum |w p|, which move the sigmoid by g (1 - g) each;
            expf, 1 + e and the division at most 4 relative to g: mag = g (1 - g) amag + g, 5 -> 8
  ECA dpool da = dg g (1 - g) inherits the gate's error through |1 - 2 g| (5 of its mag) and makes 3 of its own; the
            three products, two sums and the scale make 5 more: mag = scale * sum |w| (|dg| |1 - 2g| mag_gate + |da|),
            10 -> 13
fp32 reductions (dbeta, dgamma, tmax_dot, rowdot, depthwise dw, ECA dw3): (L + 8) * 2^-24 * sum |terms|, L = the
longest fp32 chain of the kernel's own order (rows one thread walks + the LDS row-lane sum, from the restated
geometry; combined in fp64 after that) — the standard bound on recursive summation.  Every reduction is also held to
the 2e-4 max-norm of test_backward_ops_gpu.py.  The ratio measured / allowed of every case goes to
bwd_views_report.txt, beside the other op-level reports (test_backward_ops_gpu._report)."""
import ctypes
import zlib

import pytest
import torch

import _backward_ref as B

pytestmark = pytest.mark.gpu

TOL = 2e-4
NAN = float("nan")
NTHW = (3, 2, 5, 7)  # 210 rows


def vw(kind, C):
    """(coff, pitch) of a view kind."""
    return {"dense": (0, C), "a4": (4, C + 12), "a8": (8, C + 12), "m3": (3, C + 12), "mp": (4, C + 5)}[kind]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _report(name, ratio):
    from test_backward_ops_gpu import _report as report
    report(name, ratio, "bwd_views_report.txt")


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)


def _elementwise(name, got, ref, mag, k):
    r = B.rounds(got, ref, mag) / k
    _report(name, r)
    assert r <= 1.0, (name, r * k, k)


def _reduction(name, got, ref, mag, L):
    r = B.rounds(got, ref, mag) / (L + 8)
    _report(name, r)
    assert r <= 1.0, (name, r * (L + 8), L + 8)
    rel = float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    assert rel < TOL, (name, rel)


def _vec(dev, v, off=0):
    """v on the device, `off` floats into a longer NaN tensor (off = 1: at 4 mod 16 bytes)."""
    pad = torch.full((off,), NAN)
    t = torch.cat([pad, v, pad]).to(dev)[off:off + v.numel()]
    assert t.data_ptr() % 16 == (4 * off) % 16
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ================================================================================================ BN backward
def _bn(C, nthw, route, relu=0, mask_of=1, rep=1, S=1, acc=False, dres=None, over_z=False, **views):
    """relu: 0 none, 1 ReLU, 2 ReLU6, 3 byte mask (of ReLU, or of ReLU6 with mask_of=2).  views: dy / z / y / dz / dres_v
    -> kind (default dense).  dres: None, 'acc' or 'first'.  over_z: dz is written over z."""
    d = dict(C=C, nthw=nthw, route=route, relu=relu, mask_of=mask_of, rep=rep, S=S, acc=acc, dres=dres, over_z=over_z)
    d["views"] = {k: vw(views.pop(k if k != "dres" else "dres_v", "dense"), C) for k in ("dy", "z", "y", "dz", "dres")}
    assert not views, views
    return d


BN_REDUCE_CASES = {
    # 210 rows: one to six row blocks, the last arriver finishes
    "small_C27_relu": _bn(27, NTHW, "scalar/small-fused", relu=1, dy="m3", z="a4", y="mp"),
    "small_C64": _bn(64, NTHW, "vec4/small-fused"),
    "small_C64_relu6_aligned": _bn(64, NTHW, "vec4/small-fused", relu=2, dy="a4", z="a8", y="a4"),
    "small_C64_relu_dy_m3": _bn(64, NTHW, "scalar/small-fused", relu=1, dy="m3", z="a4", y="a4"),
    "small_C64_relu_z_mp": _bn(64, NTHW, "scalar/small-fused", relu=1, dy="a4", z="mp", y="a4"),
    "small_C64_relu_y_m3": _bn(64, NTHW, "scalar/small-fused", relu=1, dy="a4", z="a4", y="m3"),
    "small_C64_mask": _bn(64, NTHW, "vec4/small-fused", relu=3, dy="a4", z="a8"),
    "small_C64_mask6": _bn(64, NTHW, "vec4/small-fused", relu=3, mask_of=2),
    "small_C32_rep4": _bn(32, (2, 2, 5, 7), "vec4/small-fused", relu=1, rep=4, dy="a4", z="a4", y="a8"),
    "small_C7_rep4_relu6": _bn(7, (2, 2, 5, 7), "scalar/small-fused", relu=2, rep=4, dy="m3", z="dense", y="a4"),
    "small_C64_acc": _bn(64, NTHW, "vec4/small-fused", relu=1, acc=True, dy="a4", z="a4", y="a4"),
    # 1600 rows: 64 channels per channel group, 12 row blocks
    "few_C256_relu": _bn(256, (2, 2, 20, 20), "vec4/few-fused", relu=1, dy="a4", z="a8", y="a4"),
    "few_C300_mask": _bn(300, (2, 2, 20, 20), "vec4/few-fused", relu=3),
    "few_C256_acc": _bn(256, (2, 2, 20, 20), "vec4/few-fused", acc=True),
    "two_C256_z_m3": _bn(256, (2, 2, 20, 20), "scalar/two-launch", relu=2, dy="a4", z="m3", y="a4"),
    # 25 600 rows: P = 200, lanes 0..7 of the final kernel take one unrolled trip, the others none
    "two_C64_P200": _bn(64, (4, 4, 40, 40), "vec4/two-launch", dy="a4", z="a4"),
    "two_C64_P200_mask_acc": _bn(64, (4, 4, 40, 40), "vec4/two-launch", relu=3, acc=True),
    # 131 072 rows: P clamped to MAX_P
    "two_C64_P1024": _bn(64, (8, 4, 64, 64), "vec4/two-launch"),
    # Sub-BN splits: one row group per sample, chunks = max_p / N where the natural count is larger
    "split_S2_N4_C130": _bn(130, (4, 1, 46, 46), "scalar/two-launch", relu=1, S=2),
    "split_S4_N8_C130": _bn(130, (8, 1, 33, 33), "scalar/two-launch", S=4, dy="m3", z="mp"),
    "split_S2_N4_C16": _bn(16, (4, 2, 5, 7), "vec4/two-launch", relu=2, S=2, dy="a4", z="a8", y="a4"),
}
BN_REDUCE_GEOMETRY = {  # case -> (P, chunks) it is meant to run with
    "two_C64_P200": (200, 200), "two_C64_P200_mask_acc": (200, 200), "two_C64_P1024": (1024, 1024),
    "split_S2_N4_C130": (1024, 256), "split_S4_N8_C130": (1024, 128), "split_S2_N4_C16": (4, 1),
    "few_C256_relu": (12, 12), "few_C300_mask": (12, 12), "two_C256_z_m3": (200, 200),
}
BN_MASK_RAGGED = ["small_C64_mask", "small_C64_mask6", "few_C300_mask"]  # four-row trips AND a ragged tail

U4_256, U4_192 = (2, 2, 32, 32), (2, 4, 1, 683)  # 4096 rows x 64 quads = 262 144 exactly; 5464 rows x 48 quads
BN_APPLY_CASES = {
    "u4_C256": _bn(256, U4_256, "unroll4", over_z=True),
    "u4_C256_acc": _bn(256, U4_256, "unroll4", dres="acc", over_z=True, dy="a4", z="a8", dres_v="a4"),
    "u4_C256_first": _bn(256, U4_256, "unroll4", dres="first", dz="a4"),
    "u4_C256_mask": _bn(256, U4_256, "unroll4", relu=3, dz="a8", z="a4"),
    "u4_C256_mask_acc": _bn(256, U4_256, "unroll4", relu=3, dres="acc", dy="a4", z="a4", dz="a8", dres_v="a8"),
    "u4_C256_mask_first": _bn(256, U4_256, "unroll4", relu=3, mask_of=2, dres="first", over_z=True, z="a4"),
    "u4_C256_S2_acc": _bn(256, U4_256, "unroll4", S=2, dres="acc", over_z=True),
    "u4_C192": _bn(192, U4_192, "unroll4", over_z=True, z="a4"),
    "u4_C192_mask_acc": _bn(192, U4_192, "unroll4", relu=3, dres="acc", dz="a4", dres_v="a4"),
    "u4_C192_mask_first": _bn(192, U4_192, "unroll4", relu=3, dres="first", over_z=True),
    "v4_C256_rows4097_mask_acc": _bn(256, (1, 1, 17, 241), "vec4", relu=3, dres="acc", over_z=True),
    "v4_C192_rows5465": _bn(192, (1, 5, 1, 1093), "vec4", dz="a4"),
    "v4_C256_under": _bn(256, (2, 2, 31, 33), "vec4", dres="first", over_z=True),  # 261 888 quads
    "v4_C64_relu_acc": _bn(64, NTHW, "vec4", relu=1, dres="acc", dy="a4", z="a8", y="a4", dz="a4", dres_v="a8"),
    "v4_C64_relu6_first": _bn(64, NTHW, "vec4", relu=2, dres="first", over_z=True, z="a4", y="a8", dres_v="a4"),
    "v4_C32_rep4": _bn(32, (2, 2, 5, 7), "vec4", relu=1, rep=4, dy="a4", z="a4", y="a8", dz="a4"),
    "v4_C16_S2": _bn(16, (4, 2, 5, 7), "vec4", relu=2, S=2, dres="acc", over_z=True, z="a4", y="a4", dres_v="a4"),
    # the float4 predicate is a conjunction: each view alone takes it away
    "sc_C64_dy_m3": _bn(64, NTHW, "scalar", relu=1, dres="acc", dy="m3", z="a4", y="a4", dz="a4", dres_v="a4"),
    "sc_C64_z_mp": _bn(64, NTHW, "scalar", relu=1, dres="acc", dy="a4", z="mp", y="a4", dz="a4", dres_v="a4"),
    "sc_C64_y_m3": _bn(64, NTHW, "scalar", relu=1, dres="acc", dy="a4", z="a4", y="m3", dz="a4", dres_v="a4"),
    "sc_C64_dz_mp": _bn(64, NTHW, "scalar", relu=1, dres="acc", dy="a4", z="a4", y="a4", dz="mp", dres_v="a4"),
    "sc_C64_dres_m3": _bn(64, NTHW, "scalar", relu=1, dres="first", dy="a4", z="a4", y="a4", dz="a4", dres_v="m3"),
    "sc_C64_over_z_m3": _bn(64, NTHW, "scalar", dres="acc", over_z=True, z="m3", dres_v="a4"),
    "sc_C27_relu6_first": _bn(27, NTHW, "scalar", relu=2, dres="first", over_z=True, z="a4", y="mp"),
    "sc_C7_S2_rep4": _bn(7, (4, 2, 5, 7), "scalar", relu=1, S=2, rep=4, dz="a4"),
}
BN_BIT_PAIRS = ["u4_C256_acc", "u4_C256_mask_acc", "u4_C192_mask_first"]  # unroll4 == plain vec4, bit for bit


class _BnData(object):
    """The fp32 inputs of one BN backward case and their fp64 consequences, made once on the CPU."""

    def __init__(self, name, case):
        g = _gen(name)
        C, (N, T, H, W), S, rep, relu = case["C"], case["nthw"], case["S"], case["rep"], case["relu"]
        act = case["mask_of"] if relu == 3 else relu
        self.z = torch.randn(N, T, H, W, C, generator=g) * 1.5 + 0.3
        zd = self.z.double()
        self.mean = torch.stack([zd[s::S].mean((0, 1, 2, 3)) for s in range(S)]).reshape(-1).float()
        var = torch.stack([zd[s::S].var((0, 1, 2, 3), unbiased=False) for s in range(S)]).reshape(-1)
        self.invstd = torch.rsqrt(var + 1e-5).float()
        self.gamma = torch.rand(S * C, generator=g) + (2.5 if act == 2 else 0.5)  # ReLU6: saturate some
        beta = torch.randn(S * C, generator=g) * 0.1 + (2.0 if act == 2 else 0.0)
        ps = lambda v: B._per_sample(v, N, S)
        pre = (ps(self.gamma) * (zd - ps(self.mean)) * ps(self.invstd) + ps(beta)).float()
        self.dy = torch.randn(N, T * rep, H, W, C, generator=g)
        self.y = self.mask = None
        if act:
            y0 = pre.clamp(0.0, 6.0) if act == 2 else pre.clamp_min(0.0)
            # only copy 0 of every `rep` frames is the layer's activation; the others pass where it blocks
            copies = [y0] + [1.0 - y0.sign()] * (rep - 1)
            self.y = torch.stack(copies, 2).reshape(N, T * rep, H, W, C).contiguous()
        ok = B.act_pass(self.y, act, rep)
        if relu == 3:
            from _elementwise_ref import mask_ref
            self.mask = mask_ref(pre.double(), 6 if act == 2 else 1)
            assert torch.equal(mask_ref(torch.where(ok, 1.0, -1.0).double(), 1), self.mask)
            passed = float(ok.float().mean())
            assert 0.05 < passed < 0.98, passed
        self.g, self.gmag = B.bn_g_ref(self.dy, ok, rep)
        self.sums = B.bn_sums_ref(self.g, self.gmag, self.z, self.mean, self.invstd, S)


_bn_cache = {}


def _bn_data(name, case):
    key = (case["C"], case["nthw"], case["S"], case["rep"], case["relu"], case["mask_of"])
    if key not in _bn_cache:
        _bn_cache[key] = _BnData("bn%r" % (key,), case)
    return _bn_cache[key]


def _bn_head(dev, d, case, z_fill=NAN):
    """The device views and the leading arguments every sf_bn_bwd_* entry point shares."""
    C, (N, T, H, W), v = case["C"], case["nthw"], case["views"]
    dya = B.view(dev, d.dy, v["dy"][0], v["dy"][1], NAN)
    za = B.view(dev, d.z, v["z"][0], v["z"][1], z_fill)
    ya = mask = None
    if case["relu"] == 3:
        mask = d.mask.to(dev)
        ytriple = (_p(mask), C // 4, 0)
    elif case["relu"]:
        ya = B.view(dev, d.y, v["y"][0], v["y"][1], NAN)
        ytriple = (ya.ptr(), ya.cs, ya.coff)
    else:
        ytriple = (None, 0, 0)
    head = (dya.ptr(), dya.cs, dya.coff) + ytriple + (za.ptr(), za.cs, za.coff, N, T, H, W, C)
    head += ((case["S"],) if case["S"] > 1 else ()) + (case["rep"], case["relu"])
    return head, dya, za, ya, mask


def _bn_reduce_run(dev, d, case, views_out=None):
    import sfhip
    C, S = case["C"], case["S"]
    head, dya, za, ya, mask = _bn_head(dev, d, case)
    mean, invstd = d.mean.to(dev), d.invstd.to(dev)
    out = torch.full((2, S * C), NAN, device=dev)
    ws = torch.empty((sfhip.lib().sf_bn_bwd_ws_floats(C),), dtype=torch.float32, device=dev)
    tail = (_p(mean), _p(invstd), _p(out[0]), _p(out[1]), _p(ws))
    sink = None
    if case["acc"]:
        sink = torch.randn(2, C, generator=_gen("sink")).to(dev)
        sfhip._call("sf_bn_bwd_reduce_acc", *head, *tail, _p(sink[0]), _p(sink[1]))
    else:
        sfhip._call("sf_bn_bwd_reduce_split" if S > 1 else "sf_bn_bwd_reduce", *head, *tail)
    torch.cuda.synchronize()
    if views_out is not None:
        views_out.extend([(dya, d.dy), (za, d.z)] + ([(ya, d.y)] if ya is not None else []))
    return out.cpu(), (sink.cpu() if sink is not None else None)


@pytest.mark.parametrize("name", list(BN_REDUCE_CASES))
def test_bn_bwd_reduce(name):
    dev = _dev()
    case = BN_REDUCE_CASES[name]
    d = _bn_data(name, case)
    route = B.bn_reduce_route(case["C"], case["nthw"], case["views"]["dy"], case["views"]["z"], case["views"]["y"],
                              case["rep"], case["relu"], case["S"])
    assert route["route"] == case["route"]
    views = []
    out, sink = _bn_reduce_run(dev, d, case, views)
    again, sink2 = _bn_reduce_run(dev, d, case)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "two runs differ"
    dbeta, dgamma, mag_b, mag_g = d.sums
    _reduction("bn_reduce/%s dbeta" % name, out[0], dbeta, mag_b, route["L"])
    _reduction("bn_reduce/%s dgamma" % name, out[1], dgamma, mag_g, route["L"])
    if case["acc"]:  # the sums are also accumulated into the parameter gradients: one more rounding
        base = torch.randn(2, case["C"], generator=_gen("sink"))
        assert torch.equal(sink, sink2)
        for i, (ref, mag) in enumerate(((dbeta, mag_b), (dgamma, mag_g))):
            _reduction("bn_reduce/%s sink%d" % (name, i), sink[i], ref + base[i].double(), mag + base[i].double().abs(),
                       route["L"] + 1)
    for a, host in views:
        assert torch.equal(B.inside(a), host), "an input view changed"


def test_bn_bwd_reduce_refusals():
    """S > 1 with more samples than row blocks, and a byte mask on a view that is not float4-addressable: SF_EINVAL,
    nothing launched."""
    import sfhip
    dev = _dev()
    assert B.bn_reduce_route(4, (1026, 1, 1, 1), (0, 4), (0, 4), None, 1, 0, 2) == B.EINVAL
    assert B.bn_reduce_route(64, NTHW, vw("m3", 64), (0, 64), None, 1, 3, 1) == B.EINVAL
    L = sfhip.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    C = 4
    t = torch.zeros(1026, 1, 1, 1, C, device=dev)
    vec = torch.ones(2 * C, device=dev)
    out = torch.full((2, 2 * C), NAN, device=dev)
    ws = torch.empty((L.sf_bn_bwd_ws_floats(C),), device=dev)
    rc = L.sf_bn_bwd_reduce_split(_p(t), C, 0, None, 0, 0, _p(t), C, 0, 1026, 1, 1, 1, C, 2, 1, 0, _p(vec), _p(vec),
                                  _p(out[0]), _p(out[1]), _p(ws), stream)
    assert rc == sfhip.SF_EINVAL
    C = 64
    coff, pitch = vw("m3", C)
    dy = torch.zeros(NTHW + (pitch,), device=dev)
    z = torch.zeros(NTHW + (C,), device=dev)
    mask = torch.zeros(210 * C // 4, dtype=torch.uint8, device=dev)
    vec = torch.ones(C, device=dev)
    out2 = torch.full((2, C), NAN, device=dev)
    ws = torch.empty((L.sf_bn_bwd_ws_floats(C),), device=dev)
    rc = L.sf_bn_bwd_reduce(_p(dy), pitch, coff, _p(mask), C // 4, 0, _p(z), C, 0, *NTHW, C, 1, 3, _p(vec), _p(vec),
                            _p(out2[0]), _p(out2[1]), _p(ws), stream)
    assert rc == sfhip.SF_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(out2).all())


def _bn_apply_run(dev, name, case, params_off=0, tag=""):
    """sf_bn_bwd_apply* fed with the fp32-rounded reference sums: the dz bound is then a per-element one.  Checks the
    bounds and the memory around every view; returns (dz, dres) as they came back."""
    import sfhip
    d = _bn_data(name, case)
    C, (N, T, H, W), S, rep, v = case["C"], case["nthw"], case["S"], case["rep"], case["views"]
    head, dya, za, ya, mask = _bn_head(dev, d, case, B.SENTINEL if case["over_z"] else NAN)
    dbeta, dgamma = d.sums[0].float(), d.sums[1].float()
    vecs = [_vec(dev, t, params_off) for t in (d.mean, d.invstd, d.gamma, dbeta, dgamma)]
    if case["over_z"]:
        dza = za
    else:
        dza = B.view(dev, torch.full((N, T, H, W, C), NAN), v["dz"][0], v["dz"][1], B.SENTINEL)
    base = dra = None
    if case["dres"]:
        base = torch.randn(N, T, H, W, C, generator=_gen("dres" + name)) if case["dres"] == "acc" else None
        dra = B.view(dev, base if base is not None else torch.full((N, T, H, W, C), NAN), v["dres"][0], v["dres"][1],
                     B.SENTINEL)
    fn = "sf_bn_bwd_apply_split" if S > 1 else ("sf_bn_bwd_apply_first" if case["dres"] == "first" else "sf_bn_bwd_apply")
    assert not (S > 1 and case["dres"] == "first")
    sfhip._call(fn, *head, *[_p(t) for t in vecs], dza.ptr(), dza.cs, dza.coff,
                dra.ptr() if dra is not None else None, dra.cs if dra is not None else 0,
                dra.coff if dra is not None else 0)
    torch.cuda.synchronize()
    ref, mag = B.bn_dz_ref(d.g, d.gmag, d.z, d.mean, d.invstd, d.gamma, dbeta, dgamma, S)
    got = B.inside(dza)
    _elementwise("bn_apply/%s%s dz" % (name, tag), got, ref, mag, 12 + (rep - 1))
    assert B.outside_is(dza) or dza.cs == C
    got_res = None
    if dra is not None:
        got_res = B.inside(dra)
        rref, rmag = B.dres_ref(d.g, d.gmag, base)
        if base is None and rep == 1:
            assert torch.equal(got_res.double(), rref), "the first writer's dres is a selection of dy"
        else:
            _elementwise("bn_apply/%s%s dres" % (name, tag), got_res, rref, rmag, rep + 3)
        assert B.outside_is(dra) or dra.cs == C
    assert torch.equal(B.inside(dya), d.dy)
    if not case["over_z"]:
        assert torch.equal(B.inside(za), d.z)
    if ya is not None:
        assert torch.equal(B.inside(ya), d.y)
    if mask is not None:
        assert torch.equal(mask.cpu(), d.mask)
    return got, got_res


def _apply_route(case, params_aligned=True):
    v = case["views"]
    return B.bn_apply_route(case["C"], case["nthw"], v["dy"], v["z"], v["y"], v["z"] if case["over_z"] else v["dz"],
                            v["dres"] if case["dres"] else None, case["rep"], case["relu"], params_aligned)


@pytest.mark.parametrize("name", list(BN_APPLY_CASES))
def test_bn_bwd_apply(name):
    case = BN_APPLY_CASES[name]
    assert _apply_route(case) == case["route"]
    _bn_apply_run(_dev(), name, case)


@pytest.mark.parametrize("name", BN_BIT_PAIRS)
def test_bn_bwd_apply_unroll4_equals_vec4(name):
    """Parameter vectors at 4 mod 16 bytes keep the four-rows-per-thread branch out: the one-row float4 form then does
    the same arithmetic per element on the same data, so the two agree bit for bit."""
    case = BN_APPLY_CASES[name]
    assert _apply_route(case) == "unroll4" and _apply_route(case, params_aligned=False) == "vec4"
    dev = _dev()
    a = _bn_apply_run(dev, name, case, 0)
    b = _bn_apply_run(dev, name, case, 1, "/params+1")
    for u, w in zip(a, b):
        assert (u is None) == (w is None)
        if u is not None:
            assert torch.equal(u.view(torch.int32), w.view(torch.int32))


def test_bn_bwd_wrapper_dz_out_and_grad_sink():
    """sfhip.bn_bwd with dz_out (z must survive) and grad_sink (sums accumulated into non-zero .grad vectors)."""
    import sfhip
    dev = _dev()
    name = "wrapper"
    case = _bn(64, NTHW, "vec4", relu=1, dy="a4", z="a8", y="a4", dz="a4")
    d = _bn_data(name, case)
    head, dya, za, ya, _ = _bn_head(dev, d, case)
    N, T, H, W = NTHW
    dza = B.view(dev, torch.full((N, T, H, W, 64), NAN), 4, 76, B.SENTINEL)
    base = torch.randn(2, 64, generator=_gen("sink"))
    wgrad, bgrad = base[0].to(dev), base[1].to(dev)
    out, dgamma, dbeta = sfhip.bn_bwd(dya, ya, za, d.mean.to(dev), d.invstd.to(dev), d.gamma.to(dev), True, dz_out=dza,
                                      grad_sink=(wgrad, bgrad))
    torch.cuda.synchronize()
    assert out is dza
    L = B.bn_reduce_route(64, NTHW, (4, 76), (8, 76), (4, 76), 1, 1, 1)["L"]
    rb, rg, mb, mg = d.sums
    _reduction("bn_wrapper dbeta", dbeta.cpu(), rb, mb, L)
    _reduction("bn_wrapper dgamma", dgamma.cpu(), rg, mg, L)
    _reduction("bn_wrapper weight.grad", wgrad.cpu(), rg + base[0].double(), mg + base[0].double().abs(), L + 1)
    _reduction("bn_wrapper bias.grad", bgrad.cpu(), rb + base[1].double(), mb + base[1].double().abs(), L + 1)
    ref, mag = B.bn_dz_ref(d.g, d.gmag, d.z, d.mean, d.invstd, d.gamma, dbeta.cpu(), dgamma.cpu())
    _elementwise("bn_wrapper dz", B.inside(dza), ref, mag, 12)
    assert B.outside_is(dza) and torch.equal(B.inside(za), d.z)


# ================================================================================================ max-pool backward
POOL_NTHW = (2, 4, 13, 12)
POOL_WINDOWS = {"k133": ((1, 3, 3), (1, 2, 2), (0, 1, 1)), "k333": ((3, 3, 3), (1, 2, 2), (1, 1, 1)),
                "k222": ((2, 2, 2), (2, 2, 2), (0, 0, 0))}  # k222: windows do not overlap
POOL_VIEWS = {  # C, x, y, dy, dx kinds, route
    "C12_dense": (12, "dense", "dense", "dense", "dense", "vec4"),
    "C12_aligned": (12, "a4", "a8", "a4", "a8", "vec4"),
    "C12_x_m3": (12, "m3", "a8", "a4", "a8", "scalar"),
    "C12_y_mp": (12, "a4", "mp", "a4", "a8", "scalar"),
    "C12_dy_m3": (12, "a4", "a8", "m3", "a8", "scalar"),
    "C12_dx_mp": (12, "a4", "a8", "a4", "mp", "scalar"),
    "C7_dense": (7, "dense", "dense", "dense", "dense", "scalar"),
    "C7_slices": (7, "a4", "m3", "a8", "mp", "scalar"),
}
_pool_cache = {}


def _pool_data(C, win, ties):
    key = (C, win, ties)
    if key not in _pool_cache:
        g = _gen("pool%r" % (key,))
        k, s, p = POOL_WINDOWS[win]
        x = torch.randn(*POOL_NTHW, C, generator=g)
        if ties:
            x = torch.relu((x * 2).round() / 2)
        y = B.maxpool_fwd_ref(x, k, s, p)
        dy = torch.randn(y.shape, generator=g)
        base = torch.randn(x.shape, generator=g)
        _pool_cache[key] = (x, y, dy, base, B.maxpool_bwd_ref(x, dy, k, s, p, base), B.maxpool_bwd_ref(x, dy, k, s, p))
    return _pool_cache[key]


@pytest.mark.parametrize("ties", [False, True], ids=["distinct", "ties"])
@pytest.mark.parametrize("win", list(POOL_WINDOWS))
@pytest.mark.parametrize("name", list(POOL_VIEWS))
def test_maxpool_bwd(name, win, ties):
    import sfhip
    dev = _dev()
    C, kx, ky, kdy, kdx, route = POOL_VIEWS[name]
    assert B.maxpool_bwd_route(C, vw(kx, C), vw(ky, C), vw(kdy, C), vw(kdx, C)) == route
    k, s, p = POOL_WINDOWS[win]
    x, y, dy, base, (ref_a, mag_a), (ref_f, mag_f) = _pool_data(C, win, ties)
    xa, ya, dya = (B.view(dev, t, *vw(kk, C), NAN) for t, kk in ((x, kx), (y, ky), (dy, kdy)))
    acc = B.view(dev, base, *vw(kdx, C), B.SENTINEL)
    first = B.view(dev, torch.full(x.shape, NAN), *vw(kdx, C), B.SENTINEL)
    sfhip.maxpool_bwd(xa, ya, dya, acc, k, s, p)
    sfhip.maxpool_bwd(xa, ya, dya, first, k, s, p, overwrite=True)
    torch.cuda.synchronize()
    nwin = 1
    for kk, ss in zip(k, s):
        nwin *= -(-kk // ss)
    tag = "maxpool/%s_%s_%s" % (name, win, "ties" if ties else "distinct")
    _elementwise(tag + " acc", B.inside(acc), ref_a, mag_a, nwin + 3)
    if nwin == 1:
        assert torch.equal(B.inside(first).double(), ref_f), "a selection must be exact"
    else:
        _elementwise(tag + " first", B.inside(first), ref_f, mag_f, nwin + 2)
    for a in (acc, first):
        assert B.outside_is(a) or a.cs == C
    for a, host in ((xa, x), (ya, y), (dya, dy)):
        assert torch.equal(B.inside(a), host)


# ================================================================================================ ECA backward
ECA_VIEWS = {"C32": (32, "a4", "a8", "a4"), "C3": (3, "m3", "mp", "m3"), "C32_dense": (32, "dense", "dense", "dense")}


@pytest.mark.parametrize("alpha", [4, 8])
@pytest.mark.parametrize("name", list(ECA_VIEWS))
def test_tmax_dot_and_eca_bwd_apply(name, alpha):
    import sfhip
    dev = _dev()
    C, kx, kdz, kdx = ECA_VIEWS[name]
    g = _gen("eca" + name)
    N, T, H, W = 2, 8, 5, 7
    x = torch.relu((torch.randn(N, T, H, W, C, generator=g) * 2).round() / 2)  # frames tie (runs of zeros)
    dz = torch.randn(N, T // alpha, H, W, C, generator=g)
    gate, dpool = torch.rand(N, C, generator=g), torch.randn(N, C, generator=g) * 0.1
    base = torch.randn(x.shape, generator=g)
    xa = B.view(dev, x, *vw(kx, C), NAN)
    dza = B.view(dev, dz, *vw(kdz, C), NAN)
    dxa = B.view(dev, base, *vw(kdx, C), B.SENTINEL)
    dot = sfhip.tmax_dot(xa, alpha, dza)
    sfhip.eca_bwd_apply(xa, alpha, dza, gate.to(dev), dpool.to(dev), dxa)
    torch.cuda.synchronize()
    ref, mag = B.tmax_dot_ref(x, alpha, dz)
    _reduction("tmax_dot/%s_a%d" % (name, alpha), dot.cpu(), ref, mag, B.tmax_dot_chain(C, (T // alpha) * H * W))
    ref, mag = B.eca_apply_ref(x, alpha, dz, gate, dpool, base)
    _elementwise("eca_bwd_apply/%s_a%d" % (name, alpha), B.inside(dxa), ref, mag, 6)
    assert B.outside_is(dxa) or dxa.cs == C
    assert torch.equal(B.inside(xa), x) and torch.equal(B.inside(dza), dz)


@pytest.mark.parametrize("N,C", [(2, 3), (2, 32), (3, 100)], ids=["n6", "n64", "n300"])
def test_eca_gate_bwd(N, C):
    import sfhip
    dev = _dev()
    g = _gen("gate%d" % (N * C))
    dg, pooled, w3 = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g), torch.randn(3, generator=g)
    scale = 1.0 / 70
    dw = torch.full((3,), 0.5, device=dev)
    gate, dpool = sfhip.eca_gate_bwd(dg.to(dev), pooled.to(dev), w3.to(dev), scale, dw)
    torch.cuda.synchronize()
    ref = B.eca_gate_bwd_ref(dg, pooled, w3, scale)
    _elementwise("eca_gate_bwd/n%d gate" % (N * C), gate.cpu(), *ref["gate"], 8)
    _elementwise("eca_gate_bwd/n%d dpool" % (N * C), dpool.cpu(), *ref["dpool"], 13)
    _reduction("eca_gate_bwd/n%d dw3" % (N * C), dw.cpu(), ref["dw"][0] + 0.5, ref["dw"][1] + 0.5,
               B.cdiv(N * C, 256) + 256 + 1)


# ================================================================================================ rowdot
ROWDOT_CASES = {  # C, a kind, b kind, route, shift
    "C4": (4, "a4", "a8", "vec4", 0), "C8": (8, "a4", "dense", "vec4", 1), "C64": (64, "a8", "a4", "vec4", 4),
    "C256": (256, "dense", "a4", "vec4", 6), "C10": (10, "a4", "a8", "scalar", None),
    "C12": (12, "a4", "a8", "scalar", None), "C512": (512, "dense", "a4", "scalar", None),
    "C64_a_m3": (64, "m3", "a4", "scalar", None), "C64_b_mp": (64, "a4", "mp", "scalar", None),
}


@pytest.mark.parametrize("nthw", [NTHW, (1, 1, 1, 257)], ids=["rows210", "rows257"])
@pytest.mark.parametrize("name", list(ROWDOT_CASES))
def test_rowdot(name, nthw):
    import sfhip
    dev = _dev()
    C, ka, kb, route, shift = ROWDOT_CASES[name]
    r = B.rowdot_route(C, vw(ka, C), vw(kb, C))
    assert r[:2] == (route, shift)
    g = _gen("rowdot" + name)
    a, b = torch.randn(*nthw, C, generator=g), torch.randn(*nthw, C, generator=g)
    aa, ba = B.view(dev, a, *vw(ka, C), NAN), B.view(dev, b, *vw(kb, C), NAN)
    out = sfhip.rowdot(aa, ba, 0.3)
    torch.cuda.synchronize()
    ref, mag = B.rowdot_ref(a, b, 0.3)
    _reduction("rowdot/%s_rows%d" % (name, aa.rows), out.cpu(), ref, mag, r[2] + 1)
    assert torch.equal(B.inside(aa), a) and torch.equal(B.inside(ba), b)


# ================================================================================================ axpy, act_bwd, bcast_add, gather_add
FLAT_SHAPES = {"n1": ((1, 1, 1, 1), 1), "n255": ((1, 1, 1, 255), 1), "n256": ((1, 1, 1, 256), 1),
               "n257": ((1, 1, 1, 257), 1), "rows210_C10": (NTHW, 10), "rows210_C12": (NTHW, 12)}


def _flat_views(C):
    return ((3, C + 5), (2, C + 7)) if C != 12 else (vw("a4", C), vw("a8", C))


def _out_view(dev, shape, base, view):
    vals = base if base is not None else torch.full(shape, NAN)
    return B.view(dev, vals, view[0], view[1], B.SENTINEL)


@pytest.mark.parametrize("accumulate", [True, False], ids=["accumulate", "overwrite"])
@pytest.mark.parametrize("shape", list(FLAT_SHAPES))
def test_axpy_act_bwd_gather_add(shape, accumulate):
    import sfhip
    dev = _dev()
    nthw, C = FLAT_SHAPES[shape]
    g = _gen("flat" + shape)
    vin, vout = _flat_views(C)
    full = nthw + (C,)
    a = torch.randn(full, generator=g)
    base = torch.randn(full, generator=g) if accumulate else None
    tag = "%s_%s" % (shape, "acc" if accumulate else "ovw")
    # axpy
    aa, oa = B.view(dev, a, *vin, NAN), _out_view(dev, full, base, vout)
    sfhip.axpy(aa, oa, alpha=-1.7, accumulate=accumulate)
    torch.cuda.synchronize()
    _elementwise("axpy/" + tag, B.inside(oa), *B.axpy_ref(a, -1.7, base), 5 if accumulate else 4)
    assert B.outside_is(oa) and torch.equal(B.inside(aa), a)
    # act_bwd: ReLU and ReLU6 masks taken from the activation's output, boundaries included
    for relu in (True, 6):
        y = (torch.randn(full, generator=g) * 4.0).clamp(0.0, 6.0) if relu == 6 else torch.relu(torch.randn(full, generator=g))
        ya, oa = B.view(dev, y, *vout, NAN), _out_view(dev, full, base, vin)
        sfhip.act_bwd(aa, ya, relu, oa, accumulate=accumulate)
        torch.cuda.synchronize()
        ref, mag = B.act_bwd_ref(a, y, 2 if relu == 6 else 1, base)
        if accumulate:
            _elementwise("act_bwd/%s_relu%d" % (tag, int(relu)), B.inside(oa), ref, mag, 4)
        else:
            assert torch.equal(B.inside(oa).double(), ref), "a selection must be exact"
        assert B.outside_is(oa) and torch.equal(B.inside(ya), y)
    # gather_add: every cmul-th channel of a wider slice whose other channels hold NaN
    for cmul in (2, 3):
        span = (C - 1) * cmul + 1
        coff, pitch = 3, span + 5
        wide = torch.full(nthw + (pitch,), NAN)
        wide[..., coff:coff + span:cmul] = a
        src = sfhip.Act(wide.to(dev), coff, span)
        oa = _out_view(dev, full, base, vout)
        sfhip.gather_add(src, cmul, oa, accumulate=accumulate)
        torch.cuda.synchronize()
        ref, mag = B.gather_add_ref(wide, coff, cmul, C, base)
        if accumulate:
            _elementwise("gather_add/%s_cmul%d" % (tag, cmul), B.inside(oa), ref, mag, 4)
        else:
            assert torch.equal(B.inside(oa).double(), ref), "a selection must be exact"
        assert B.outside_is(oa)


@pytest.mark.parametrize("shape", list(FLAT_SHAPES))
def test_bcast_add(shape):
    import sfhip
    dev = _dev()
    nthw, C = FLAT_SHAPES[shape]
    g = _gen("bcast" + shape)
    base = torch.randn(nthw + (C,), generator=g)
    v = torch.randn(nthw[0], C, generator=g)
    ga = _out_view(dev, None, base, _flat_views(C)[1])
    sfhip.bcast_add(ga, v.to(dev), 0.3)
    torch.cuda.synchronize()
    _elementwise("bcast_add/" + shape, B.inside(ga), *B.bcast_add_ref(base, v, 0.3), 5)
    assert B.outside_is(ga)


# ================================================================================================ depthwise backward
DW_CASES = {  # C, in NTHW, kernel, stride, padding, dilation, x / dz / dx kinds, wgrad route, dgrad route
    "k133_C12": (12, (2, 4, 10, 10), (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1), "a4", "a8", "a4", "partial4<9,4>", "vec4"),
    "k333_C12": (12, (2, 4, 10, 10), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), "dense", "a4", "a8", "partial4<27,4>", "vec4"),
    "k133_C7": (7, (2, 4, 10, 10), (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1), "a4", "m3", "mp", "partial4<9,1>", "scalar"),
    "k333_C7": (7, (2, 4, 10, 10), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), "dense", "dense", "dense", "partial4<27,1>", "scalar"),
    "k133_C12_x_m3": (12, (2, 4, 10, 10), (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1), "m3", "a8", "a4", "partial4<9,1>", "vec4"),
    "k333_C12_dz_mp": (12, (2, 4, 10, 10), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), "a4", "mp", "a4", "partial4<27,1>", "scalar"),
    "k133_C12_dx_m3": (12, (2, 4, 10, 10), (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1), "a4", "a8", "m3", "partial4<9,4>", "scalar"),
    "k177_s2_C12": (12, (2, 2, 13, 11), (1, 7, 7), (1, 2, 2), (0, 3, 3), (1, 1, 1), "a4", "a8", "a4", "per-tap", "vec4"),
    "k177_s2_C7": (7, (2, 2, 13, 11), (1, 7, 7), (1, 2, 2), (0, 3, 3), (1, 1, 1), "m3", "a4", "dense", "per-tap", "scalar"),
    "k155_s121_C12": (12, (2, 4, 10, 10), (1, 5, 5), (1, 2, 1), (0, 2, 2), (1, 1, 1), "a4", "a4", "a8", "partial4<27,4>", "vec4"),
    "k133_d2_C12": (12, (2, 4, 10, 10), (1, 3, 3), (1, 1, 1), (0, 2, 2), (1, 2, 2), "a8", "a4", "a4", "partial4<9,4>", "vec4"),
    "k333_rows25_C12": (12, (1, 1, 5, 5), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), "a4", "a8", "a4", "partial4<27,4>", "vec4"),
    "k133_rows25_C7": (7, (1, 1, 5, 5), (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1), "a4", "a8", "a4", "partial4<9,1>", "scalar"),
}


@pytest.fixture
def generic_dw():
    """The row-march kernels switched off (a process-wide knob) so the generic kernels of backward.hip run on every
    shape; switched back on afterwards."""
    import sfhip
    L = sfhip.lib()
    try:
        assert L.sf_conv_tune(30, 0) == 0
        yield
    finally:
        L.sf_conv_tune(30, 1)


@pytest.mark.parametrize("name", list(DW_CASES))
def test_dwconv_backward(name, generic_dw):
    import sfhip
    dev = _dev()
    C, nthw, k, s, p, dil, kx, kdz, kdx, wroute, droute = DW_CASES[name]
    o = B.out_thw(nthw[1:], k, s, p, dil)
    rows, ntaps = nthw[0] * o[0] * o[1] * o[2], k[0] * k[1] * k[2]
    wr = B.dw_wgrad_route(C, rows, ntaps, vw(kx, C), vw(kdz, C))
    assert wr[0] == wroute and B.dw_dgrad_route(C, vw(kdz, C), vw(kdx, C), C) == droute
    g = _gen("dw" + name)
    x = torch.randn(*nthw, C, generator=g)
    dz = torch.randn(nthw[0], *o, C, generator=g)
    w = torch.randn(ntaps, C, generator=g) / ntaps ** 0.5
    base = torch.randn(x.shape, generator=g)
    xa, dza = B.view(dev, x, *vw(kx, C), NAN), B.view(dev, dz, *vw(kdz, C), NAN)
    dxa = B.view(dev, base, *vw(kdx, C), B.SENTINEL)
    d = sfhip._conv_desc(xa, o, 0, 0, C, k, s, p, dil, cin_pad=C)
    ws = torch.empty((sfhip.lib().sf_dwconv_wgrad_ws_floats(ctypes.byref(d), C),), dtype=torch.float32, device=dev)
    pbase = torch.randn(C, 1, *k, generator=g)
    guard = lambda vals: torch.cat([torch.full((8,), B.SENTINEL), vals.reshape(-1), torch.full((8,), B.SENTINEL)]).to(dev)
    packed, stored, summed = guard(torch.full((ntaps * C,), NAN)), guard(torch.full((ntaps * C,), NAN)), guard(pbase)
    n = ntaps * C
    head = (ctypes.byref(d), xa.ptr(), dza.ptr(), dza.cs, dza.coff, C)
    sfhip._call("sf_dwconv_wgrad", *head, _p(packed[8:8 + n]), _p(ws))
    sfhip._call("sf_dwconv_wgrad_param", *head, _p(stored[8:8 + n]), 0, _p(ws))
    sfhip._call("sf_dwconv_wgrad_param", *head, _p(summed[8:8 + n]), 1, _p(ws))
    wd = w.to(dev)
    sfhip._call("sf_dwconv_dgrad", ctypes.byref(d), dza.ptr(), dza.cs, dza.coff, _p(wd), dxa.ptr(), dxa.cs, dxa.coff, C)
    torch.cuda.synchronize()
    ref, mag = B.dw_wgrad_ref(x, dz, k, s, p, dil)
    packed, stored, summed = packed.cpu(), stored.cpu(), summed.cpu()
    _reduction("dw_wgrad/%s packed" % name, packed[8:8 + n].view(ntaps, C), ref, mag, wr[2])
    assert torch.equal(stored[8:8 + n].view(C, 1, *k), B.dw_to_param(packed[8:8 + n].view(ntaps, C), k)), \
        "the parameter layout holds other numbers than the packed one"
    pb = pbase.double()
    _reduction("dw_wgrad/%s param+=" % name, summed[8:8 + n].view(C, 1, *k), B.dw_to_param(ref, k) + pb,
               B.dw_to_param(mag, k) + pb.abs(), wr[2] + 1)
    for t in (packed, stored, summed):
        edge = torch.cat([t[:8], t[8 + n:]])
        assert torch.equal(edge.view(torch.int32), torch.full_like(edge, B.SENTINEL).view(torch.int32))
    ref, mag = B.dw_dgrad_ref(dz, w, nthw[1:], k, s, p, dil, base)
    _elementwise("dw_dgrad/" + name, B.inside(dxa), ref, mag, ntaps + 4)
    assert B.outside_is(dxa) or dxa.cs == C
    assert torch.equal(B.inside(xa), x) and torch.equal(B.inside(dza), dz)
