"""float64 CPU references, term-magnitude sums, seeded inputs and the rounding bound for test_conv_views_gpu.py and
test_conv_ref_cpu.py (CPU only: nothing here imports the GPU library at module level).

Layouts: activations are NDHWC [N, T, H, W, C] as the kernels see them, weights nn.Conv3d's [Cout, Cin, kT, kH, kW].
Every reference takes the fp32 tensors the kernel gets, computes in float64 and also returns `mag`, the sum of the
absolute values of every term added into an element (the same linear map applied to absolute values, as
_elementwise_ref.affine_ref does it).

Bound: an fp32 sum of K products in ANY order, each product rounded once, is within (K + 8) * 2^-24 * mag of the exact
value to first order (K roundings of the running sum and the products, a few more for scale, bias, residual or an
accumulation base); K = taps * Cin (forward), taps * Cout (data gradient), N * To * Ho * Wo (weight gradient), S (the
split sum).  Derived, not tuned: test_conv_ref_cpu.py shows torch's own fp32 convolution inside it on the very inputs
the GPU cases use."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from _elementwise_ref import U, act_ref, rounds, to_ncthw, to_ndhwc  # noqa: F401  (re-exported for the tests)

EXTRA_ROUNDINGS = 8


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)


def bound(K):
    """Allowed |got - ref| in units of 2^-24 * mag for an element summed from K products."""
    return float(K + EXTRA_ROUNDINGS)


def out_thw(thw, kernel, stride, padding, dilation=(1, 1, 1)):
    return tuple((i + 2 * p - d * (k - 1) - 1) // s + 1 for i, k, s, p, d in zip(thw, kernel, stride, padding, dilation))


# ------------------------------------------------------------------------------------------------ references
def _conv(x, w, stride, padding, dilation):
    return to_ndhwc(F.conv3d(to_ncthw(x), w, None, stride, padding, dilation))


def conv_ref(x, w, bias, scale, res, act, stride, padding, dilation=(1, 1, 1)):
    """x, res NDHWC fp32; w [Cout, Cin, kT, kH, kW]; scale, bias [Cout] or None -> (ref, mag) NDHWC float64."""
    y = _conv(x.double(), w.double(), stride, padding, dilation)
    mag = _conv(x.double().abs(), w.double().abs(), stride, padding, dilation)
    if scale is not None:
        y, mag = y * scale.double(), mag * scale.double().abs()
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    if res is not None:
        y, mag = y + res.double(), mag + res.double().abs()
    return act_ref(y, act), mag


def _dgrad(dz, w, x_shape, stride, padding, dilation):
    n, t, h, wd, c = x_shape
    x0 = torch.zeros((n, c, t, h, wd), dtype=dz.dtype, requires_grad=True)
    y = F.conv3d(x0, w, None, stride, padding, dilation)
    (g,) = torch.autograd.grad(y, (x0,), to_ncthw(dz).contiguous())
    return to_ndhwc(g)


def dgrad_ref(dz, w, x_shape, stride, padding, dilation=(1, 1, 1), base=None):
    """dz NDHWC fp32 [N, To, Ho, Wo, Cout]; x_shape = the forward input's NDHWC shape; base: what the kernel
    accumulates onto (None: it overwrites) -> (ref, mag) NDHWC float64."""
    ref = _dgrad(dz.double(), w.double(), x_shape, stride, padding, dilation)
    mag = _dgrad(dz.double().abs(), w.double().abs(), x_shape, stride, padding, dilation)
    if base is not None:
        ref, mag = ref + base.double(), mag + base.double().abs()
    return ref, mag


def _wgrad(x, dz, w_shape, stride, padding, dilation):
    w0 = torch.zeros(w_shape, dtype=x.dtype, requires_grad=True)
    y = F.conv3d(to_ncthw(x).contiguous(), w0, None, stride, padding, dilation)
    (g,) = torch.autograd.grad(y, (w0,), to_ncthw(dz).contiguous())
    return g


def wgrad_ref(x, dz, w_shape, stride, padding, dilation=(1, 1, 1), base=None):
    """x, dz NDHWC fp32 -> (ref, mag) [Cout, Cin, kT, kH, kW] float64; base as in dgrad_ref."""
    ref = _wgrad(x.double(), dz.double(), w_shape, stride, padding, dilation)
    mag = _wgrad(x.double().abs(), dz.double().abs(), w_shape, stride, padding, dilation)
    if base is not None:
        ref, mag = ref + base.double(), mag + base.double().abs()
    return ref, mag


def finish_ref(part, cin, fold_kw, base=None):
    """part [S, Cout, taps, cin_pad] fp32 -> (ref, mag) float64 in the layout sf_conv_wgrad_finish writes:
    [Cout, Cin, taps], or for the stem form (a packed channel is (kw, ci) = (c / 4, c % 4)) [Cout, Cin, taps, fold_kw]."""
    s = part.double().sum(0)
    m = part.double().abs().sum(0)
    if fold_kw > 0:
        cout, taps = s.shape[0], s.shape[1]

        def unfold(v):
            return v[:, :, :4 * fold_kw].reshape(cout, taps, fold_kw, 4)[..., :cin].permute(0, 3, 1, 2).contiguous()
        s, m = unfold(s), unfold(m)
    else:
        s, m = s[:, :, :cin].permute(0, 2, 1).contiguous(), m[:, :, :cin].permute(0, 2, 1).contiguous()
    if base is not None:
        s, m = s + base.double().reshape(s.shape), m + base.double().abs().reshape(s.shape)
    return s, m


# ------------------------------------------------------------------------------------------------ fp32 counterparts
def conv_fp32(x, w, bias, scale, res, act, stride, padding, dilation=(1, 1, 1)):
    """torch's own fp32 convolution and epilogue of the same inputs (what a correct fp32 implementation gives)."""
    y = _conv(x, w, stride, padding, dilation)
    if scale is not None:
        y = y * scale
    if bias is not None:
        y = y + bias
    if res is not None:
        y = y + res
    return act_ref(y, act)


def dgrad_fp32(dz, w, x_shape, stride, padding, dilation=(1, 1, 1), base=None):
    g = _dgrad(dz, w, x_shape, stride, padding, dilation)
    return g if base is None else base + g


def wgrad_fp32(x, dz, w_shape, stride, padding, dilation=(1, 1, 1), base=None):
    g = _wgrad(x, dz, w_shape, stride, padding, dilation)
    return g if base is None else base + g


# ------------------------------------------------------------------------------------------------ seeded inputs
def conv_inputs(case):
    """The fp32 tensors of a case (a dict with name, cin, cout, k, s, p, nthw; res / act for the forward tables):
    x [N,T,H,W,Cin], w / sqrt(taps * Cin) so that outputs are O(1), scale of both signs in 0.5 .. 1.5, bias, res and
    dz over the output positions, base_dx / base_dw for the accumulating forms."""
    g = gen(case["name"])
    n, t, h, wd = case["nthw"]
    cin, cout, k = case["cin"], case["cout"], case["k"]
    to, ho, wo = out_thw((t, h, wd), k, case["s"], case["p"])
    assert min(to, ho, wo) > 0, case["name"]
    x = torch.randn(n, t, h, wd, cin, generator=g)
    w = torch.randn(cout, cin, *k, generator=g) / float(np.sqrt(cin * k[0] * k[1] * k[2]))
    scale = (torch.rand(cout, generator=g) + 0.5) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1).float()
    bias = torch.randn(cout, generator=g)
    if case.get("act") == 6:  # spread the pre-activation over both clamps
        scale, bias = scale * 3, bias * 3 + 2
    res = torch.randn(n, to, ho, wo, cout, generator=g)
    dz = torch.randn(n, to, ho, wo, cout, generator=g)
    base_dx = torch.randn(n, t, h, wd, cin, generator=g)
    base_dw = torch.randn(cout, cin, *k, generator=g)
    return dict(x=x, w=w, scale=scale, bias=bias, res=res, dz=dz, base_dx=base_dx, base_dw=base_dw)


def finish_inputs(case):
    """part [S, Cout, taps, cin_pad] (random in the real columns, the given `pad_fill` in the padding columns, which the
    finish kernels must drop) and a base in the destination's element count."""
    g = gen(case["name"])
    S, cout, taps, cin_pad, cin, fold = (case[k] for k in ("S", "cout", "taps", "cin_pad", "cin", "fold_kw"))
    part = torch.randn(S, cout, taps, cin_pad, generator=g)
    real = torch.zeros(cin_pad, dtype=torch.bool)
    if fold > 0:
        real.view(-1, 4)[:fold, :cin] = True
    else:
        real[:cin] = True
    part[..., ~real] = case.get("pad_fill", -7777.25)
    base = torch.randn(cout * cin * taps * max(fold, 1), generator=g)
    return dict(part=part, base=base)


# ------------------------------------------------------------------------------------------------ views
def shifted_view(dev, vals, coff, pitch, fill):
    """As _elementwise_ref.view, but the buffer starts ONE float into its allocation: pitch and offset may be multiples
    of 4 while no row is 16-byte addressable — what only a run-time pointer check can see.  Returns (Act, allocation);
    allocation[0] is the float in front of the buffer and holds `fill`."""
    import sfhip
    C = vals.shape[-1]
    assert coff + C <= pitch
    shape = tuple(vals.shape[:-1]) + (pitch,)
    flat = torch.full((int(np.prod(shape)) + 1,), fill, dtype=torch.float32)
    flat[1:].view(shape)[..., coff:coff + C] = vals
    flat = flat.to(dev)
    buf = flat[1:].view(shape)
    assert buf.is_contiguous() and buf.data_ptr() % 16 == 4
    return sfhip.Act(buf, coff, C), flat
