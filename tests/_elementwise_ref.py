"""float64 CPU references, error magnitudes and view builders for test_elementwise_views_gpu.py.

Every reference takes the fp32 inputs the kernel gets and computes in float64.  For the elementwise kernels it also
returns `mag`, the sum of the absolute values of the terms added to make each element: one fp32 rounding moves an
element by at most 2^-24 * mag, so the tests bound |got - ref| by a small number of roundings with no guessed
tolerance."""
import torch

U = 2.0 ** -24          # unit roundoff of fp32
SENTINEL = -7777.25     # what a buffer holds outside the view a kernel owns (exact in fp32, never a result)


def rounds(got, ref, mag):
    """max over elements of |got - ref| in units of 2^-24 * mag (elements with mag == 0 must match exactly)."""
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all()), "non-finite output"
    zero = mag == 0
    assert bool((err[zero] == 0).all()), "an element with nothing added to it is not exact"
    return float((err[~zero] / (U * mag[~zero])).max()) if bool((~zero).any()) else 0.0


def rel(got, ref):
    """max-norm relative error, the measure test_ops_gpu.py applies to the same kernels."""
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def view(dev, vals, coff, pitch, fill):
    """Act over channels [coff, coff + C) of a new [.., pitch] device buffer that holds `fill` everywhere else."""
    import sfhip
    C = vals.shape[-1]
    assert coff + C <= pitch
    buf = torch.full(tuple(vals.shape[:-1]) + (pitch,), fill, dtype=torch.float32)
    buf[..., coff:coff + C] = vals
    return sfhip.Act(buf.to(dev), coff, C)


def inside(a):
    return a.buf[..., a.coff:a.coff + a.C].cpu()


def outside_is(a, fill=SENTINEL):
    """True when every channel of the buffer that the view does not own still holds `fill`, bit for bit."""
    own = torch.zeros(a.cs, dtype=torch.bool)
    own[a.coff:a.coff + a.C] = True
    rest = a.buf.cpu()[..., ~own].contiguous()
    want = torch.full_like(rest, fill)
    return rest.numel() > 0 and torch.equal(rest.view(torch.int32), want.view(torch.int32))


def act_ref(y, relu):
    if relu == 6:
        return y.clamp(0.0, 6.0)
    return y.clamp_min(0.0) if relu else y


def affine_ref(x, scale, bias, res, relu, rep=1, nsplit=1):
    """x, res [N,T,H,W,C]; scale, bias [nsplit * C] (sample n takes block n % nsplit) -> (ref, mag) [N,T*rep,H,W,C]."""
    N, C = x.shape[0], x.shape[-1]
    y = x.double()
    if scale is not None:
        blk = torch.arange(N) % nsplit
        y = y * scale.double().view(nsplit, C)[blk].view(N, 1, 1, 1, C)
        b = bias.double().view(nsplit, C)[blk].view(N, 1, 1, 1, C)
        mag = y.abs() + b.abs()
        y = y + b
    else:
        mag = y.abs()
    if res is not None:
        y = y + res.double()
        mag = mag + res.double().abs()
    return (act_ref(y, relu).repeat_interleave(rep, dim=1), mag.repeat_interleave(rep, dim=1))


def mask_ref(y, relu):
    """y: the fp64 pre-activation [.., C] -> uint8 [rows * C/4]: bit e of byte [row * C/4 + c/4] is set iff channel
    c + e passes a gradient through the activation."""
    C = y.shape[-1]
    ok = y > 0
    if relu == 6:
        ok = ok & (y < 6)
    bits = ok.reshape(-1, C // 4, 4).to(torch.int32) << torch.arange(4, dtype=torch.int32)
    return bits.sum(-1).to(torch.uint8).reshape(-1)


def softmax_bwd_ref(p, dp, scale):
    pd, dd = p.double(), dp.double()
    return scale * pd * (dd - (pd * dd).sum(-1, keepdim=True))


def sigmoid_bwd_ref(y, dy, base):
    g = dy.double() * y.double() * (1.0 - y.double())
    if base is None:
        return g, g.abs()
    return base.double() + g, base.double().abs() + g.abs()


def to_ncthw(v):
    return v.permute(0, 4, 1, 2, 3)


def to_ndhwc(v):
    return v.permute(0, 2, 3, 4, 1)


def pool_ref(x, kernel, stride, padding, avg):
    """x [N,T,H,W,C] -> (ref, mag) in NDHWC; mag = sum |x| over the window's in-bounds taps / taps (average only)."""
    import torch.nn.functional as F
    xd = to_ncthw(x.double())
    if not avg:
        return to_ndhwc(F.max_pool3d(xd, kernel, stride, padding)), None
    ref = F.avg_pool3d(xd, kernel, stride, padding, count_include_pad=True)
    mag = F.avg_pool3d(xd.abs(), kernel, stride, padding, count_include_pad=True)
    return to_ndhwc(ref), to_ndhwc(mag)


def eca_ref(x, alpha, w3, scale, bias):
    """x [N,T,H,W,C] -> (pooled [N,C], out [N,T/alpha,H,W,C]): max over alpha frames, mean, 3-tap conv over channels,
    sigmoid gate, affine, ReLU."""
    import torch.nn.functional as F
    N, T, H, W, C = x.shape
    m = x.double().view(N, T // alpha, alpha, H, W, C).amax(2)
    pooled = m.mean((1, 2, 3))
    gate = torch.sigmoid(F.conv1d(pooled.unsqueeze(1), w3.double().view(1, 1, 3), None, 1, 1).squeeze(1))
    out = m * gate.view(N, 1, 1, 1, C) * scale.double() + bias.double()
    return pooled, out.clamp_min(0.0)
