"""float64 CPU references, error magnitudes and a restatement of the launch predicates of csrc/backward.hip, for
test_backward_ref_cpu.py and test_backward_views_gpu.py.

References.  Every reference takes the fp32 inputs the kernel gets, computes in float64 in closed form (no autograd)
and returns (ref, mag): mag is the sum of the absolute values of the terms added to make each output element, so one
fp32 rounding moves an element by at most 2^-24 * mag.  Tensors are NDHWC, [N, T, H, W, C].

Routes.  The *_route functions restate, in plain Python, which kernel a launcher of backward.hip picks for a case and
with what geometry; each names the lines it restates.  Views are (coff, pitch) pairs; base pointers and parameter
vectors are taken to be 16-byte aligned (torch allocations are) unless a case says otherwise, and the ticket ring to
be ready (it is allocated on first use outside a stream capture)."""
import torch

from _elementwise_ref import SENTINEL, U, inside, outside_is, rounds, view  # noqa: F401  (shared, not copied)

TPB = 256
MAX_P = 1024
EINVAL = "SF_EINVAL"


def cdiv(a, b):
    return -(-a // b)


def pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def f4(*views):
    """Every (coff, pitch) given is float4-addressable."""
    return all(v is None or (v[0] % 4 == 0 and v[1] % 4 == 0) for v in views)


# ================================================================================================ routes
def red_geometry(rows, C, vec):
    """backward.hip, red_geometry(): (CB, P)."""
    cv = cdiv(C, vec)
    CB = min(pow2ceil(cv), TPB)
    rpi = TPB // CB
    return CB, max(1, min(MAX_P, rows // (rpi * 8)))


def bn_reduce_route(C, nthw, dy, z, y, rep=1, relu=0, S=1, ring=True):
    """backward.hip, bn_bwd_reduce_launch(): the argument checks, `vec4`, `small` / `few` / fused, the CB = 16 form of
    `few`, the max_p clamps.  relu: 0 none, 1 ReLU, 2 ReLU6, 3 byte mask.  Returns EINVAL or a dict with the route
    name, P, chunks, CB, rpi, per (rows of one chunk) and L, the longest fp32 chain: the rows one thread walks, the
    `rep` copies summed into g and the LDS row-lane sum (the partials are then combined in fp64)."""
    N, T, H, W = nthw
    if relu == 3 and (rep != 1 or C % 4 != 0):
        return EINVAL
    if N % S != 0 or (S > 1 and N > MAX_P):
        return EINVAL
    rows = N * T * H * W
    vec4 = C % 4 == 0 and f4(dy, z) and (relu in (0, 3) or f4(y))
    if relu == 3 and not vec4:
        return EINVAL
    groups = N if S > 1 else 1
    group_rows = rows // groups
    CB, P = red_geometry(group_rows, C, 4 if vec4 else 1)
    small = ring and S == 1 and P <= 16
    few = (not small) and ring and S == 1 and vec4 and C >= 256
    max_p = 64 if few else (512 if small else MAX_P)
    if few and CB > 16:
        CB = 16
        P = max(1, min(max_p, group_rows // ((TPB // CB) * 8)))
    P = min(P, max_p)
    if P * groups > max_p:
        P = max_p // groups
    if P < 1:
        return EINVAL
    chunks, P = P, P * groups
    rpi = TPB // CB
    per = cdiv(group_rows, chunks)
    kind = "small-fused" if small else ("few-fused" if few else "two-launch")
    return dict(route=("vec4/" if vec4 else "scalar/") + kind, P=P, chunks=chunks, CB=CB, rpi=rpi, per=per,
                L=cdiv(per, rpi) + rep + rpi,
                four_row_trips=bool(vec4 and rep == 1 and relu in (0, 3) and per > 3 * rpi),
                ragged_tail=per % (4 * rpi) != 0)


def bn_apply_route(C, nthw, dy, z, y, dz, dres, rep=1, relu=0, params_aligned=True):
    """backward.hip, bn_bwd_apply_launch(): `vec4` (a conjunction over every view) and `unroll4`."""
    N, T, H, W = nthw
    rows = N * T * H * W
    vec4 = C % 4 == 0 and f4(dy, z, dz, dres) and (relu in (0, 3) or f4(y))
    if relu == 3 and (not vec4 or rep != 1):
        return EINVAL
    if not vec4:
        return "scalar"
    total = rows * (C // 4)
    unroll4 = (rep == 1 and relu in (0, 3) and total >= 262144 and total < 0x7fffffff and rows % 4 == 0 and
               params_aligned)
    return "unroll4" if unroll4 else "vec4"


def maxpool_bwd_route(C, x, y, dy, dx):
    """backward.hip, maxpool_bwd_launch(): `vec4`."""
    return "vec4" if C % 4 == 0 and f4(x, y, dy, dx) else "scalar"


def rowdot_route(C, a, b):
    """backward.hip, sf_rowdot(): the float4 / shuffle kernel for C / 4 a power of two <= 64.  Returns (route, shift,
    L): L is the fp32 chain of one output (four products, `shift` shuffle steps; C fused multiply-adds)."""
    cv = C // 4
    if C % 4 == 0 and cv <= 64 and (cv & (cv - 1)) == 0 and f4(a, b):
        shift = cv.bit_length() - 1
        return "vec4", shift, 4 + shift
    return "scalar", None, C


def dw_dgrad_route(C, dz, dx, wpitch):
    """backward.hip, sf_dwconv_dgrad(), below the march (switched off by the tests)."""
    return "vec4" if C % 4 == 0 and f4(dz, dx) and wpitch % 4 == 0 else "scalar"


def dw_quads_per_block(nq):
    CQ = 1
    while CQ < nq and CQ < 64:
        CQ <<= 1
    return CQ


def dw_row_blocks(C, rows):
    """backward.hip, dw_row_blocks()."""
    nq = C // 4 if C % 4 == 0 else C
    ncb = cdiv(nq, dw_quads_per_block(nq))
    return max(64, min(1024 // ncb, 512, rows // 64))


def dw_wgrad_route(C, rows, ntaps, x, dz):
    """backward.hip, dwconv_wgrad_impl(), below the march: (route, nblk, L).  L: rows one thread walks + the LDS
    row-lane sum; the blocks are combined in fp64."""
    if ntaps > 27:
        CB = min(pow2ceil(C), TPB)
        rpi = TPB // CB
        return "per-tap", 256, cdiv(cdiv(rows, 256), rpi) + rpi
    nblk = dw_row_blocks(C, rows)
    nt = 9 if ntaps <= 9 else 27
    if C % 4 == 0 and f4(x, dz):
        CQ, V = dw_quads_per_block(C // 4), 4
    else:
        CQ, V = dw_quads_per_block(C), 1
    rpi = TPB // CQ
    return "partial4<%d,%d>" % (nt, V), nblk, cdiv(cdiv(rows, nblk), rpi) + rpi


def tmax_dot_chain(C, rows_out):
    """backward.hip, tmax_dot_partial_kernel / pool_final_kernel: rows one thread walks, the LDS row-lane sum and the 64
    partials summed in fp32."""
    CB = min(pow2ceil(C), TPB)
    rpi = TPB // CB
    return cdiv(cdiv(rows_out, 64), rpi) + rpi + 64


ROUTES = {
    # vec4 is a condition of `few`: there is no scalar/few-fused
    "bn_reduce": ["vec4/small-fused", "scalar/small-fused", "vec4/few-fused", "vec4/two-launch", "scalar/two-launch"],
    "bn_apply": ["unroll4", "vec4", "scalar"],
    "maxpool": ["vec4", "scalar"],
    "rowdot": ["vec4", "scalar"],
    "dw_dgrad": ["vec4", "scalar"],
    "dw_wgrad": ["partial4<9,4>", "partial4<27,4>", "partial4<9,1>", "partial4<27,1>", "per-tap"],
}


# ================================================================================================ BN backward
def act_pass(y, relu, rep=1):
    """Which elements of the un-repeated layer pass a gradient: taken from copy 0 of every `rep` frames of y."""
    if not relu:
        return None
    N, TR, H, W, C = y.shape
    y0 = y.double().view(N, TR // rep, rep, H, W, C)[:, :, 0]
    ok = y0 > 0
    return ok & (y0 < 6) if relu in (2, 6) else ok


def bn_g_ref(dy, ok, rep=1):
    """dy [N, T*rep, H, W, C], ok bool [N, T, H, W, C] or None -> (g, mag) [N, T, H, W, C]."""
    N, TR, H, W, C = dy.shape
    d = dy.double().view(N, TR // rep, rep, H, W, C)
    g, mag = d.sum(2), d.abs().sum(2)
    if ok is not None:
        g, mag = g * ok, mag * ok
    return g, mag


def _per_sample(v, N, S):
    C = v.numel() // S
    return v.double().view(S, C)[torch.arange(N) % S].view(N, 1, 1, 1, C)


def bn_sums_ref(g, gmag, z, mean, invstd, S=1):
    """-> (dbeta, dgamma, mag_dbeta, mag_dgamma), each [S * C]: sample n belongs to split n % S."""
    N, C = g.shape[0], g.shape[-1]
    xhat = (z.double() - _per_sample(mean, N, S)) * _per_sample(invstd, N, S)
    outs = []
    for t in (g, g * xhat, gmag, gmag * xhat.abs()):
        outs.append(torch.stack([t[s::S].sum((0, 1, 2, 3)) for s in range(S)]).reshape(S * C))
    return tuple(outs)


def bn_dz_ref(g, gmag, z, mean, invstd, gamma, dbeta, dgamma, S=1):
    """dz = gamma*invstd*(g - dbeta/M - xhat*dgamma/M), M = rows / S; dbeta, dgamma: the fp32 sums the kernel is fed."""
    N = g.shape[0]
    M = g.numel() // g.shape[-1] / S
    ps = lambda v: _per_sample(v, N, S)
    xhat = (z.double() - ps(mean)) * ps(invstd)
    a = ps(gamma) * ps(invstd)
    b, c = ps(dbeta) / M, xhat * ps(dgamma) / M
    return a * (g - b - c), a.abs() * (gmag + b.abs() + c.abs())


def dres_ref(g, gmag, base):
    """base None: first writer (dres = g)."""
    if base is None:
        return g, gmag
    return base.double() + g, base.double().abs() + gmag


# ================================================================================================ windows
def out_thw(in_thw, kernel, stride, padding, dilation=(1, 1, 1)):
    return tuple((i + 2 * p - d * (k - 1) - 1) // s + 1 for i, k, s, p, d in zip(in_thw, kernel, stride, padding,
                                                                                   dilation))


def _taps(kernel):
    return [(a, b, c) for a in range(kernel[0]) for b in range(kernel[1]) for c in range(kernel[2])]  # scan order


def _tap_slices(tap, o_thw, stride, dilation):
    return tuple(slice(t * d, t * d + s * (o - 1) + 1, s) for t, o, s, d in zip(tap, o_thw, stride, dilation))


def _pad(x, padding, fill):
    N, T, H, W, C = x.shape
    p = padding
    out = torch.full((N, T + 2 * p[0], H + 2 * p[1], W + 2 * p[2], C), fill, dtype=torch.float64)
    out[:, p[0]:p[0] + T, p[1]:p[1] + H, p[2]:p[2] + W] = x.double()
    return out


def _unpad(xp, padding, thw):
    p = padding
    return xp[:, p[0]:p[0] + thw[0], p[1]:p[1] + thw[1], p[2]:p[2] + thw[2]]


def _windows(x, kernel, stride, padding, dilation, fill):
    """[N, To, Ho, Wo, C, taps]: the taps of every window in (t, h, w) scan order, `fill` outside the tensor."""
    o = out_thw(x.shape[1:4], kernel, stride, padding, dilation)
    xp = _pad(x, padding, fill)
    return torch.stack([xp[(slice(None),) + _tap_slices(t, o, stride, dilation)] for t in _taps(kernel)], -1)


def _scatter(contrib, in_thw, kernel, stride, padding, dilation):
    """The adjoint of _windows: contrib [N, To, Ho, Wo, C, taps] summed back onto [N, Ti, Hi, Wi, C]."""
    N, C = contrib.shape[0], contrib.shape[4]
    o = tuple(contrib.shape[1:4])
    acc = torch.zeros((N,) + tuple(i + 2 * p for i, p in zip(in_thw, padding)) + (C,), dtype=torch.float64)
    for i, t in enumerate(_taps(kernel)):
        acc[(slice(None),) + _tap_slices(t, o, stride, dilation)] += contrib[..., i]
    return _unpad(acc, padding, in_thw)


def maxpool_bwd_ref(x, dy, kernel, stride, padding, base=None):
    """nn.MaxPool3d's rule: a window's gradient goes to its FIRST maximum in (t, h, w) scan order.  -> (dx, mag)."""
    win = _windows(x, kernel, stride, padding, (1, 1, 1), float("-inf"))
    eq = win == win.amax(-1, keepdim=True)
    first = eq & (eq.cumsum(-1) == 1)
    d = dy.double().unsqueeze(-1) * first
    dx = _scatter(d, x.shape[1:4], kernel, stride, padding, (1, 1, 1))
    mag = _scatter(d.abs(), x.shape[1:4], kernel, stride, padding, (1, 1, 1))
    if base is not None:
        dx, mag = dx + base.double(), mag + base.double().abs()
    return dx, mag


def maxpool_fwd_ref(x, kernel, stride, padding):
    return _windows(x, kernel, stride, padding, (1, 1, 1), float("-inf")).amax(-1).float()


# ================================================================================================ depthwise conv
def dw_fwd_ref(x, w_packed, kernel, stride, padding, dilation=(1, 1, 1)):
    """w_packed [taps, C] -> y [N, To, Ho, Wo, C] (float64; used by the CPU cross-check only)."""
    return (_windows(x, kernel, stride, padding, dilation, 0.0) * w_packed.double().t()).sum(-1)


def dw_dgrad_ref(dz, w_packed, in_thw, kernel, stride, padding, dilation=(1, 1, 1), base=None):
    """dx = base + sum_taps dz[q(p, tap)] * w[tap]; w_packed [taps, >= C] -> (dx, mag)."""
    C = dz.shape[-1]
    d = dz.double().unsqueeze(-1) * w_packed.double()[:, :C].t()
    dx = _scatter(d, in_thw, kernel, stride, padding, dilation)
    mag = _scatter(d.abs(), in_thw, kernel, stride, padding, dilation)
    if base is not None:
        dx, mag = dx + base.double(), mag + base.double().abs()
    return dx, mag


def dw_wgrad_ref(x, dz, kernel, stride, padding, dilation=(1, 1, 1)):
    """-> (dw, mag) in the packed layout [taps, C]."""
    t = _windows(x, kernel, stride, padding, dilation, 0.0) * dz.double().unsqueeze(-1)
    return t.sum((0, 1, 2, 3)).t().contiguous(), t.abs().sum((0, 1, 2, 3)).t().contiguous()


def dw_to_param(dw_packed, kernel):
    """[taps, C] -> nn.Conv3d's depthwise layout [C, 1, kT, kH, kW]."""
    return dw_packed.t().reshape(dw_packed.shape[1], 1, *kernel).contiguous()


# ================================================================================================ ECA
def _tmax(x, alpha):
    N, T, H, W, C = x.shape
    return x.double().view(N, T // alpha, alpha, H, W, C)


def tmax_dot_ref(x, alpha, dz):
    """out[b, c] = sum_{t', hw} dz * max_r x[b, t'*alpha + r]  -> (out, mag) [N, C]."""
    t = _tmax(x, alpha).amax(2) * dz.double()
    return t.sum((1, 2, 3)), t.abs().sum((1, 2, 3))


def eca_apply_ref(x, alpha, dz, gate, dpool, base):
    """dx = base, plus dz * gate + dpool at the FIRST frame of every alpha that holds the temporal maximum."""
    N, T, H, W, C = x.shape
    xs = _tmax(x, alpha)
    eq = xs == xs.amax(2, keepdim=True)
    first = eq & (eq.cumsum(2) == 1)
    gb = lambda v: v.double().view(N, 1, 1, 1, 1, C)
    a = dz.double().unsqueeze(2) * gb(gate)
    dm, dmag = (a + gb(dpool)) * first, (a.abs() + gb(dpool).abs()) * first
    return base.double() + dm.reshape(x.shape), base.double().abs() + dmag.reshape(x.shape)


def eca_gate_bwd_ref(dg, pooled, w3, scale):
    """a = w (*) pooled along C (k = 3, zero padded), gate = sigmoid(a), da = dg * gate * (1 - gate),
    dpool[c] = (w0 da[c+1] + w1 da[c] + w2 da[c-1]) * scale, dw[k] = sum da[b, c] pooled[b, c+k-1].
    -> dict of (ref, mag) for gate, dpool, dw.  mag of gate and dpool carry the first-order effect of the roundings of
    `a` through the sigmoid (see test_backward_views_gpu.py)."""
    p, d, w = pooled.double(), dg.double(), w3.double()
    z = torch.zeros_like(p[:, :1])
    sh = lambda v, k: torch.cat([z, v[:, :-1]], 1) if k == 0 else (v if k == 1 else torch.cat([v[:, 1:], z], 1))
    a = sum(w[k] * sh(p, k) for k in range(3))
    amag = sum((w[k] * sh(p, k)).abs() for k in range(3))
    g = 1.0 / (1.0 + torch.exp(-a))
    da = d * g * (1 - g)
    gate_mag = g * (1 - g) * amag + g
    da_mag = d.abs() * (1 - 2 * g).abs() * gate_mag + da.abs()
    dpool = sum(w[k] * sh(da, 2 - k) for k in range(3)) * scale
    dpool_mag = sum(w[k].abs() * sh(da_mag, 2 - k) for k in range(3)) * abs(scale)
    dw = torch.stack([(da * sh(p, k)).sum() for k in range(3)])
    dw_mag = torch.stack([(da * sh(p, k)).abs().sum() for k in range(3)])
    return dict(gate=(g, gate_mag), dpool=(dpool, dpool_mag), dw=(dw, dw_mag))


# ================================================================================================ helpers
def rowdot_ref(a, b, scale):
    t = a.double() * b.double() * scale
    return t.sum(-1).reshape(-1), t.abs().sum(-1).reshape(-1)


def _into(v, base):
    if base is None:
        return v, v.abs()
    return base.double() + v, base.double().abs() + v.abs()


def axpy_ref(a, alpha, base):
    return _into(alpha * a.double(), base)


def bcast_add_ref(base, v, scale):
    """base [N, T, H, W, C] += v[n, c] * scale."""
    N, C = v.shape
    return _into(v.double().view(N, 1, 1, 1, C) * scale + torch.zeros_like(base.double()), base)


def act_bwd_ref(dy, y, relu, base):
    return _into(dy.double() * act_pass(y, relu), base)


def gather_add_ref(wide, coff, cmul, C, base):
    """out[r, c] (+)= wide[r, coff + c * cmul]."""
    return _into(wide.double()[..., coff:coff + (C - 1) * cmul + 1:cmul], base)
