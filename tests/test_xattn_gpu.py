"""Streaming cross-length attention (sf_xattn_fwd / sf_xattn_bwd, attn_cross.hip) against torch fp64 on the CPU:
softmax(sm_scale Q K^T) V and its gradients by fp64 autograd, measured as max |a - b| / max |b| at the bound every
attention op test uses (tests/test_ops_gpu.py: TOL = 2e-4), through the binding and through the two modules it serves."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 2e-4
LOG2E = 1.4426950408889634


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _view(x, fill=None):
    """[B, N, C] cpu tensor (or a shape, with `fill`) -> Act view with pitch C + 8 and channel offset 4."""
    import sfhip
    shape = tuple(x) if fill is not None else tuple(x.shape)
    B, n, c = shape
    buf = torch.full((B, 1, 1, n, c + 8), 7.0 if fill is None else fill, dtype=torch.float32, device=_dev())
    if fill is None:
        buf[..., 4:4 + c] = x.view(B, 1, 1, n, c).to(buf.device)
    return sfhip.Act(buf, 4, c)


def _get(a):
    return a.buf[:, 0, 0, :, a.coff:a.coff + a.C].cpu()


def _reference(q, k, v, dy, sm_scale):
    qd, kd, vd = [t.double().requires_grad_(True) for t in (q, k, v)]
    y = torch.softmax(sm_scale * (qd @ kd.transpose(1, 2)), -1) @ vd
    y.backward(dy.double())
    return y.detach(), qd.grad, kd.grad, vd.grad


def _run(q, k, v, dy, sm_scale, accumulate=(False, False, False), prev=None):
    """Forward and backward through the binding on padded, offset views; returns (y, dq, dk, dv) on the CPU."""
    import sfhip
    qa, ka, va, dya = _view(q), _view(k), _view(v), _view(dy)
    saved = {}
    ya = sfhip.cross_attention(qa, ka, va, sm_scale, save=saved)
    grads = [_view(t.shape, fill=float("nan")) if p is None else _view(p)
             for t, p in zip((q, k, v), prev or (None, None, None))]
    sfhip.cross_attention_bwd(qa, ka, va, ya, dya, saved["lse"], sm_scale, grads[0], grads[1], grads[2],
                              accumulate=accumulate)
    torch.cuda.synchronize()
    for a in (qa, ka, va, dya) + tuple(grads):  # nothing outside the channel slice was written
        pad = torch.cat([a.buf[..., :4], a.buf[..., 4 + a.C:]], -1)
        assert bool(((pad == 7.0) | torch.isnan(pad)).all())
    return (_get(ya),) + tuple(_get(g) for g in grads)


def _check(name, got, ref, zero_scale=None):
    """zero_scale: for a gradient whose fp64 reference is IDENTICALLY zero (one key: the softmax is the constant 1, so
    dS = P (dP - D) cancels exactly and dQ = dK = 0) max |b| is no scale; the error is then measured against the size
    of the terms that cancel, zero_scale[name] = max over elements of sum |terms|, at the same TOL."""
    errs = {}
    for n, a, b in zip(("y", "dq", "dk", "dv"), got, ref):
        if zero_scale is not None and n in zero_scale and float(b.abs().max()) == 0.0:
            errs[n] = float(a.double().abs().max() / zero_scale[n])
        else:
            errs[n] = _rel(a, b)
    print("%s: %s" % (name, {n: "%.2e" % e for n, e in errs.items()}))
    assert all(bool(torch.isfinite(a).all()) for a in got), name
    assert max(errs.values()) < TOL, (name, errs)


def _inputs(nq, nk, d, dv, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, nq, d, generator=g), torch.randn(B, nk, d, generator=g), torch.randn(B, nk, dv, generator=g),
            torch.randn(B, nq, dv, generator=g))


SHAPES = [(50, 1, 20, 36), (33, 18, 16, 16), (300, 150, 24, 48), (96, 80, 256, 256), (70, 45, 512, 512),
          (40, 200, 132, 4)]


@pytest.mark.parametrize("nq,nk,d,dv", SHAPES)
def test_shape_sweep_forward_backward(nq, nk, d, dv):
    """B = 2 different samples, sm_scale = d^-0.5, pitch > width and a channel offset: Y, dQ, dK, dV."""
    _dev()
    q, k, v, dy = _inputs(nq, nk, d, dv, 10 + nq)
    sm = float(d) ** -0.5
    zero_scale = None
    if nk == 1:  # dS = sm P (dP - D) with P = 1 and dP = D: dQ = dS K and dK = dS^T Q are sums of cancelling terms
        qd, kd, vd, dyd = [t.double() for t in (q, k, v, dy)]
        terms = 2.0 * sm * (dyd.abs() @ vd.abs().transpose(1, 2))  # |dP| + |D| per (query, key)
        zero_scale = {"dq": float((terms @ kd.abs()).max()), "dk": float((terms.transpose(1, 2) @ qd.abs()).max())}
    _check("sweep %s" % ((nq, nk, d, dv),), _run(q, k, v, dy, sm), _reference(q, k, v, dy, sm), zero_scale)
    if nk == 1:  # one key: every query's output is that key's value row
        y = _run(q, k, v, dy, sm)[0]
        assert _rel(y, v.expand(2, nq, dv)) < 1e-6


def test_padded_keys_score_minus_infinity_not_zero():
    """All true scores near -30: a padded key scored 0 would outweigh every real key by e^30."""
    _dev()
    nq, nk, d = 64, 37, 32
    g = torch.Generator().manual_seed(5)
    u = torch.randn(d, generator=g)
    u = u / u.norm()
    sm = float(d) ** -0.5
    q = u * 4.0 + 0.05 * torch.randn(2, nq, d, generator=g)
    k = -u * (30.0 / (4.0 * sm)) + 0.3 * torch.randn(2, nk, d, generator=g)
    v = torch.randn(2, nk, d, generator=g)
    dy = torch.randn(2, nq, d, generator=g)
    scores = sm * (q @ k.transpose(1, 2))
    assert float(scores.max()) < -20
    _check("padded keys", _run(q, k, v, dy, sm), _reference(q, k, v, dy, sm))


@pytest.mark.parametrize("jump", [100, 10])
def test_online_softmax_rescale(jump):
    """The kernel's softmax reference is stale with 16 log2 units of headroom (XATTN_HEADROOM in attn_cross.hip).  One
    query spikes at a key in a LATE tile, another at an early key, `jump` log2 units above the rest: 100 is beyond the
    headroom (the refresh: accumulator and denominator rescaled), 10 inside it (the reference stays put and
    2^(s - m) reaches 2^10).  Forward and backward."""
    _dev()
    nq, nk, d = 128, 640, 32
    q, k, v, dy = _inputs(nq, nk, d, d, 1, B=1)
    k[0, 517] = q[0, 100] * (jump / LOG2E / float(q[0, 100].pow(2).sum()))
    k[0, 3] = q[0, 70] * (0.8 * jump / LOG2E / float(q[0, 70].pow(2).sum()))
    _check("rescale jump %d" % jump, _run(q, k, v, dy, 1.0), _reference(q, k, v, dy, 1.0))


def test_backward_is_deterministic_and_accumulates():
    _dev()
    q, k, v, dy = _inputs(300, 150, 24, 48, 77)
    sm = 24.0 ** -0.5
    first = _run(q, k, v, dy, sm)
    second = _run(q, k, v, dy, sm)
    for a, b in zip(first[1:], second[1:]):
        assert torch.equal(a, b)
    g = torch.Generator().manual_seed(78)
    prev = [torch.randn(t.shape, generator=g) for t in (q, k, v)]
    acc = _run(q, k, v, dy, sm, accumulate=(True, True, True), prev=prev)
    for a, b, p in zip(acc[1:], first[1:], prev):
        assert _rel(a, b + p) < 1e-6
    mixed = _run(q, k, v, dy, sm, accumulate=(False, True, False), prev=prev)  # the mask is per gradient
    assert torch.equal(mixed[1], first[1]) and torch.equal(mixed[3], first[3])
    assert _rel(mixed[2], first[2] + prev[1]) < 1e-6


def _act(x):
    import sfhip
    return sfhip.Act(x.detach().permute(0, 2, 3, 4, 1).contiguous().to(_dev()))


def _back(a):
    return a.buf[..., a.coff:a.coff + a.C].permute(0, 4, 1, 2, 3).contiguous().cpu()


def test_nonlocal_key_width_not_a_multiple_of_16():
    """Nonlocal(40, 20, (1,2,2), "softmax"), train mode: d = 20.  Output, input gradient and every parameter gradient
    against oracle.nonlocal_block under fp64 autograd, measured as tests/test_backward_ops_gpu.py measures them."""
    from oracle import slowfast_oracle as oracle
    from slowfast.models import engine
    from slowfast.models.nonlocal_helper import Nonlocal
    dev = _dev()
    torch.manual_seed(40)
    dim, pool, inst, thw = 40, (1, 2, 2), "softmax", (2, 6, 6)
    blk = Nonlocal(dim, dim // 2, pool, instantiation=inst).to(dev).train()
    with torch.no_grad():
        for k, v in blk.named_parameters():
            v.copy_(torch.randn_like(v) * (0.3 if v.dim() > 1 else 0.2) + (1.0 if k == "bn.weight" else 0.0))
    x = torch.randn((2, dim) + thw)
    dy = torch.randn((2, dim) + thw)
    sd = {"m." + k: v.detach().double().cpu().requires_grad_(v.dtype.is_floating_point and "running" not in k)
          for k, v in blk.state_dict().items() if "num_batches" not in k}
    xr = x.double().requires_grad_(True)
    ref = oracle.nonlocal_block(sd, "m", xr, pool, inst, True)
    ref.backward(dy.double())
    t = engine.Tape()
    xa = _act(x)
    with torch.no_grad(), engine.taping(t):
        ya = blk.run(xa)
        out = _back(ya)
        t.grad_of(ya).buf.copy_(dy.permute(0, 2, 3, 4, 1).to(dev))
        dxa = t.grad_of(xa)
        t.backward()
    torch.cuda.synchronize()
    errs = {"y": _rel(out, ref), "dx": _rel(_back(dxa), xr.grad)}
    for k, v in blk.named_parameters():
        a, b = t.pgrads[v].double().cpu(), sd["m." + k].grad
        scale = b.abs().max()
        if k.endswith(".bias"):  # exactly-zero bias gradients carry cancellation noise only: relative to the weight's
            scale = torch.maximum(scale, sd["m." + k[:-4] + "weight"].grad.abs().max())
        errs[k] = float((a.reshape(b.shape) - b).abs().max() / scale.clamp_min(1e-30))
    print("nonlocal d=20:", {k: "%.2e" % e for k, e in errs.items()})
    assert max(errs.values()) < TOL, errs


def test_no_score_matrix_in_memory():
    """Nonlocal(32, 16, None, "softmax") on x [1,32,2,48,48]: N_q = N_k = 4608, one score matrix = 85 MB.  Taped
    forward plus backward may raise the allocator's peak by less than 24 MB."""
    from slowfast.models import engine
    from slowfast.models.nonlocal_helper import Nonlocal
    dev = _dev()
    torch.manual_seed(3)
    blk = Nonlocal(32, 16, None, instantiation="softmax").to(dev).train()
    xa = _act(torch.randn(1, 32, 2, 48, 48))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t = engine.Tape()
    with torch.no_grad(), engine.taping(t):
        ya = blk.run(xa)
        t.grad_of(ya).buf.fill_(1.0)
        dxa = t.grad_of(xa)
        t.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise %.1f MB" % (rise / 1e6))
    assert bool(torch.isfinite(dxa.buf).all())
    assert rise < 24e6, rise


def test_nonlocal_forward_is_one_attention_launch():
    """B = 4: between the g projection and conv_out the trace holds one xattn_fwd and no per-sample conv."""
    import sfhip
    from slowfast.models.nonlocal_helper import Nonlocal
    dev = _dev()
    torch.manual_seed(4)
    blk = Nonlocal(32, 16, (1, 2, 2), instantiation="softmax").to(dev).eval()
    xa = _act(torch.randn(4, 32, 2, 8, 8))
    sfhip.EVENT_TRACE = []
    try:
        with torch.no_grad():
            blk.run(xa)
        torch.cuda.synchronize()
        tags = [e[0] for e in sfhip.EVENT_TRACE]
    finally:
        sfhip.EVENT_TRACE = None
    kinds = [tg[0] for tg in tags]
    assert kinds.count("xattn_fwd") == 1, kinds
    i = kinds.index("xattn_fwd")
    assert tags[i] == ("xattn_fwd", 4, 128, 32, 16, 16), tags[i]
    assert kinds[:i].count("conv") == 3 and kinds[i + 1:].count("conv") == 1, kinds


def test_wide_head_runs_on_the_streaming_kernels():
    """The 240-channel SpatialAttention head as the models build it (reduction = 1: q, k and v are all 240 wide; the
    class default of 8 would give 30-channel q / k rows, which are not float4-addressable) on x [2,240,1,8,8], eval."""
    import sfhip
    from oracle import slowfast_oracle as oracle
    from slowfast.models.wdf_attention_helper import SpatialAttention
    dev = _dev()
    c = 240
    g = torch.Generator().manual_seed(c)
    x = torch.randn(2, c, 1, 8, 8, generator=g)
    m = SpatialAttention(c, reduction=1)
    with torch.no_grad():
        for cv in (m.query_conv, m.key_conv, m.value_conv):
            cv.weight.copy_(torch.randn(cv.weight.shape, generator=g) * (0.7 / np.sqrt(c)))
            cv.bias.copy_(torch.randn(cv.bias.shape, generator=g) * 0.1)
        m.gamma.fill_(0.6)
    sd = {"m." + k: v.detach().double() for k, v in m.state_dict().items()}
    ref = oracle.spatial_attention(sd, "m", x.double())
    m = m.to(dev).eval()
    sfhip.EVENT_TRACE = []
    try:
        with torch.no_grad():
            y = m(x.to(dev))
        torch.cuda.synchronize()
        kinds = [e[0][0] for e in sfhip.EVENT_TRACE]
    finally:
        sfhip.EVENT_TRACE = None
    assert "xattn_fwd" in kinds, kinds
    assert _rel(y, ref) < TOL
