"""Float64 restatements of the global-context pooling, the per-sample affine and the two attention blocks built on them
(reference wdf_attention_helper.py:97-124 ChannelAttention, :289-379 ContextBlock3D), written from the cited lines with
plain torch ops — they never touch the library — plus the seeded parameter fill the module tests share."""
import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ ops (NDHWC)
def ctx_pool_ref(x, w, b):
    """x [N,T,H,W,C], w [C], b [1] -> (ctx [N,C], lse [N]) in float64 (spatial_pool, 'att': :341-358)."""
    N, C = x.shape[0], x.shape[-1]
    xf = x.double().reshape(N, -1, C)
    l = xf @ w.double().reshape(C) + b.double().reshape(())
    p = torch.softmax(l, dim=1)
    return (p.unsqueeze(-1) * xf).sum(1), torch.logsumexp(l, dim=1)


def ctx_pool_bwd_ref(x, w, b, dctx):
    """(dx [N,T,H,W,C], dw [C], db) of <dctx, ctx> by autograd in float64."""
    xd = x.double().clone().requires_grad_(True)
    wd = w.double().reshape(-1).clone().requires_grad_(True)
    bd = b.double().reshape(1).clone().requires_grad_(True)
    ctx, _ = ctx_pool_ref(xd, wd, bd)
    gx, gw, gb = torch.autograd.grad(ctx, (xd, wd, bd), dctx.double())
    return gx, gw, gb


def sample_affine_ref(x, mul, add):
    N, C = x.shape[0], x.shape[-1]
    y = x.double()
    if mul is not None:
        y = y * mul.double().view(N, 1, 1, 1, C)
    if add is not None:
        y = y + add.double().view(N, 1, 1, 1, C)
    return y


def sample_affine_bwd_ref(dy, x, mul):
    """-> (dx, dmul [N,C], dadd [N,C]) in float64."""
    N, C = dy.shape[0], dy.shape[-1]
    g = dy.double()
    dx = g * mul.double().view(N, 1, 1, 1, C) if mul is not None else g.clone()
    return dx, (g * x.double()).sum((1, 2, 3)), g.sum((1, 2, 3))


# ------------------------------------------------------------------------------------------------ modules (NCTHW)
def channel_attention_ref(sd, x):
    """x [N,C,T,H,W]; sd: conv_du.0 / conv_du.2 weights and biases (:121-124): y = sigmoid(W2 relu(W1 mean(x) + b1) + b2),
    out = x * y + x."""
    y = x.mean((2, 3, 4), keepdim=True)
    y = torch.relu(F.conv3d(y, sd["conv_du.0.weight"], sd["conv_du.0.bias"]))
    y = torch.sigmoid(F.conv3d(y, sd["conv_du.2.weight"], sd["conv_du.2.bias"]))
    return x * y + x


def context_block_ref(sd, x, pooling_type, eps=1e-5):
    """x [N,C,T,H,W]; 'channel_add' fusion only (:339-379)."""
    N, C = x.shape[:2]
    if pooling_type == "att":
        flat = x.reshape(N, C, -1)
        mask = F.conv3d(x, sd["conv_mask.weight"], sd["conv_mask.bias"]).reshape(N, 1, -1)
        mask = torch.softmax(mask, dim=2)
        context = torch.matmul(flat.unsqueeze(1), mask.unsqueeze(-1)).reshape(N, C, 1, 1, 1)
    else:
        context = x.mean((2, 3, 4), keepdim=True)
    h = F.conv3d(context, sd["channel_add_conv.0.weight"], sd["channel_add_conv.0.bias"])
    h = F.layer_norm(h, tuple(h.shape[1:]), sd["channel_add_conv.1.weight"], sd["channel_add_conv.1.bias"], eps)
    h = F.conv3d(torch.relu(h), sd["channel_add_conv.3.weight"], sd["channel_add_conv.3.bias"])
    return x + h


def module_ref(kind, pooling_type, sd, x, g, dtype):
    """Train-mode output, dL/dx and every parameter gradient of <g, block(x)> in `dtype` (CPU)."""
    sdr = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.to(dtype).clone().requires_grad_(True)
    out = channel_attention_ref(sdr, xr) if kind == "ChannelAttention" else context_block_ref(sdr, xr, pooling_type)
    names = sorted(sdr)
    grads = torch.autograd.grad(out, [xr] + [sdr[k] for k in names], g.to(dtype), allow_unused=True)
    pg = {k: (v if v is not None else torch.zeros_like(sdr[k])) for k, v in zip(names, grads[1:])}
    return out.detach(), grads[0], pg


def rel_l2(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    n = float(ref.norm())
    return float((got - ref).norm()) / n if n > 0 else float((got - ref).norm())


def seeded_fill(module, seed):
    """Every parameter of `module` gets seeded non-zero values (a fresh block is the identity: its last conv is zero),
    by tests/golden/paramgen.py's generator — the same fill the fixture was made with."""
    from paramgen import fill_state_dict
    fill_state_dict(module.state_dict(), seed)
    return module


def build_block(case):
    """The HIP-side module of a fixture case {kind, C, reduction | ratio, pooling_type}."""
    from slowfast.models.wdf_attention_helper import ChannelAttention, ContextBlock3D
    if case["kind"] == "ChannelAttention":
        return ChannelAttention(int(case["C"]), reduction=int(case["reduction"]))
    return ContextBlock3D(int(case["C"]), ratio=float(case["ratio"]), pooling_type=case["pooling_type"])


def case_tensors(case):
    """(x, upstream gradient) of a fixture case, NCTHW float32, regenerated from its seeds."""
    from paramgen import make_upstream
    shape = tuple(case["shape"])
    x = torch.from_numpy(np.random.RandomState(int(case["input_seed"])).standard_normal(shape).astype(np.float32))
    return x, torch.from_numpy(make_upstream(int(case["upstream_seed"]), shape))
