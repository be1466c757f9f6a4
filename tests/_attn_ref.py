"""float64 CPU reference, seeded inputs and error measures for test_attention_views_gpu.py and test_attn_ref_cpu.py
(CPU only: nothing here imports the GPU library at module level; the view builders live in _elementwise_ref.py and
_conv_ref.py).

Semantics (attn_flash.hip): per clip, over the N = T * H * W positions and with NO 1/sqrt(d) scaling,
    S = q k^T,  P = softmax_j(S),  O = P v,  lse = logsumexp_j(S) * log2 e,
    y = gamma * O + x,  z = act(scale * y + bias), every frame of z repeated `alpha` times along T.
The backward kernels take dz = dL/dy: dq, dk, dv and dgamma come from autograd through this float64 graph with
L = <y, dz>; dvec_i = <dz_i, O_i> is what sfhip.attention_bwd returns (its sum is dgamma).

Inputs: unit-scale randn for 5 <= C <= 64 (as test_attention_bx_gpu.py draws them), q and k scaled by 0.7 outside that
range (as test_backward_ops_gpu.py::test_attention_backward does): the two groups carry the bounds of those tests."""
import zlib

import torch

LOG2E = 1.4426950408889634


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)


def tight(C):
    """True for the channel counts whose inputs are unit-scale and whose bounds are test_attention_bx_gpu.py's."""
    return 5 <= C <= 64


def attn_inputs(name, B, thw, C):
    """The fp32 tensors of a case: qkv [B,T,H,W,3C] (q | k | v), x and dz [B,T,H,W,C], gamma [1], scale of both signs
    in 0.5 .. 1.5 and bias [C]."""
    g = gen(name)
    t, h, w = thw
    qkv = torch.randn(B, t, h, w, 3 * C, generator=g)
    if not tight(C):
        qkv[..., :2 * C] *= 0.7
    x = torch.randn(B, t, h, w, C, generator=g)
    dz = torch.randn(B, t, h, w, C, generator=g)
    scale = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    bias = torch.randn(C, generator=g)
    gamma = torch.tensor([0.7 if tight(C) else 0.6])
    return dict(qkv=qkv, x=x, dz=dz, scale=scale, bias=bias, gamma=gamma)


def attn_ref(t):
    """-> dict of float64 tensors: o, y [B,N,C], lse, dvec [B,N], dq, dk, dv [B,N,C], dgamma [1]."""
    qkv = t["qkv"]
    B, C = qkv.shape[0], qkv.shape[-1] // 3
    flat = qkv.double().reshape(B, -1, 3 * C)
    q, k, v = [flat[..., i * C:(i + 1) * C].clone().requires_grad_(True) for i in range(3)]
    gamma = t["gamma"].double().clone().requires_grad_(True)
    s = q @ k.transpose(1, 2)
    o = torch.softmax(s, dim=-1) @ v
    y = gamma * o + t["x"].double().reshape(B, -1, C)
    dz = t["dz"].double().reshape(B, -1, C)
    dq, dk, dv, dgamma = torch.autograd.grad((y * dz).sum(), (q, k, v, gamma))
    return dict(o=o.detach(), y=y.detach(), lse=(torch.logsumexp(s, dim=-1) * LOG2E).detach(),
                dvec=(dz * o.detach()).sum(-1), dq=dq, dk=dk, dv=dv, dgamma=dgamma)


def epilogue_ref(y, thw, scale, bias, relu, alpha):
    """y [B,N,C] float64 -> z [B, T * alpha, H, W, C]."""
    B, _, C = y.shape
    z = y
    if scale is not None:
        z = z * scale.double() + bias.double()
    if relu:
        z = z.clamp_min(0.0)
    return z.reshape(B, thw[0], thw[1], thw[2], C).repeat_interleave(alpha, dim=1)


def errs(got, ref):
    """(max, rms) of |got - ref| over the reference's max magnitude — the measures of test_attention_bx_gpu.py."""
    e = (got.double() - ref).abs()
    m = ref.abs().max().clamp_min(1e-30)
    return float(e.max() / m), float(e.pow(2).mean().sqrt() / m)
