"""The reference helper of test_attention_views_gpu.py, checked without a GPU: on one tiny case its O, log2-domain lse,
gradients, dvec and dgamma agree with torch.autograd through F.scaled_dot_product_attention on dense float64 tensors and
with the closed-form backward the kernels implement (attn_bwd.hip's header); the epilogue agrees with a frame-by-frame
loop; the seeded input maker is deterministic and draws the two input scales the bounds are tied to."""
import torch
import torch.nn.functional as F

import _attn_ref as A

B, THW, C = 2, (2, 3, 5), 6
N = THW[0] * THW[1] * THW[2]


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_reference_matches_autograd_and_closed_form():
    t = A.attn_inputs("ref_cpu", B, THW, C)
    r = A.attn_ref(t)
    flat = t["qkv"].double().reshape(B, N, 3 * C)
    q, k, v = [flat[..., i * C:(i + 1) * C].clone().requires_grad_(True) for i in range(3)]
    gamma = t["gamma"].double().clone().requires_grad_(True)
    x, dz = t["x"].double().reshape(B, N, C), t["dz"].double().reshape(B, N, C)
    o = F.scaled_dot_product_attention(q, k, v, scale=1.0)
    y = gamma * o + x
    y.backward(dz)
    assert _close(r["o"], o.detach()) and _close(r["y"], y.detach())
    assert _close(r["dq"], q.grad) and _close(r["dk"], k.grad) and _close(r["dv"], v.grad)
    assert _close(r["dgamma"], gamma.grad)
    # closed form: P from the saved lse, dO = gamma dz, D = <dO, O>, dS = P (dP - D)
    with torch.no_grad():
        s = q @ k.transpose(1, 2)
        p = torch.exp2(s * A.LOG2E - r["lse"].unsqueeze(-1))
        assert _close(p.sum(-1), torch.ones(B, N, dtype=torch.float64))
        do = gamma * dz
        ds = p * (do @ v.transpose(1, 2) - (do * r["o"]).sum(-1, keepdim=True))
        assert _close(r["dv"], p.transpose(1, 2) @ do)
        assert _close(r["dq"], ds @ k) and _close(r["dk"], ds.transpose(1, 2) @ q)
        assert _close(r["dvec"], (dz * o).sum(-1)) and _close(r["dvec"].sum().view(1), r["dgamma"])


def test_epilogue_reference():
    t = A.attn_inputs("ref_cpu", B, THW, C)
    y = A.attn_ref(t)["y"]
    plain = A.epilogue_ref(y, THW, None, None, False, 1)
    assert plain.shape == (B,) + THW + (C,) and torch.equal(plain.reshape(B, N, C), y)
    alpha = 2
    z = A.epilogue_ref(y, THW, t["scale"], t["bias"], True, alpha)
    assert z.shape == (B, THW[0] * alpha, THW[1], THW[2], C)
    want = (y * t["scale"].double() + t["bias"].double()).clamp_min(0.0).reshape(B, *THW, C)
    for f in range(THW[0] * alpha):
        assert torch.equal(z[:, f], want[:, f // alpha])
    assert bool((z == 0).any()) and bool((z > 0).any())   # the ReLU cuts some and passes some


def test_input_maker_is_deterministic_and_scaled():
    a, b = A.attn_inputs("c8_n35", B, THW, 8), A.attn_inputs("c8_n35", B, THW, 8)
    assert all(torch.equal(a[key], b[key]) for key in a)
    other = A.attn_inputs("c8_n36", B, THW, 8)
    assert not torch.equal(a["qkv"], other["qkv"])
    assert all(v.dtype == torch.float32 for v in a.values())
    assert bool((a["scale"] < 0).any()) and bool((a["scale"] > 0).any())
    assert float(a["scale"].abs().min()) >= 0.5 and float(a["scale"].abs().max()) <= 1.5
    # unit scale inside 5 .. 64 channels, q and k at 0.7 outside it; v, x, dz always unit scale
    big = (4, 7, 11)
    for c, qk in ((4, 0.7), (5, 1.0), (64, 1.0), (65, 0.7), (128, 0.7)):
        assert A.tight(c) == (qk == 1.0)
        t = A.attn_inputs("scale_c%d" % c, 2, big, c)
        assert abs(float(t["qkv"][..., :2 * c].std()) - qk) < 0.05, c
        assert abs(float(t["qkv"][..., 2 * c:].std()) - 1.0) < 0.06, c
        assert torch.equal(t["gamma"], torch.tensor([0.7 if qk == 1.0 else 0.6]))
