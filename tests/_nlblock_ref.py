"""Float64 restatements of the stripe pooling, the per-stripe broadcast add, their backward, and the two blocks built on
them (reference wdf_attention_helper.py:129-195 NonLocalBlock, :198-273 Stripe_NonLocalBlock), written from the cited
lines with plain torch ops — they never touch the library — plus the helpers the fixture tests share."""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM = 1e-5, 0.1  # nn.BatchNorm3d's defaults, which the reference keeps (:153, :234)
SAMPLE_ABOVE = 4096              # fixture tensors with more elements are stored as a strided sample of at most SAMPLE_N
SAMPLE_N = 4096


# ------------------------------------------------------------------------------------------------ ops (NDHWC)
def stripe_pool_ref(x, S, mode):
    """x [N,T,H,W,C] -> (out [N,T,S,Cout] float64, arg [N,T,S,C] int64 or None).  Stripe s = rows s*hs..(s+1)*hs-1, all W
    columns (:245-254); of equal maxima the FIRST position in (h, w) order, PyTorch's adaptive max-pool rule."""
    N, T, H, W, C = x.shape
    assert H % S == 0
    L = (H // S) * W
    xr = x.double().reshape(N, T, S, L, C)
    if mode == "sum":
        return xr.sum(3), None
    mean = xr.mean(3)
    if mode == "mean":
        return mean, None
    m = xr.max(3).values
    pos = torch.arange(L).view(1, 1, 1, L, 1).expand_as(xr)
    arg = torch.where(xr == m.unsqueeze(3), pos, torch.full_like(pos, L)).min(3).values
    return (m if mode == "max" else torch.cat([mean, m], -1)), arg


def stripe_add_ref(x, v):
    """z[n,t,h,w,c] = x[n,t,h,w,c] + v[n,t,h // hs,c] for v [N,T,S,C] (:269-271)."""
    N, T, H, W, C = x.shape
    S = v.shape[2]
    return x.double() + v.double().reshape(N, T, S, 1, 1, C).expand(N, T, S, H // S, W, C).reshape(N, T, H, W, C)


def stripe_pool_bwd_ref(shape, S, dz=None, dmean=None, dmax=None, arg=None):
    """dz + dmean / (hs*W) + [pos == arg] * dmax as float64 [N,T,H,W,C]; each term may be None."""
    N, T, H, W, C = shape
    L = (H // S) * W
    out = torch.zeros(N, T, S, L, C, dtype=torch.float64)
    if dz is not None:
        out += dz.double().reshape(N, T, S, L, C)
    if dmean is not None:
        out += dmean.double().reshape(N, T, S, 1, C) / L
    if dmax is not None:
        pos = torch.arange(L).view(1, 1, 1, L, 1)
        out += (pos == arg.reshape(N, T, S, 1, C)).double() * dmax.double().reshape(N, T, S, 1, C)
    return out.reshape(N, T, H, W, C)


# ------------------------------------------------------------------------------------------------ modules (NCTHW)
def _attend(theta, phi, g, instance, scale_by_keys=False):
    """theta [b, Nq, d], phi [b, d, Nk], g [b, Nk, dv] (:185-190, :260-265).  'dot' divides by f.shape[1] = Nq."""
    f = torch.matmul(theta, phi)
    if instance == "soft":
        f = torch.softmax(f, dim=-1)
    else:
        f = f / (f.shape[2] if scale_by_keys else f.shape[1])
    return torch.matmul(f, g)


def _bn(y, sd, pre, stats, training):
    """BatchNorm3d; training: batch statistics, `stats` = [running_mean, running_var] updated in place."""
    return F.batch_norm(y, stats[0], stats[1], sd[pre + "weight"], sd[pre + "bias"], training, BN_MOMENTUM, BN_EPS)


def nonlocal_block_ref(sd, x, case, stats, training, scale_by_keys=False):
    """NonLocalBlock.forward (:174-195)."""
    b = x.shape[0]
    sub = bool(case["sub_sample"])
    k = ("g.0.", "phi.0.") if sub else ("g.", "phi.")
    gx = F.conv3d(x, sd[k[0] + "weight"], sd[k[0] + "bias"])
    px = F.conv3d(x, sd[k[1] + "weight"], sd[k[1] + "bias"])
    if sub:
        gx, px = F.max_pool3d(gx, (1, 2, 2)), F.max_pool3d(px, (1, 2, 2))
    ci = gx.shape[1]
    tx = F.conv3d(x, sd["theta.weight"], sd["theta.bias"]).reshape(b, ci, -1).permute(0, 2, 1)
    y = _attend(tx, px.reshape(b, ci, -1), gx.reshape(b, ci, -1).permute(0, 2, 1), case["instance"], scale_by_keys)
    y = y.permute(0, 2, 1).reshape(b, ci, *x.shape[2:])
    if case["bn_layer"]:
        wy = _bn(F.conv3d(y, sd["W.0.weight"], sd["W.0.bias"]), sd, "W.1.", stats, training)
    else:
        wy = F.conv3d(y, sd["W.weight"], sd["W.bias"])
    return wy + x


def stripe_block_ref(sd, x, case, stats, training):
    """Stripe_NonLocalBlock.forward (:239-273)."""
    b, c, t, h, w = x.shape
    S = int(case["stripe"])
    assert S * (h // S) == h
    xr = x.reshape(b, c, t, S, (h // S) * w)
    avg, mx = xr.mean(-1, keepdim=True), xr.max(-1, keepdim=True).values
    discri = {"mean": avg, "max": mx, "meanmax": torch.cat([avg, mx], 1)}[case["pool_type"]]
    ci = sd["g.weight"].shape[0]
    g = F.conv3d(discri, sd["g.weight"], sd["g.bias"]).reshape(b, ci, -1).permute(0, 2, 1)
    theta = F.conv3d(discri, sd["theta.weight"], sd["theta.bias"]).reshape(b, ci, -1).permute(0, 2, 1)
    phi = F.conv3d(discri, sd["phi.weight"], sd["phi.bias"]).reshape(b, ci, -1)
    y = _attend(theta, phi, g, case["instance"]).permute(0, 2, 1).reshape(b, ci, t, S, 1)
    wy = _bn(F.conv3d(y, sd["W.0.weight"], sd["W.0.bias"]), sd, "W.1.", stats, training)
    wy = wy.reshape(b, c, t, S, 1, 1).expand(b, c, t, S, h // S, w).reshape(b, c, t, h, w)
    return wy + x


def is_param(key):
    return not key.endswith(("running_mean", "running_var", "num_batches_tracked"))


def module_ref(case, sd, x, g, dtype, scale_by_keys=False):
    """One train-mode step in `dtype` on the CPU, then the eval-mode forward with the updated running statistics.
    -> dict(out, dx, grads {param key: grad}, running_mean, running_var, eval_out); the running entries are None for
    a block without a BN."""
    sdr = {k: (v.to(dtype).clone().requires_grad_(True) if is_param(k) else v) for k, v in sd.items()}
    has_bn = "W.1.running_mean" in sd
    stats = [sd["W.1.running_mean"].to(dtype).clone(), sd["W.1.running_var"].to(dtype).clone()] if has_bn else None
    xr = x.to(dtype).clone().requires_grad_(True)

    def fwd(inp, training):
        if case["kind"] == "NonLocalBlock":
            return nonlocal_block_ref(sdr, inp, case, stats, training, scale_by_keys)
        return stripe_block_ref(sdr, inp, case, stats, training)

    out = fwd(xr, True)
    names = [k for k in sd if is_param(k)]
    grads = torch.autograd.grad(out, [xr] + [sdr[k] for k in names], g.to(dtype))
    with torch.no_grad():
        ev = fwd(x.to(dtype), False)
    return dict(out=out.detach(), dx=grads[0], grads=dict(zip(names, grads[1:])),
                running_mean=stats[0] if has_bn else None, running_var=stats[1] if has_bn else None, eval_out=ev)


# ------------------------------------------------------------------------------------------------ shared helpers
def rel_l2(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    n = float(ref.norm())
    return float((got - ref).norm()) / n if n > 0 else float((got - ref).norm())


ZERO_NORM = 1e-7  # a float64 reference gradient below this norm is an analytical zero


def err(got, ref, sibling=None):
    """rel_l2 — except where the float64 reference is an analytical zero (a conv bias in front of a train-mode BN, which
    removes the mean; g's bias under a softmax, whose rows sum to 1, in front of that BN; phi's bias under a softmax,
    which is shift invariant per query).  There is nothing to be relative to and fp32 leaves cancellation noise in
    proportion to the terms that cancel: the distance is then taken relative to the norm of `sibling`, the float64
    gradient of the same conv's WEIGHT (the same upstream gradient against inputs of order 1)."""
    if float(ref.double().norm()) < ZERO_NORM:
        d = float((got.double().cpu() - ref.double().cpu()).norm())
        return d / float(sibling.double().norm()) if sibling is not None else d
    return rel_l2(got, ref)


def grad_err(got, grads64, key):
    """err of the parameter gradient `key` against the float64 gradients `grads64` (bias -> its weight as sibling)."""
    return err(got, grads64[key], grads64.get(key[:-len("bias")] + "weight") if key.endswith("bias") else None)


def sample_index(numel):
    """Flat indices a fixture tensor of `numel` elements is stored at: all of them up to SAMPLE_ABOVE, else at most
    SAMPLE_N at an ODD stride (an even one would visit few columns of the even-sized dimensions)."""
    if numel <= SAMPLE_ABOVE:
        return None
    step = -(-numel // SAMPLE_N) | 1
    return np.arange(0, numel, step)


def stored(t):
    """What the fixture holds of the tensor `t` (see sample_index), as a flat or full torch tensor."""
    idx = sample_index(t.numel())
    return t if idx is None else t.reshape(-1)[torch.from_numpy(idx)]


def seeded_fill(module, seed, qk_scale=1.0):
    """Seeded non-zero values for every parameter and running statistic (a fresh block is the identity: its last BN /
    conv is zero) by tests/golden/paramgen.py's generator — the fill the fixture was made with.  qk_scale (a case's
    "qk_scale") then multiplies theta's and phi's weights and biases: max-pooled stripes of 280 standard normals are
    about +2.9 in EVERY channel, which the generic fill turns into logits of +-100 — a one-hot softmax whose
    gradients are fp32 noise in the reference itself (paramgen scales Nonlocal's theta / phi for the same reason)."""
    from paramgen import fill_state_dict
    fill_state_dict(module.state_dict(), seed)
    if qk_scale != 1.0:
        with torch.no_grad():
            for conv in (module.theta, module.phi):
                conv = conv[0] if isinstance(conv, torch.nn.Sequential) else conv
                conv.weight.mul_(qk_scale)
                conv.bias.mul_(qk_scale)
    return module


def fill_case(module, case):
    return seeded_fill(module, int(case["param_seed"]), float(case.get("qk_scale", 1.0)))


def build_kwargs(case):
    if case["kind"] == "NonLocalBlock":
        return dict(in_channels=int(case["C"]), sub_sample=bool(case["sub_sample"]), bn_layer=bool(case["bn_layer"]),
                    instance=case["instance"])
    return dict(stripe=int(case["stripe"]), in_channels=int(case["C"]), pool_type=case["pool_type"],
                instance=case["instance"])


def build_block(case):
    """The HIP-side module of a fixture case."""
    from slowfast.models import wdf_attention_helper as M
    cls = M.NonLocalBlock if case["kind"] == "NonLocalBlock" else M.Stripe_NonLocalBlock
    return cls(**build_kwargs(case))


def case_tensors(case):
    """(x, upstream gradient) of a fixture case, NCTHW float32, regenerated from its seeds."""
    from paramgen import make_upstream
    shape = tuple(case["shape"])
    x = torch.from_numpy(np.random.RandomState(int(case["input_seed"])).standard_normal(shape).astype(np.float32))
    return x, torch.from_numpy(make_upstream(int(case["upstream_seed"]), shape))
