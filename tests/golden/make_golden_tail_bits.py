#!/usr/bin/env python3
"""Golden bits of the training-step tail: SHA-256 digests of what the loss kernels, the table optimizers and the gradient
clipper write, through the public Python API of slowfast/models/step_tail.py alone.  Every sum in those kernels runs in a
fixed order, so equal inputs give equal bits on every run; the digests pin them across changes that must not move a bit
(a refactor of the kernels' shared code, say).

Needs an MI355X and the built library.  Run ONCE on a checkout of the commit whose bits are to be kept; never to make a
failing tests/test_tail_bits_gpu.py pass: a digest that moved means the order of a sum or an fma moved.

`compute()` rebuilds the inputs from a seeded CPU generator and returns {name: digest}; tests/test_tail_bits_gpu.py
calls it and compares.  Writes tests/golden/tail_bits.json.

Losses: N = 5 rows (fewer than the 16 wavefronts: some take no row) of K = 70 classes (> 64: the lane stride wraps) at
row stride 72 (the `ld` path) — ce_topk, ce_topk_w, ce_mix (eps = 0.1, rows 0 and 3 mixed with each other), bce and
bce_w on logits and on probabilities, topk_errors; per call the gradient, the ring and `out`.
Table kernels: numel 1, 3, 4, 5, C - 1, C, C + 1, 2 C + 1 (C = sf_sgd_chunk_elems()) in two groups, the C + 1 tensor's
parameter and gradient 4 bytes off a 16-byte boundary — HipSGD (momentum, nesterov, weight decay), HipLARS (clip),
HipAdam, HipAdamW, two steps each; HipGradClip with norm types 2 and inf (max_norm below the norm), then clip_value."""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "efficient-slowfast_amd"))
sys.dont_write_bytecode = True

OUT = os.path.join(HERE, "tail_bits.json")
N, K, LD, TOPK = 5, 70, 72, 5
OFF_TENSOR = 6  # the C + 1 tensor: two chunks, both off 16 bytes
LRS = (0.1, 0.05)


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _rows(host, ld=LD):
    """host [N, K] on the GPU as a row view of stride `ld`."""
    buf = torch.zeros((host.shape[0], ld), dtype=host.dtype, device="cuda")
    buf[:, :host.shape[1]] = host.cuda()
    return buf[:, :host.shape[1]]


def losses(st, out):
    g = torch.Generator().manual_seed(1234)
    x = _rows(torch.randn((N, K), generator=g) * 3.0)
    y = torch.randint(0, K, (N,), generator=g).cuda()
    w = (torch.rand((K,), generator=g) + 0.5).cuda()
    pos = (torch.rand((K,), generator=g) + 0.5).cuda()
    t = _rows(torch.rand((N, K), generator=g))
    p = _rows(torch.rand((N, K), generator=g))
    mix = torch.zeros((N, 7), dtype=torch.int64)
    mix[:, 0] = torch.arange(N)
    mix[:, 2] = 0x3f800000                       # lam = 1.0f: the row is not mixed
    mix[0, :3] = torch.tensor([3, 1, 0x3e99999a])  # rows 0 and 3 mixed with each other, lam = 0.3f
    mix[3, :3] = torch.tensor([0, 1, 0x3e99999a])
    assert x.stride(0) == LD and t.stride(0) == LD

    def run(name, fn):
        ring, res = st.StatsRing(2), torch.zeros((2,), dtype=torch.float32, device="cuda")
        grad = fn(ring, res)
        if grad is not None:
            out[name + ".grad"] = digest(grad)
            out[name + ".out"] = digest(res)
        out[name + ".ring"] = digest(ring.rows)
        out[name + ".counter"] = digest(ring.counter)

    run("ce_topk", lambda ring, res: st.ce_topk(x, y, TOPK, ring, res))
    run("ce_topk_w", lambda ring, res: st.ce_topk_w(x, y, w, TOPK, ring, res))
    run("ce_mix", lambda ring, res: st.ce_mix(x, y, TOPK, ring, res, mix_host=mix, mix=mix.cuda(), smoothing=0.1))
    run("bce.logits", lambda ring, res: st.bce(x, t, True, ring, res))
    run("bce.probs", lambda ring, res: st.bce(p, t, False, ring, res))
    run("bce_w.logits", lambda ring, res: st.bce_w(x, t, True, ring, res, weight=w, pos_weight=pos))
    run("bce_w.probs", lambda ring, res: st.bce_w(p, t, False, ring, res, weight=w))
    run("topk_errors", lambda ring, res: st.topk_errors(x, y, TOPK, ring))


def _problem():
    import sfhip
    C = sfhip.lib().sf_sgd_chunk_elems()
    numels = [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 1]
    g = torch.Generator().manual_seed(4321)
    return numels, [torch.randn(n, generator=g) for n in numels], \
        [[torch.randn(n, generator=g) for n in numels] for _ in LRS]


def _tensors(numels, p0):
    """The parameters with their gradient views, each pair in allocations of its own; OFF_TENSOR's one float in."""
    params = []
    for i, (n, v) in enumerate(zip(numels, p0)):
        o = 1 if i == OFF_TENSOR else 0
        p = torch.nn.Parameter(torch.zeros((n + 4,), device="cuda")[o:o + n])
        p.data.copy_(v)
        p.grad = torch.zeros((n + 4,), device="cuda")[o:o + n]
        assert p.data_ptr() % 16 == 4 * o and p.grad.data_ptr() % 16 == 4 * o
        params.append(p)
    return params


def _load(params, grads):
    for p, g in zip(params, grads):
        p.grad.copy_(g)


def _groups(params):
    return [{"params": params[0::2], "weight_decay": 0.0}, {"params": params[1::2], "weight_decay": 5e-2}]


def optimizers(st, out):
    numels, p0, grads = _problem()
    sgd = dict(lr=LRS[0], momentum=0.9, nesterov=True)
    arms = (("sgd", lambda g: st.HipSGD(g, **sgd), ("momentum_buffer",)),
            ("lars", lambda g: st.HipLARS(g, trust_coefficient=0.02, clip=True, **sgd), ("momentum_buffer",)),
            ("adam", lambda g: st.HipAdam(g, lr=1e-2), ("exp_avg", "exp_avg_sq", "step")),
            ("adamw", lambda g: st.HipAdamW(g, lr=1e-2), ("exp_avg", "exp_avg_sq", "step")))
    for name, make, keys in arms:
        params = _tensors(numels, p0)
        opt = make(_groups(params))
        for s, lr in enumerate(LRS):  # the first-step path, then the steady one
            if name in ("sgd", "lars"):
                for gr in opt.param_groups:
                    gr["lr"] = lr
            _load(params, grads[s])
            opt.step()
        for i, p in enumerate(params):
            out["%s.p%d" % (name, i)] = digest(p)
            for k in keys:
                out["%s.%s%d" % (name, k, i)] = digest(opt.state[p][k])
        if name == "lars":
            out["lars.ratios"] = digest(opt.ratios)
            out["lars.guard"] = digest(opt.guard)


def clipping(st, out):
    numels, p0, grads = _problem()
    arms = (("clip.l2", dict(max_norm=1.0, norm_type=2.0)), ("clip.inf", dict(max_norm=0.5, norm_type=float("inf"))),
            ("clip.value", dict(clip_value=0.75)))
    for name, kw in arms:
        params = _tensors(numels, p0)
        _load(params, grads[0])
        clip = st.HipGradClip(params, **kw)
        clip.clip()
        if "max_norm" in kw:
            out[name + ".total_norm64"] = digest(clip.total_norm64)
            out[name + ".total_norm"] = digest(clip.total_norm)
            out[name + ".coef"] = digest(clip.coef)
            out[name + ".guard"] = digest(clip.guard)
        for i, p in enumerate(params):
            out["%s.g%d" % (name, i)] = digest(p.grad)


def compute():
    from slowfast.models import step_tail as st
    out = {}
    losses(st, out)
    optimizers(st, out)
    clipping(st, out)
    torch.cuda.synchronize()
    return out


def main():
    out = compute()
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d digests" % (OUT, len(out)))


if __name__ == "__main__":
    main()
