"""End-to-end GPU parity of the grayscale models at the driver-monitoring YAMLs' own spatial strides
(RESNET.SPATIAL_STRIDES [[1,1],[1,1],[2,2],[2,2]]) against golden vectors produced by the REFERENCE itself
(tests/golden/make_golden_tired.py).  res5 is crop/16 wide under the head's crop//32 window, so the head is fully
convolutional: pooled extent 1 x 3 x 3 at crop 64 and TRAINING logits [2, 27], ordered ((t*Ho + h)*Wo + w)*classes + k
(reference head_helper.py:198-223) — pooled by sf_avgpool_win_fwd, differentiated by sf_avgpool_win_bwd.

Measures and bounds are those of tests/test_gray_models_gpu.py: max-norm relative error < 1e-3 at every recorded child
boundary, the pre-activation logits and the output; the train step's loss within 1e-3 absolute, every recorded
gradient's sampled relative L2 error < 8e-2 (< 0.3 for a parameter of fewer than 16 elements) and its norm within 5 %
for a gradient of at least 16 elements; every parameter has a gradient.

The floor of those measures — the reference in fp32 against itself in fp64, `make_golden_tired.py check`:
  fast_r18_gray_tired_s64: eval out 1.07e-07, train logits 3.49e-06, |loss diff| 7.77e-07; gradients' L2rel at most
                           1.244e-02 (s2.pathway0_res1.branch2.b.weight), norms within 0.07 %
  dual_r18_gray_tired_s64: eval out 9.27e-08, train logits 5.41e-06, |loss diff| 1.09e-06; gradients' L2rel at most
                           1.544e-02 (the scalar s2_fuse.attention_spatial_s2f.gamma, norm 1.0672e-01 vs 1.0839e-01 =
                           1.5 %), 7.9e-03 and norms within 0.6 % on the others

Dropout (p = 0.5) runs on torch.native_dropout over the pooled [N,1,3,3,C] buffer; the reference draws its mask on a
permuted, non-contiguous tensor there, so masks are not compared with it: the tests below check seeding and that the
forward's mask is the backward's."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

from _gray import build_gray, gray_inputs
from _tired import TIRED_CASES, TRAIN_LOGITS
from _util import rel_err, sample_activation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TOL = 1e-3


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.parametrize("name", TIRED_CASES)
def test_tired_eval_forward_matches_reference_golden(name):
    _need_gpu()
    import sfhip
    from slowfast.models import head_helper
    model, sd, z, meta, cfg = build_gray(name)
    model.eval()
    acts, tap = {}, {}

    def hook(child):
        def f(m, i, o):
            if isinstance(o, (list, tuple)):
                acts[child] = [sfhip.to_ncthw(a).cpu().numpy() if isinstance(a, sfhip.Act) else a.cpu().numpy()
                               for a in o]
        return f

    for n, m in model.named_children():
        m.register_forward_hook(hook(n))
    head_helper.LOGITS_TAP = lambda t: tap.__setitem__("logits", t.detach().cpu().numpy())
    try:
        with torch.no_grad():
            out = model([x.cuda() for x in gray_inputs(meta)])
        torch.cuda.synchronize()
    finally:
        head_helper.LOGITS_TAP = None
    checked = 0
    for child in z["children"]:
        child = str(child)
        if child not in acts:
            continue
        for i, a in enumerate(acts[child]):
            tag = "eval/%s/%d" % (child, i)
            assert tuple(a.shape) == tuple(z[tag + "/shape"]), tag
            s, amax, mean = sample_activation(a)
            e = rel_err(s, z[tag])
            print("%-24s %-10s p%d %.3e" % (name, child, i, e))
            assert e < TOL, (tag, e)
            checked += 1
    assert checked >= (5 if meta.get("single") else 16)
    assert tuple(acts["s5"][0].shape[-2:]) == (4, 4)  # res5 at crop/16
    assert tuple(tap["logits"].shape[:4]) == (meta["batch"], 1, 3, 3)
    e_log = rel_err(tap["logits"].reshape(meta["batch"], -1), z["eval/logits_full"])
    e_out = rel_err(out.cpu().numpy(), z["eval/out"])
    print("%-24s logits %.3e out %.3e" % (name, e_log, e_out))
    assert e_log < TOL and e_out < TOL


@pytest.mark.parametrize("name", TIRED_CASES)
def test_tired_train_step_matches_reference_golden(name):
    """logits = model(x); loss = CE(logits, labels); loss.backward() (train_net.py:78-96), dropout off."""
    _need_gpu()
    model, sd, z, meta, cfg = build_gray(name)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.train()
    logits = model([x.cuda() for x in gray_inputs(meta)])
    assert tuple(logits.shape) == (2, TRAIN_LOGITS) == tuple(z["train/logits"].shape)
    labels = torch.from_numpy(z["train/labels"]).cuda()
    loss = torch.nn.functional.cross_entropy(logits, labels)
    loss.backward()
    torch.cuda.synchronize()
    e = rel_err(logits.detach().cpu().numpy(), z["train/logits"])
    print("%-24s train logits %.3e  loss %.6f vs %.6f" % (name, e, loss.item(), float(z["train/loss"][0])))
    assert e < TOL
    assert abs(loss.item() - float(z["train/loss"][0])) < 1e-3
    params = dict(model.named_parameters())
    keys = [k[5:] for k in z.files if k.startswith("grad/") and not k.endswith("/stats")]
    assert len(keys) >= 4 and "s1.pathway0_stem.conv.weight" in keys and "head.projection.weight" in keys
    assert meta.get("single") or "s1.pathway1_stem.conv.weight" in keys
    for k in keys:
        g = params[k].grad
        assert g is not None, k
        s, amax, _ = sample_activation(g.cpu().numpy(), 4096)
        ref = z["grad/" + k].astype(np.float64)
        e = float(np.linalg.norm(s.astype(np.float64) - ref) / max(np.linalg.norm(ref), 1e-30))
        norm, rnorm = float(g.norm()), float(z["grad/" + k + "/stats"][1])
        print("%-24s grad %-50s L2rel %.3e  |g| %.4e vs %.4e" % (name, k, e, norm, rnorm))
        assert e < (0.3 if g.numel() < 16 else 8e-2), (k, e)
        if g.numel() >= 16:
            assert abs(norm - rnorm) < 5e-2 * rnorm + 1e-9, (k, norm, rnorm)
    missing = [k for k, p in params.items() if p.grad is None]
    assert not missing, missing[:5]


def _dropout_model(name):
    model, sd, z, meta, cfg = build_gray(name)
    drops = [m for m in model.modules() if isinstance(m, torch.nn.Dropout)]
    assert drops, "the head has a dropout layer"
    for m in drops:
        m.p = 0.5
    model.train()
    xs = [x.cuda() for x in gray_inputs(meta)]
    labels = torch.from_numpy(z["train/labels"]).cuda()
    return model, xs, labels


def _train_step(model, xs, labels, seed, backward=True):
    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    logits = model(xs)
    if backward:
        torch.nn.functional.cross_entropy(logits, labels).backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if backward}


@pytest.mark.parametrize("name", TIRED_CASES)
def test_tired_dropout_follows_the_seed(name):
    """p = 0.5: two train steps under one torch.manual_seed give bitwise-equal logits and gradients, another seed
    gives other logits."""
    _need_gpu()
    model, xs, labels = _dropout_model(name)
    l1, g1 = _train_step(model, xs, labels, 1234)
    l2, g2 = _train_step(model, xs, labels, 1234)
    l3, _ = _train_step(model, xs, labels, 99, backward=False)
    assert tuple(l1.shape) == (2, TRAIN_LOGITS) and bool(torch.isfinite(l1).all())
    assert torch.equal(l1, l2), "logits differ under one seed"
    assert set(g1) == set(g2) == set(dict(model.named_parameters()))
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    assert not torch.equal(l1, l3), "another seed drew the same mask"


@pytest.mark.parametrize("name", TIRED_CASES)
def test_tired_dropout_mask_is_the_same_forward_and_backward(name):
    """The logits are linear in W = head.projection.weight for a fixed mask: logits = drop(pooled) W^T + b.  So for any
    D, <dL/dW, D> = <dL/dlogits, logits(W + D) - logits(W)> with dL/dlogits = (softmax - onehot) / N — which holds
    only if the backward multiplies by the mask the forward drew and the weight gradient sums the N * 9 rows the
    forward projected.  Relative 1e-3: fp32 rounding of a linear map (the reference's logits floor is 5e-6)."""
    _need_gpu()
    model, xs, labels = _dropout_model(name)
    W = model.head.projection.weight
    D = torch.randn(W.shape, generator=torch.Generator().manual_seed(5)).to(W.device) * float(W.detach().std())
    l0, grads = _train_step(model, xs, labels, 777)
    W0 = W.detach().clone()
    with torch.no_grad():
        W.add_(D)
    l1, _ = _train_step(model, xs, labels, 777, backward=False)
    with torch.no_grad():
        W.copy_(W0)
    l0b, grads_b = _train_step(model, xs, labels, 777)  # the backward at W, after the restore
    assert torch.equal(l0, l0b) and torch.equal(grads["head.projection.weight"], grads_b["head.projection.weight"])
    logits = l0.double().cpu()
    dlogits = torch.softmax(logits, 1)
    dlogits[torch.arange(logits.shape[0]), labels.cpu()] -= 1.0
    dlogits /= logits.shape[0]
    lhs = float((grads_b["head.projection.weight"].double().cpu() * D.double().cpu()).sum())
    rhs = float((dlogits * (l1.double().cpu() - logits)).sum())
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-30)
    print("%-24s <gradW, D> %.9e  <dlogits, logits(W+D) - logits(W)> %.9e  rel %.3e" % (name, lhs, rhs, rel))
    assert lhs != 0.0 and rel < 1e-3, (lhs, rhs, rel)


def test_tired_graph_replayed_train_step_equals_eager_step():
    """bench.make_train_step's closure (zero grads, forward with dropout, cross-entropy, backward, SGD) on the dual
    fixture, captured into a hipGraph and replayed once: the flat gradient, the loss and the logits equal the eager
    step's from the same snapshot bit for bit — the bound of tests/test_graph_train_gpu.py."""
    _need_gpu()
    sys.path.insert(0, ROOT)
    import bench
    from slowfast.models import engine
    try:
        model, sd, z, meta, cfg = build_gray("dual_r18_gray_tired_s64")
        xs = [x.cuda() for x in gray_inputs(meta)]
        labels = torch.from_numpy(z["train/labels"]).cuda()
        with contextlib.redirect_stdout(io.StringIO()):
            step, flat, opt = bench.make_train_step(model, xs, labels, overlap_allreduce=True, lr=0.02)
        assert any(isinstance(m, torch.nn.Dropout) and m.p > 0 for m in model.modules()), "dropout is part of the step"
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):      # momentum buffers, packed-weight caches, allocator pools
                step()
        torch.cuda.synchronize()
        state = [v for _, v in model.named_parameters()] + [v for _, v in model.named_buffers()]
        state += [opt.state[p]["momentum_buffer"] for p in model.parameters()]
        snap = [v.detach().clone() for v in state]

        def restore():
            with torch.no_grad():
                for v, s in zip(state, snap):
                    v.copy_(s)
            torch.cuda.manual_seed(4242)
            torch.cuda.synchronize()

        restore()
        with torch.cuda.stream(side):
            loss = step().detach().clone()
            logits = step.logits.clone()
        torch.cuda.synchronize()
        eager = (flat.flat.detach().clone(), loss, logits)
        assert tuple(logits.shape) == (2, TRAIN_LOGITS)

        restore()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            static_loss = step()
        static_logits = step.logits
        restore()
        with torch.cuda.stream(side):
            g.replay()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(eager[0]).all()) and bool(torch.isfinite(eager[1]).all())
        assert float(eager[0].abs().max()) > 0.0
        assert torch.equal(eager[1], static_loss.detach().reshape(eager[1].shape)), "loss"
        assert torch.equal(eager[2], static_logits), "logits"
        assert torch.equal(eager[0], flat.flat), "flat gradient"
    finally:
        engine.set_grad_sink(False)   # make_train_step switched the in-kernel gradient sink on (process-global)
