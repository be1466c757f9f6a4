"""The multi-label and detection training tails on whole (64^2 golden-size) models: HipBCE behind the detection head's
sigmoid probabilities (slowfast_r50_ava_s64 with boxes), HipBCEWithLogits behind the raw training logits of a
HEAD_ACT-sigmoid / MULTI_LABEL classifier (slow_r18_s64), and HipAdam over every parameter of that model.

The loss plumbing is pinned without a tolerance: `loss.backward()` and `preds.backward(gradient=loss_fun.dlogits)` on an
identical second forward run the same kernels in the same order, so every parameter gradient has equal bits.  HipAdam
is checked against float64 on the CPU with the op tests' bound: what torch's own float32 foreach Adam misses the same
float64 values by, times 2 (figures: profiles/step_tail_multilabel.txt)."""
import contextlib
import io

import pytest
import torch

from _util import case_inputs, load_case, seeded_state_dict

pytestmark = pytest.mark.gpu


def _build(name, **model_cfg):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta = load_case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    for k, v in model_cfg.items():
        setattr(cfg.MODEL, k, v)
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    model.load_state_dict(seeded_state_dict(z["sd_keys"], z["sd_shapes"], meta["param_seed"]), strict=True)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return cfg, model.train(), [x.cuda() for x in case_inputs(meta)], z


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _two_routes(model, forward, loss_fun, targets):
    """Parameter gradients of `loss_fun(preds, targets).backward()` and of `preds.backward(gradient=dlogits)`."""
    params = list(model.parameters())
    preds = forward()
    loss = loss_fun(preds, targets)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss.detach())) and float(loss_fun.guard[0]) == 0.0
    a = [p.grad.detach().clone() for p in params]
    d = loss_fun.dlogits.clone()
    for p in params:
        p.grad = None
    preds = forward()
    preds.backward(gradient=d)
    torch.cuda.synchronize()
    b = [p.grad.detach().clone() for p in params]
    assert all(bool(torch.isfinite(g).all()) for g in a) and sum(float(g.abs().max()) > 0 for g in a) > 0.9 * len(a)
    differ = [n for (n, _), x, y in zip(model.named_parameters(), a, b) if not _same_bits(x, y)]
    assert not differ, differ[:5]
    for p in params:
        p.grad = None
    return preds.detach(), float(loss.detach())


def test_detection_bce_routes_give_equal_gradient_bits():
    from slowfast.models.step_tail import HipBCE, StatsRing, get_hip_loss_func
    cfg, model, xs, z = _build("slowfast_r50_ava_s64")
    boxes = torch.from_numpy(z["boxes"]).cuda()
    labels = torch.from_numpy(z["labels"]).cuda()
    cfg.MODEL.LOSS_FUNC = "bce"
    ring = StatsRing(4)
    loss_fun = get_hip_loss_func(cfg, ring)
    assert type(loss_fun) is HipBCE
    probs, loss = _two_routes(model, lambda: model(xs, boxes), loss_fun, labels)
    assert probs.dim() == 2 and probs.shape == labels.shape and 0.0 <= float(probs.min()) and float(probs.max()) <= 1.0
    # the value is nn.BCELoss's: the reference's own recorded loss, with the detection test's bound
    assert abs(loss - float(z["train/loss"][0])) < 1e-3
    assert int(ring.counter[0]) == 1 and ring.rows[0].tolist()[3:7] == [0.0, float(probs.shape[0]), 0.0, 1.0]


def test_multilabel_bce_logit_routes_and_adam_on_the_whole_model():
    from slowfast.models import engine
    from slowfast.models.step_tail import HipAdam, HipBCEWithLogits, StatsRing, construct_hip_solver, get_hip_loss_func
    cfg, model, xs, z = _build("slow_r18_s64", HEAD_ACT="sigmoid", LOSS_FUNC="bce_logit")
    cfg.DATA.MULTI_LABEL = True
    loss_fun = get_hip_loss_func(cfg, StatsRing(4))
    assert type(loss_fun) is HipBCEWithLogits
    N, K = xs[0].shape[0], cfg.MODEL.NUM_CLASSES
    g = torch.Generator().manual_seed(4)
    targets = (torch.rand(N, K, generator=g) < 0.1).double().cuda()  # multi-hot, float64 as the reference's loader
    logits, loss = _two_routes(model, lambda: model(xs), loss_fun, targets)
    assert tuple(logits.shape) == (N, K)
    ref = float(torch.nn.BCEWithLogitsLoss(reduction="mean")(logits.double().cpu(), targets.cpu()))
    t = float(torch.nn.BCEWithLogitsLoss(reduction="mean")(logits, targets.float()))
    print("multi-label model: loss err %.3e (torch %.3e)" % (abs(loss - ref), abs(t - ref)))
    assert abs(loss - ref) <= 2 * abs(t - ref)

    # ---- HipAdam over every parameter: two steps on seeded gradients against float64 on the CPU
    cfg.SOLVER.OPTIMIZING_METHOD, cfg.SOLVER.BASE_LR = "adam", 1e-3
    cfg.SOLVER.WEIGHT_DECAY, cfg.BN.WEIGHT_DECAY = 1e-3, 0.0
    opt = construct_hip_solver(model, cfg)
    assert isinstance(opt, HipAdam)
    params = list(model.parameters())
    index = {id(p): i for i, p in enumerate(params)}
    grads = [[torch.randn(p.shape, generator=g) * 1e-2 for p in params] for _ in range(2)]

    def reference(dtype, device):
        copies = [torch.nn.Parameter(p.detach().to(device=device, dtype=dtype).clone()) for p in params]
        groups = [{"params": [copies[index[id(p)]] for p in gr["params"]], "weight_decay": gr["weight_decay"]}
                  for gr in opt.param_groups]
        ref = torch.optim.Adam(groups, lr=1e-3, betas=(0.9, 0.999), foreach=(device == "cuda"))
        for s, lr in enumerate((1e-3, 5e-4)):
            for gr in ref.param_groups:
                gr["lr"] = lr
            for c, gg in zip(copies, grads[s]):
                c.grad = gg.to(device=device, dtype=dtype)
            ref.step()
        return copies
    ref64, ref32 = reference(torch.float64, "cpu"), reference(torch.float32, "cuda")
    epoch = engine._PARAM_EPOCH
    for s, lr in enumerate((1e-3, 5e-4)):
        for gr in opt.param_groups:
            gr["lr"] = lr
        for p, gg in zip(params, grads[s]):
            p.grad = gg.cuda()
        opt.step()
    torch.cuda.synchronize()
    assert engine._PARAM_EPOCH == epoch + 2  # the engine's derived weight caches are invalidated
    ep = max(float((p.detach().double().cpu() - r.detach()).abs().max()) for p, r in zip(params, ref64))
    tp = max(float((q.detach().double().cpu() - r.detach()).abs().max()) for q, r in zip(ref32, ref64))
    print("multi-label model: Adam parameter err %.3e (torch %.3e) over %d tensors" % (ep, tp, len(params)))
    assert ep <= 2 * tp
    assert all(float(opt.state[p]["step"]) == 2.0 for p in params) and len(opt._blocks) == 1
    model.eval()
    with torch.no_grad():
        out = model(xs)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (N, K) and bool(torch.isfinite(out).all())
    assert 0.0 <= float(out.min()) and float(out.max()) <= 1.0  # HEAD_ACT sigmoid
