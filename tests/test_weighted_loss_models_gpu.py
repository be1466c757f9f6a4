"""One training step of a whole model with class weights: slow_r18_s64 (the smallest fixture of the model tests),
HipCrossEntropy(weight=[2, 3, 1, 1, ...]) for the loss, HipSGD for the update, DeviceTrainMeter for the statistics.

The parameter gradients are compared with those of the same HIP forward and backward when the gradient handed to the
logits is instead torch.autograd's of F.cross_entropy(weight=...) on the same logits, under the model tests' training
tolerance (tests/test_models_gpu.py: relative L2 below 8e-2 per tensor, 0.3 for tensors of fewer than 16 elements)."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

from _util import case_inputs, load_case, seeded_state_dict

pytestmark = pytest.mark.gpu
NAME = "slow_r18_s64"


def _build():
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta = load_case(NAME)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    model.load_state_dict(seeded_state_dict(z["sd_keys"], z["sd_shapes"], meta["param_seed"]), strict=True)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    labels = torch.from_numpy(z["train/labels"]).long().cuda()
    return cfg, model.train(), [x.cuda() for x in case_inputs(meta)], labels


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_weighted_training_step_guard_and_meter():
    from slowfast.models.step_tail import HipCrossEntropy, construct_hip_optimizer
    from slowfast.utils.meters import DeviceTrainMeter
    cfg, model, xs, labels = _build()
    K = cfg.MODEL.NUM_CLASSES
    cfg.SOLVER.OPTIMIZING_METHOD, cfg.SOLVER.BASE_LR = "sgd", 0.05
    cfg.SOLVER.MOMENTUM, cfg.SOLVER.NESTEROV, cfg.SOLVER.DAMPENING = 0.9, True, 0.0
    cfg.SOLVER.WEIGHT_DECAY, cfg.BN.WEIGHT_DECAY = 1e-3, 0.0
    cfg.LOG_PERIOD, cfg.TRAIN.TOPK = 2, min(5, K)
    params = list(model.parameters())
    names = [n for n, _ in model.named_parameters()]
    opt = construct_hip_optimizer(model, cfg)
    meter = DeviceTrainMeter(10, cfg)
    weight = [2.0, 3.0] + [1.0] * (K - 2)
    for i, l in enumerate(sorted(set(labels.tolist()))):  # the classes of the batch weigh differently from each other
        weight[l] = (2.0, 3.0, 1.5, 0.5)[i % 4]
    loss_fun = HipCrossEntropy(cfg.TRAIN.TOPK, meter.ring, weight=weight)
    w = loss_fun.weight
    assert w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == (K,)

    # ---- the HIP loss's gradient through the model
    preds = model(xs)
    loss = loss_fun(preds, labels)
    loss.backward()
    torch.cuda.synchronize()
    assert float(loss_fun.guard[0]) == 0.0
    hip = [p.grad.detach().clone() for p in params]
    logits = preds.detach()
    ref_loss = float(F.cross_entropy(logits.double().cpu(), labels.cpu(), weight=w.double().cpu()))
    t_loss = float(F.cross_entropy(logits, labels, weight=w))
    e, te = abs(float(loss.detach()) - ref_loss), abs(t_loss - ref_loss)
    print("weighted model step: loss err %.3e (torch %.3e)" % (e, te))
    assert e <= 2 * te
    # the meter folds the weighted row as it folds any cross-entropy row: the loss is the weighted mean
    assert meter.drain() == 1
    assert meter.loss.get_win_median() == float(loss.detach()) and meter.num_samples == labels.shape[0]
    assert meter.loss_total == float(loss.detach()) * labels.shape[0]
    unweighted = float(F.cross_entropy(logits, labels))
    assert abs(unweighted - ref_loss) > 1e-4 * abs(ref_loss)  # the weights matter on this batch

    # ---- the same forward and backward with torch.autograd's gradient of F.cross_entropy(weight=) at the logits
    for p in params:
        p.grad = None
    preds2 = model(xs)
    assert _same_bits(preds2.detach(), logits)
    leaf = logits.clone().requires_grad_(True)
    F.cross_entropy(leaf, labels, weight=w).backward()
    preds2.backward(gradient=leaf.grad)
    torch.cuda.synchronize()
    worst = 0.0
    for n, a, p in zip(names, hip, params):
        b = p.grad.detach()
        err = float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))
        worst = max(worst, err)
        assert err < (0.3 if a.numel() < 16 else 8e-2), (n, err)
    print("weighted model step: worst parameter-gradient L2rel %.3e over %d tensors" % (worst, len(params)))
    assert sum(float(g.abs().max()) > 0 for g in hip) > 0.9 * len(hip)

    # ---- the update, then a step whose weights sum to nothing over the batch: the guard switches the update off
    for p, g in zip(params, hip):
        p.grad = g.clone()
    before = [p.detach().clone() for p in params]
    opt.step(guard=loss_fun.guard)
    torch.cuda.synchronize()
    assert sum(int(not torch.equal(p.detach(), q)) for p, q in zip(params, before)) > 0.9 * len(params)
    zero = w.clone()
    zero[labels] = 0.0
    loss_fun.set_weight(zero)
    for p in params:
        p.grad = None
    preds = model(xs)
    loss = loss_fun(preds, labels)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss.detach())) and float(loss_fun.guard[0]) == 1.0
    assert bool((loss_fun.dlogits.view(torch.int32) == 0).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)  # no NaN reached a gradient
    before = [p.detach().clone() for p in params]
    moms = [opt.state[p]["momentum_buffer"].clone() for p in params]
    opt.step(guard=loss_fun.guard)
    torch.cuda.synchronize()
    assert all(_same_bits(p.detach(), q) for p, q in zip(params, before))
    assert all(_same_bits(opt.state[p]["momentum_buffer"], m) for p, m in zip(params, moms))

    # ---- the ring: both rows are cross-entropy rows; the second carries the flag, which the meter reports as the
    # reference's check_nan_losses does
    rows = meter.ring.rows.cpu()
    assert int(meter.ring.counter[0]) == 2 and rows[:, 6].tolist() == [0.0, 0.0]
    assert float(rows[0, 3]) == 0.0 and float(rows[1, 3]) == 1.0 and bool(torch.isnan(rows[1, 0]))
    with pytest.raises(RuntimeWarning, match="NaN losses"):
        meter.drain()
