"""One whole training step with the tail on libsfhip kernels: model forward and taped backward into FlatGradients,
HipCrossEntropy for the loss, HipSGD for the update, DeviceTrainMeter for the statistics — on shufflenetv2_cfg1, the
smallest two-pathway fixture of the model tests.  The loss and the update are checked against float64 on the CPU with
the op tests' bound: what torch's own float32 GPU kernel misses the same float64 values by, on the same inputs, times 2.
Measured on an MI355X (profiles/step_tail.txt): loss 4.1e-8 (torch 4.1e-8), parameters over 390 tensors 1.1e-7
(torch 1.1e-7)."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _frozen

pytestmark = pytest.mark.gpu
NAME = "shufflenetv2_cfg1"


def _build():
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta, sd, xs = _frozen.case(NAME)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    model.load_state_dict(sd, strict=True)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    labels = torch.from_numpy(z["train/labels"]).long().cuda()
    return cfg, model.train(), [x.cuda() for x in xs], labels


def _sgd_reference(opt, params, p0, g0, dtype, device):
    """torch.optim.SGD with `opt`'s groups on copies of the parameters / gradients from before the update."""
    index = {id(p): i for i, p in enumerate(params)}
    copies = [torch.nn.Parameter(p.to(device=device, dtype=dtype).clone()) for p in p0]
    for c, g in zip(copies, g0):
        c.grad = g.to(device=device, dtype=dtype).clone()
    groups = []
    for g in opt.param_groups:
        d = {k: v for k, v in g.items() if k not in ("params", "foreach", "fused")}
        d["params"] = [copies[index[id(p)]] for p in g["params"]]
        groups.append(d)
    ref = torch.optim.SGD(groups, lr=0.1, foreach=(device == "cuda"))
    ref.step()
    return copies


def test_training_step_through_the_hip_tail():
    from slowfast.models import engine
    from slowfast.models.step_tail import HipCrossEntropy, construct_hip_optimizer
    from slowfast.utils.distributed import FlatGradients
    from slowfast.utils.meters import DeviceTrainMeter, _ScalarWindow
    cfg, model, xs, labels = _build()
    cfg.SOLVER.OPTIMIZING_METHOD, cfg.SOLVER.BASE_LR = "sgd", 0.05
    cfg.SOLVER.MOMENTUM, cfg.SOLVER.NESTEROV, cfg.SOLVER.DAMPENING = 0.9, True, 0.0
    cfg.SOLVER.WEIGHT_DECAY, cfg.BN.WEIGHT_DECAY = 1e-3, 0.0
    cfg.LOG_PERIOD, cfg.TRAIN.TOPK = 2, min(5, cfg.MODEL.NUM_CLASSES)
    params = list(model.parameters())
    flat = FlatGradients(params)
    opt = construct_hip_optimizer(model, cfg)
    meter = DeviceTrainMeter(10, cfg)
    assert meter.ring.cap == 2
    loss_fun = HipCrossEntropy(cfg.TRAIN.TOPK, meter.ring)

    def forward_backward():
        flat.zero()
        preds = model(xs)
        loss = loss_fun(preds, labels)
        loss.backward()
        return preds.detach(), loss

    # ---- one step, checked piece by piece
    preds, loss = forward_backward()
    torch.cuda.synchronize()
    p0 = [p.detach().clone() for p in params]
    g0 = [p.grad.detach().clone() for p in params]
    assert bool(torch.isfinite(flat.flat).all()) and float(flat.flat.abs().max()) > 0
    ref_loss = float(F.cross_entropy(preds.double().cpu(), labels.cpu()))
    t_loss = float(F.cross_entropy(preds, labels))
    e, te = abs(float(loss.detach()) - ref_loss), abs(t_loss - ref_loss)
    print("model step: loss err %.3e (torch %.3e)" % (e, te))
    assert e <= 2 * te
    epoch = engine._PARAM_EPOCH
    opt.step(guard=loss_fun.guard)
    torch.cuda.synchronize()
    assert engine._PARAM_EPOCH > epoch
    ref64 = _sgd_reference(opt, params, p0, g0, torch.float64, "cpu")
    ref32 = _sgd_reference(opt, params, p0, g0, torch.float32, "cuda")
    ep = max(float((p.detach().double().cpu() - r.detach()).abs().max()) for p, r in zip(params, ref64))
    tp = max(float((t.detach().double().cpu() - r.detach()).abs().max()) for t, r in zip(ref32, ref64))
    print("model step: parameter err %.3e (torch %.3e) over %d tensors" % (ep, tp, len(params)))
    assert ep <= 2 * tp
    assert sum(int(not torch.equal(p.detach(), q)) for p, q in zip(params, p0)) > 0.9 * len(params)
    # gradients still live in the flat buffer (the optimizer read them there)
    off = 0
    for p in params:
        assert p.grad.data_ptr() == flat.flat.data_ptr() + 4 * off
        off += p.numel()

    # ---- LOG_PERIOD = 2 more steps through the meter (the ring holds step 0 too: drain it first)
    assert meter.drain() == 1
    meter.reset()
    seen = []
    stats = None
    meter.iter_tic()
    for it in range(2):
        lr = 0.05 * (0.5 ** it)
        for g in opt.param_groups:
            g["lr"] = lr
        preds, loss = forward_backward()
        opt.step(guard=loss_fun.guard)
        # the reference's route, read back one by one (tools/train_net.py:122-138)
        _, inds = torch.topk(preds, cfg.TRAIN.TOPK, dim=1, largest=True, sorted=True)
        correct = inds.t().eq(labels.view(1, -1).expand(cfg.TRAIN.TOPK, -1))
        errs = [(1.0 - correct[:k, :].reshape(-1).float().sum() / preds.size(0)) * 100.0 for k in (1, cfg.TRAIN.TOPK)]
        seen.append((errs[0].item(), errs[1].item(), meter.ring.rows[(it + 1) % 2, 0].item(), lr, preds.size(0)))
        meter.iter_toc()
        meter.update_stats(lr)
        stats = meter.log_iter_stats(0, it)
        meter.iter_tic()
    assert stats is not None and stats["_type"] == "train_iter" and stats["iter"] == "2/10"
    want = [_ScalarWindow(2) for _ in range(3)]
    for t1, t5, ls, lr, n in seen:
        want[0].add_value(ls)
        want[1].add_value(t1)
        want[2].add_value(t5)
    assert stats["loss"] == np.median([s[2] for s in seen]) == want[0].get_win_median()
    assert stats["top1_err"] == want[1].get_win_median() and stats["top5_err"] == want[2].get_win_median()
    assert stats["lr"] == seen[-1][3]
    ep_stats = meter.log_epoch_stats(0)
    n = sum(s[4] for s in seen)
    assert ep_stats["loss"] == sum(s[2] * s[4] for s in seen) / n
    assert ep_stats["top1_err"] == sum(s[0] * s[4] for s in seen) / n
    assert ep_stats["top5_err"] == sum(s[1] * s[4] for s in seen) / n
    assert all(np.isfinite(s[2]) for s in seen) and seen[0][2] != seen[1][2]
