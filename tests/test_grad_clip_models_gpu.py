"""One whole training step with gradient clipping between the backward pass and the update — loss -> backward ->
HipGradClip.clip(guard=loss_fun.guard) -> HipSGD.step(guard=clip.guard) — on slow_r18_s64 (one pathway) and
shufflenet_g1_s64 (two).  The reference is numpy float64 on the host from the float32 gradients the kernels read; the
bounds are the op tests' (tests/test_grad_clip_ops_gpu.py): 1e-13 on the norm, 2^-22 |g c| on a scaled gradient."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

import _frozen

pytestmark = pytest.mark.gpu


def _build(name):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta, sd, xs = _frozen.case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    cfg.SOLVER.OPTIMIZING_METHOD, cfg.SOLVER.BASE_LR = "sgd", 0.05
    cfg.SOLVER.MOMENTUM, cfg.SOLVER.NESTEROV, cfg.SOLVER.DAMPENING = 0.9, True, 0.0
    cfg.SOLVER.WEIGHT_DECAY, cfg.BN.WEIGHT_DECAY = 1e-3, 0.0
    cfg.LOG_PERIOD, cfg.TRAIN.TOPK = 1, min(5, cfg.MODEL.NUM_CLASSES)
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    model.load_state_dict(sd, strict=True)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    labels = torch.from_numpy(z["train/labels"]).long().cuda()
    return cfg, model.train(), [x.cuda() for x in xs], labels


def _bits(t):
    return t.detach().view(torch.int32)


def _same_parameters(a, b):
    return all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))


@pytest.mark.parametrize("name", ["slow_r18_s64", "shufflenet_g1_s64"])
def test_training_step_with_clipping(name):
    from slowfast.models.step_tail import HipCrossEntropy, HipGradClip, construct_hip_optimizer
    from slowfast.utils.distributed import FlatGradients
    from slowfast.utils.meters import DeviceTrainMeter
    cfg, model, xs, labels = _build(name)
    _, twin, _, _ = _build(name)
    params, twin_params = list(model.parameters()), list(twin.parameters())
    flat, twin_flat = FlatGradients(params), FlatGradients(twin_params)
    meter = DeviceTrainMeter(10, cfg, grad_norm=True)
    loss_fun = HipCrossEntropy(cfg.TRAIN.TOPK, meter.ring)

    flat.zero()
    meter.iter_tic()
    loss = loss_fun(model(xs), labels)
    loss.backward()
    torch.cuda.synchronize()
    p0 = [p.detach().clone() for p in params]
    g0 = flat.flat.clone()
    g64 = g0.cpu().numpy().astype(np.float64)
    norm = math.sqrt(float(np.sum(g64 * g64)))
    assert math.isfinite(norm) and norm > 0 and _same_parameters(params, twin_params)

    # ---- clip at half the step's norm
    max_norm = float(np.float32(0.5 * norm))
    opt = construct_hip_optimizer(model, cfg)
    clip = HipGradClip(opt.param_groups, max_norm=max_norm, ring=meter.ring)
    clip.clip(guard=loss_fun.guard)
    torch.cuda.synchronize()
    got_norm = float(clip.total_norm64.cpu()[0])
    c = min(1.0, max_norm / (norm + 1e-6))
    want = g64 * c
    err = np.abs(flat.flat.cpu().numpy().astype(np.float64) - want)
    nz = want != 0
    print("%s: %d gradient elements in %d tensors, norm %.9g (rel err %.3e), coefficient %.9g, worst relative error of "
          "a scaled gradient %.3e (bound %.3e)" % (name, g64.size, len(params), got_norm, abs(got_norm - norm) / norm, c,
                                                   float((err[nz] / np.abs(want[nz])).max()), 2.0 ** -22))
    assert abs(got_norm - norm) <= 1e-13 * norm
    assert float(clip.total_norm.cpu()[0]) == float(np.float32(got_norm))
    assert (err <= 2.0 ** -22 * np.abs(want)).all()
    assert float(clip.guard.cpu()[0]) == 0.0
    clipped = flat.flat.clone()
    opt.step(guard=clip.guard)
    # the twin gets the clipped gradients and steps without a clipper
    twin_flat.flat.copy_(clipped)
    construct_hip_optimizer(twin, cfg).step()
    torch.cuda.synchronize()
    assert _same_parameters(params, twin_params)
    assert sum(int(not torch.equal(p.detach(), q)) for p, q in zip(params, p0)) > 0.9 * len(params)

    # ---- the meters: the logged norm is the fp32 norm; the default meter's record has no new key
    meter.iter_toc()
    meter.update_stats(0.05)
    stats = meter.log_iter_stats(0, 0)
    assert stats["grad_norm"] == float(clip.total_norm.cpu()[0])
    plain = DeviceTrainMeter(10, cfg, ring=meter.ring)
    plain.update_stats(0.05)
    plain_stats = plain.log_iter_stats(0, 0)
    assert set(plain_stats) == {"_type", "epoch", "iter", "time_diff", "eta", "loss", "lr", "gpu_mem", "top1_err",
                                "top5_err"} == set(stats) - {"grad_norm"}
    assert plain_stats["loss"] == stats["loss"] == float(loss.detach().cpu())

    # ---- max_norm far above the norm: the step of a loop without a clipper, bit for bit
    with torch.no_grad():
        for p, q, v in zip(params, twin_params, p0):
            p.copy_(v)
            q.copy_(v)
    flat.flat.copy_(g0)
    twin_flat.flat.copy_(g0)
    opt = construct_hip_optimizer(model, cfg)
    clip = HipGradClip(model.parameters(), max_norm=float(np.float32(1000.0 * norm)))
    clip.clip(guard=loss_fun.guard)
    opt.step(guard=clip.guard)
    construct_hip_optimizer(twin, cfg).step(guard=loss_fun.guard)
    torch.cuda.synchronize()
    assert float(clip.coef.cpu()[0]) == 1.0 and torch.equal(_bits(flat.flat), _bits(g0))
    assert _same_parameters(params, twin_params)
    assert sum(int(not torch.equal(p.detach(), q)) for p, q in zip(params, p0)) > 0.9 * len(params)
