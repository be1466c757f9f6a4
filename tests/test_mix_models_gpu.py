"""One training step with soft targets end to end on shufflenetv2_cfg1, the smallest two-pathway fixture of the model
tests: gpu_train_batch_mix (mixup inside the one-launch input step) -> model -> HipCrossEntropy(label_smoothing=0.1) on
the batch's mix rows -> backward -> HipSGD.step(guard=) -> DeviceTrainMeter.  The loss is checked against float64 on the
CPU (tests/_mix_ref.py) with the op tests' bound: what torch's own float32 GPU F.cross_entropy(preds, t_dense) misses the
same float64 value by, times 2."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _frozen
import _mix_ref as ref

pytestmark = pytest.mark.gpu
NAME = "shufflenetv2_cfg1"


def test_training_step_with_mixup_and_label_smoothing():
    from slowfast.config.defaults import get_cfg
    from slowfast.datasets import utils as ds
    from slowfast.models import build_model
    from slowfast.models.step_tail import HipCrossEntropy, construct_hip_optimizer
    from slowfast.utils.distributed import FlatGradients
    from slowfast.utils.meters import DeviceTrainMeter
    z, meta, sd, xs = _frozen.case(NAME)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    cfg.SOLVER.OPTIMIZING_METHOD, cfg.SOLVER.BASE_LR, cfg.SOLVER.MOMENTUM = "sgd", 0.05, 0.9
    cfg.LOG_PERIOD, cfg.TRAIN.TOPK = 2, min(5, cfg.MODEL.NUM_CLASSES)
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    model.load_state_dict(sd, strict=True)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.train()
    labels = torch.from_numpy(z["train/labels"]).long().cuda()
    B, K = labels.numel(), cfg.MODEL.NUM_CLASSES
    crop, t = xs[1].shape[3], xs[1].shape[2]
    assert xs[1].shape[0] == B

    # the batch: B decoded spans of their own sizes, upstream's mix decision (mixup only, always), one launch
    rs = np.random.RandomState(4)
    videos = [torch.from_numpy(rs.randint(0, 256, (t + b, crop + 9 + b, crop + 17, 3)).astype(np.uint8)).cuda()
              for b in range(B)]
    np.random.seed(9)
    samples = [(torch.arange(t) + b, ds.sample_spatial_params(crop + 9 + b, crop + 17, -1, crop, crop + 12, crop))
               for b in range(B)]
    mix = ds.sample_mix_params(B, crop, mixup_alpha=0.8, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5)
    assert mix.mode == ds.MIX_MIXUP and 0.0 < mix.lam < 1.0
    ph, pw, wp = ds.stem_input_geometry(model, crop)
    packed, rows = ds.gpu_train_batch_mix(videos, samples, mix, cfg.DATA.MEAN, cfg.DATA.STD, cfg.SLOWFAST.ALPHA,
                                          pad=(ph, pw), wp=wp)
    plain = ds.gpu_train_batch(videos, samples, cfg.DATA.MEAN, cfg.DATA.STD, cfg.SLOWFAST.ALPHA, pad=(ph, pw), wp=wp)
    assert not torch.equal(packed[1].buf, plain[1].buf)  # the clips were mixed

    params = list(model.parameters())
    flat = FlatGradients(params)
    opt = construct_hip_optimizer(model, cfg)
    meter = DeviceTrainMeter(10, cfg)
    loss_fun = HipCrossEntropy(cfg.TRAIN.TOPK, meter.ring, label_smoothing=0.1)
    flat.zero()
    preds = model(list(packed))
    preds.retain_grad()
    loss = loss_fun(preds, labels, mix=rows)
    loss.backward()
    torch.cuda.synchronize()

    # the logits' gradient is the kernel's, and loss / gradient are the float64 restatement's
    assert preds.grad is not None and torch.equal(preds.grad.view(torch.int32), loss_fun.dlogits.view(torch.int32))
    eps = float(np.float32(0.1))
    host_rows = rows.mix_host.numpy()
    want, want_d, bad = ref.ce_mix(preds.detach().double().cpu().numpy(), labels.cpu().numpy(), host_rows, eps)
    assert bad == 0
    t64 = torch.from_numpy(ref.dense_targets(labels.cpu().numpy(), host_rows, K, eps))
    t_loss = float(F.cross_entropy(preds.detach(), t64.float().cuda()))
    e, te = abs(float(loss.detach()) - want), abs(t_loss - want)
    print("mix model step: loss err %.3e (torch %.3e)" % (e, te))
    assert e <= 2 * te
    assert float(np.abs(loss_fun.dlogits.double().cpu().numpy() - want_d).max()) <= 1e-7
    assert float(loss_fun.guard[0]) == 0.0
    assert bool(torch.isfinite(flat.flat).all()) and float(flat.flat.abs().max()) > 0

    # the parameters move, and the meter drains the step's row
    p0 = [p.detach().clone() for p in params]
    opt.step(guard=loss_fun.guard)
    torch.cuda.synchronize()
    assert sum(int(not torch.equal(p.detach(), q)) for p, q in zip(params, p0)) > 0.9 * len(params)
    row = meter.ring.rows[0].tolist()
    assert row[0] == float(loss.detach()) and row[3] == 0.0 and row[4] == B and row[5] == 0.0 and row[6] == 0.0
    h1, hk = ref.hit_counts(preds.detach().cpu().numpy(), labels.cpu().numpy(), host_rows, cfg.TRAIN.TOPK)
    assert row[1] == float((1.0 - torch.tensor(float(h1)) / B) * 100.0)
    assert row[2] == float((1.0 - torch.tensor(float(hk)) / B) * 100.0)
    assert meter.drain() == 1
