"""Whole training steps with construct_hip_solver's "adamw" and SOLVER.LARS_ON optimizers — model forward, taped backward
into FlatGradients, HipCrossEntropy, then HipAdamW / HipLARS with the loss's guard — on shufflenetv2_cfg1, the smallest
two-pathway fixture of the step-tail model tests.  Three eager steps under a changing learning rate, then the same three
as replays of ONE captured step (eager warm-up first, the learning rate a device-side write between replays): every
parameter, buffer, optimizer state tensor and ring row must have equal bits."""
import contextlib
import io

import pytest
import torch

import _frozen

pytestmark = pytest.mark.gpu
NAME = "shufflenetv2_cfg1"


def _build(kind):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta, sd, xs = _frozen.case(NAME)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    cfg.SOLVER.WEIGHT_DECAY, cfg.BN.WEIGHT_DECAY = 1e-3, 0.0
    cfg.TRAIN.TOPK = min(5, cfg.MODEL.NUM_CLASSES)
    if kind == "adamw":
        cfg.SOLVER.OPTIMIZING_METHOD, cfg.SOLVER.BASE_LR = "adamw", 1e-3
    else:
        cfg.SOLVER.OPTIMIZING_METHOD, cfg.SOLVER.BASE_LR, cfg.SOLVER.LARS_ON = "sgd", 0.05, True
        cfg.SOLVER.MOMENTUM, cfg.SOLVER.NESTEROV, cfg.SOLVER.DAMPENING = 0.9, True, 0.0
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    model.load_state_dict(sd, strict=True)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    labels = torch.from_numpy(z["train/labels"]).long().cuda()
    return cfg, model.train(), [x.cuda() for x in xs], labels


@pytest.mark.parametrize("kind", ["adamw", "lars"])
def test_eager_steps_train_and_a_replayed_step_follows_the_lr_schedule(kind):
    from slowfast.models import engine
    from slowfast.models.step_tail import HipAdamW, HipCrossEntropy, HipLARS, StatsRing, construct_hip_solver
    from slowfast.utils.distributed import FlatGradients
    cfg, model, xs, labels = _build(kind)
    params = list(model.parameters())
    flat = FlatGradients(params)
    opt = construct_hip_solver(model, cfg)
    assert type(opt) is (HipAdamW if kind == "adamw" else HipLARS)
    ring = StatsRing(8)
    loss_fun = HipCrossEntropy(cfg.TRAIN.TOPK, ring)
    base = cfg.SOLVER.BASE_LR
    lrs = (base, base * 0.5, base * 2.0)

    def step():
        flat.zero()
        loss = loss_fun(model(xs), labels)
        loss.backward()
        opt.step(guard=loss_fun.guard)
        flat.rebind()

    def set_lr(lr):
        for g in opt.param_groups:
            g["lr"] = lr

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(3):  # optimizer state, address tables, packed-weight caches, allocator pools
            step()
    torch.cuda.synchronize()
    state = [("p/" + k, v) for k, v in model.named_parameters()] + [("b/" + k, v) for k, v in model.named_buffers()]
    for i, p in enumerate(params):
        state += [("s/%d/%s" % (i, k), v) for k, v in opt.state[p].items()]
    state += [("ring", ring.rows), ("counter", ring.counter)]
    assert sum(1 for k, _ in state if k.startswith("s/")) == len(params) * (3 if kind == "adamw" else 1)
    snap = [v.detach().clone() for _, v in state]
    assert int(ring.counter[0]) == 3

    def restore():
        with torch.no_grad():
            for (_, v), s in zip(state, snap):
                v.copy_(s)
        torch.cuda.synchronize()

    # ---- three eager steps: the loss stays finite, the ring rows advance, the model moves
    with torch.cuda.stream(side):
        for lr in lrs:
            set_lr(lr)
            step()
    torch.cuda.synchronize()
    eager = [v.detach().clone() for _, v in state]
    assert int(ring.counter[0]) == 6 and float(loss_fun.guard[0]) == 0.0
    losses = ring.rows[3:6, 0].tolist()
    print("%s: losses of the three steps %s" % (kind, losses))
    assert all(torch.isfinite(torch.tensor(losses))) and len(set(losses)) == 3 and ring.rows[3:6, 3].tolist() == [0.0] * 3
    moved = sum(int(not torch.equal(a, s)) for (k, _), a, s in zip(state, eager, snap) if k.startswith("p/"))
    assert moved > 0.9 * len(params)
    if kind == "lars":
        n_bn = len(opt.param_groups[0]["params"])
        r = opt.ratios[:, 0]
        assert bool((r[:n_bn] == 1.0).all()) and bool((r[n_bn:] != 1.0).any())  # the BN group does not apply LARS
        assert float(opt.guard[0]) == 0.0
    else:
        assert all(float(opt.state[p]["step"]) == 6.0 for p in params)

    # ---- the same three steps as replays of one captured step; the lr is a device-side write between replays
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    restore()
    with torch.cuda.stream(side):
        for lr in lrs:
            set_lr(lr)
            assert opt.upload_hyper()
            engine.replay(graph)
    torch.cuda.synchronize()
    for (k, v), e in zip(state, eager):
        assert torch.equal(v.detach().view(torch.int32) if v.dtype == torch.float32 else v.detach(),
                           e.view(torch.int32) if e.dtype == torch.float32 else e), k
