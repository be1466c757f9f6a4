"""HipAveragedModel on whole models (slow_r18_s64, the smallest fixture): parity with torch's AveragedModel over three
HipSGD training steps, evaluation on the averaged weights through the model's own caches, a captured training step with
the update inside it, and the precise-BN pass on the same native call (once more on dual_r50_subbn_s64, whose
SubBatchNorm3d layers contribute `bn` and `split_bn`).

The training step is bench.make_train_step's form (zero the flat gradients, forward, loss, backward, optimizer step,
rebind) on the step-tail objects, so that the loss's guard reaches the optimizer and the averaging call."""
import contextlib
import io

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

import _frozen

pytestmark = pytest.mark.gpu
NAME = "slow_r18_s64"


def _build(name, gpus=1):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta, sd, xs = _frozen.case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = gpus
    cfg.SOLVER.OPTIMIZING_METHOD, cfg.SOLVER.BASE_LR = "sgd", 0.05
    cfg.SOLVER.MOMENTUM, cfg.SOLVER.NESTEROV, cfg.SOLVER.DAMPENING = 0.9, True, 0.0
    cfg.SOLVER.WEIGHT_DECAY, cfg.BN.WEIGHT_DECAY = 1e-3, 0.0
    cfg.TRAIN.TOPK = min(5, cfg.MODEL.NUM_CLASSES)
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    model.load_state_dict(sd, strict=True)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    labels = torch.from_numpy(z["train/labels"]).long()
    if gpus:
        return cfg, model.train(), [x.cuda() for x in xs], labels.cuda()
    return cfg, model.train(), xs, labels


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def make_train_step(cfg, model, xs, labels, ema=None):
    from slowfast.models.step_tail import HipCrossEntropy, StatsRing, construct_hip_optimizer
    from slowfast.utils.distributed import FlatGradients
    flat = FlatGradients(list(model.parameters()))
    opt = construct_hip_optimizer(model, cfg)
    loss_fun = HipCrossEntropy(cfg.TRAIN.TOPK, StatsRing(8))

    def step():
        flat.zero()
        loss = loss_fun(model(xs), labels)
        loss.backward()
        opt.step(guard=loss_fun.guard)
        flat.rebind()
        if ema is not None:
            ema.update_parameters(guard=loss_fun.guard)
        return loss

    return step, flat, opt, loss_fun


def _model_state(model, opt):
    state = [("p/" + k, v) for k, v in model.named_parameters()] + [("b/" + k, v) for k, v in model.named_buffers()]
    for i, p in enumerate(model.parameters()):
        state.append(("m/%d" % i, opt.state[p]["momentum_buffer"]))
    return state


def test_three_training_steps_match_torchs_averaged_model():
    from slowfast.models.weight_avg import HipAveragedModel
    decay = 0.9
    cfg, model, xs, labels = _build(NAME)
    ema = HipAveragedModel(model, decay=decay, use_buffers=True)
    step, flat, opt, loss_fun = make_train_step(cfg, model, xs, labels, ema)
    snaps = []
    for _ in range(3):
        step()
        snaps.append({k: v.detach().clone() for k, v in model.state_dict().items()})
    torch.cuda.synchronize()
    assert float(loss_fun.guard[0]) == 0.0 and int(ema.n_averaged) == 3

    def torch_run(feeder):
        avg = AveragedModel(feeder, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True)
        for snap in snaps:
            feeder.load_state_dict({k: v.to(next(feeder.parameters()).dtype) if v.is_floating_point() else v
                                    for k, v in snap.items()})
            avg.update_parameters(feeder)
        return {k: v.detach().double().cpu() for k, v in avg.module.state_dict().items()}

    ref = torch_run(_build(NAME, gpus=0)[1].double())
    own = torch_run(_build(NAME)[1])
    e = t = 0.0
    floats = 0
    for k, v in ema.averaged.items():
        if v.dtype != torch.float32:
            assert k.endswith("num_batches_tracked") and torch.equal(v, model.state_dict()[k]), k
            continue
        floats += 1
        e = max(e, float((v.double().cpu() - ref[k]).abs().max()))
        t = max(t, float((own[k] - ref[k]).abs().max()))
    print("%s: %d averaged float tensors after 3 steps, err %.3e (torch's float32 foreach run %.3e)" % (NAME, floats, e, t))
    assert floats > 40 and t > 0.0 and e <= 2 * t
    moved = sum(int(not torch.equal(ema.averaged[k], snaps[-1][k])) for k, _ in model.named_parameters())
    assert moved > 0.9 * len(list(model.parameters()))  # an average, not the last weights


def test_evaluation_on_the_averaged_weights_and_back():
    from slowfast.models.weight_avg import HipAveragedModel
    cfg, model, xs, labels = _build(NAME)
    ema = HipAveragedModel(model, decay=0.5)
    step, flat, opt, loss_fun = make_train_step(cfg, model, xs, labels, ema)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    state = _model_state(model, opt)
    snap = [v.detach().clone() for _, v in state]
    averaged = {k[len("module."):]: v.clone() for k, v in ema.state_dict().items() if k != "n_averaged"}

    model.eval()
    with torch.no_grad():
        base = model(xs).clone()  # the model's eval caches (packed weights, folded BN) now hold the TRAINED weights
        with ema.applied():
            got = model(xs).clone()
            assert all(_same(v, averaged[k]) for k, v in model.state_dict().items())
        after = model(xs).clone()
    twin = _build(NAME)[1]
    twin.load_state_dict(averaged, strict=True)
    twin.eval()
    with torch.no_grad():
        want = twin(xs).clone()
    torch.cuda.synchronize()
    assert _same(got, want) and not _same(got, base)
    assert _same(after, base)
    assert all(_same(v, s) for (_, v), s in zip(state, snap))  # every bit is back
    assert all(_same(v, averaged[k]) for k, v in ema.averaged.items())

    # the next training step equals the one of a run that never swapped
    model.train()
    step()
    torch.cuda.synchronize()
    swapped = [v.detach().clone() for _, v in state]
    with torch.no_grad():
        for (_, v), s in zip(state, snap):
            v.copy_(s)
    step()
    torch.cuda.synchronize()
    for (k, v), s in zip(state, swapped):
        assert _same(v, s), k
    assert sum(int(not _same(a, b)) for a, b in zip(swapped, snap)) > 0.9 * len(snap)

    # copy_to_model / reset_from_model
    ema.copy_to_model()
    assert all(_same(v, ema.averaged[k]) for k, v in model.state_dict().items())
    with torch.no_grad():
        for (_, v), s in zip(state, snap):
            v.copy_(s)
    ema.reset_from_model()
    torch.cuda.synchronize()
    assert all(_same(v, ema.averaged[k]) for k, v in model.state_dict().items())


def test_a_captured_step_with_the_update_follows_set_decay():
    from slowfast.models import engine
    from slowfast.models.weight_avg import HipAveragedModel
    cfg, model, xs, labels = _build(NAME)
    ema = HipAveragedModel(model, decay=0.5)
    step, flat, opt, loss_fun = make_train_step(cfg, model, xs, labels, ema)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(3):  # optimizer state, address tables, packed-weight caches, allocator pools
            step()
    torch.cuda.synchronize()
    state = _model_state(model, opt) + [("ema/float", ema._block), ("ema/words", ema._words), ("ema/n", ema.n_averaged)]
    snap = [v.detach().clone() for _, v in state]
    decays = (0.9, 0.99)

    def restore():
        with torch.no_grad():
            for (_, v), s in zip(state, snap):
                v.copy_(s)
        torch.cuda.synchronize()

    with torch.cuda.stream(side):
        for d in decays:
            ema.set_decay(d)
            step()
    torch.cuda.synchronize()
    eager = [v.detach().clone() for _, v in state]
    assert int(ema.n_averaged) == 5 and float(loss_fun.guard[0]) == 0.0
    assert not _same(eager[-3], snap[-3])

    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    restore()
    with torch.cuda.stream(side):
        for d in decays:
            assert ema.set_decay(d)
            engine.replay(graph)
    torch.cuda.synchronize()
    for (k, v), e in zip(state, eager):
        assert _same(v, e), k


@pytest.mark.parametrize("name", [NAME, "dual_r50_subbn_s64"])
def test_precise_bn_pass_equals_the_torch_loop_bit_for_bit(name):
    """update_bn_stats against the loop it replaced, restated on torch ops from the per-iteration statistics:
    mean += (running - mean) / (k + 1) per layer on the GPU."""
    from slowfast.utils.precise_bn import get_bn_modules, update_bn_stats
    cfg, model, xs, labels = _build(name)
    batches = [[x * s for x in xs] for s in (1.0, 0.7, 1.3)]
    layers = get_bn_modules(model)
    assert len(layers) == sum(isinstance(m, torch.nn.BatchNorm3d) for m in model.modules()) > 0
    if name != NAME:
        assert any(n.endswith("split_bn") for n, m in model.named_modules() if m in layers)
    momenta = [bn.momentum for bn in layers]
    for bn in layers:
        bn.momentum = 1.0
    mean = [torch.zeros_like(bn.running_mean) for bn in layers]
    var = [torch.zeros_like(bn.running_var) for bn in layers]
    with torch.no_grad():
        for k, b in enumerate(batches):
            model(b)
            for i, bn in enumerate(layers):
                mean[i] += (bn.running_mean - mean[i]) / (k + 1)
                var[i] += (bn.running_var - var[i]) / (k + 1)
    for bn, m in zip(layers, momenta):
        bn.momentum = m
    addresses = [bn.running_mean.data_ptr() for bn in layers]
    update_bn_stats(model, iter(batches), num_iters=3)
    torch.cuda.synchronize()
    assert [bn.momentum for bn in layers] == momenta
    assert [bn.running_mean.data_ptr() for bn in layers] == addresses  # written in place
    for i, bn in enumerate(layers):
        assert _same(bn.running_mean, mean[i]) and _same(bn.running_var, var[i]), i
    with pytest.raises(AssertionError):
        update_bn_stats(model, iter(batches[:1]), num_iters=2)  # loader shorter than num_iters
