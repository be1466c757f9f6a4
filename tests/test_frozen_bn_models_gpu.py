"""Training through frozen (eval-mode) BatchNorm layers on whole models: model.train(); misc.frozen_bn_stats(model); one
step of cross-entropy on the fixture's labels.

Reference: the oracle's eval forward with the parameters as autograd leaves (tests/_frozen.py), once in float64 and once
in float32.  Per parameter, as relative L2:
    err(HIP, oracle fp64) <= max(1e-3, 4 x err(oracle fp32, oracle fp64))
— the rule of tests/test_gradcam_models_gpu.py.  Parameters whose fp64 gradient norm is below 1e-6 of the largest (the
SpatialAttention key biases; tests/test_frozen_bn_args_cpu.py holds the list by the oracle alone) are bounded absolutely:
|g_HIP| <= 1e-5 of the largest gradient norm.  The logits must match the fixture's eval logits (1e-3 max-norm relative,
TOL of test_gradcam_models_gpu.py) and every BN buffer must keep its bits.

Observed on an MI355X, worst parameter per fixture as (HIP vs fp64, oracle fp32 vs fp64) — every run appends its values
to models_report.txt through _report:
    slow_r18_s64          s1.pathway0_stem.conv.weight                        6.1e-7 / 9.2e-7   (median HIP 2.8e-7)
    dual_r50_s64          s3.pathway1_res1.branch2.a_bn.weight                3.6e-4 / 3.5e-4   (median HIP 4.4e-5)
    dual_r50_subbn_s64    s2.pathway1_res1.branch2.c.weight                   1.8e-4 / 2.3e-4   (median HIP 2.1e-5)
    shufflenet_w2_g3_s64  s3_fuse.attention_spatial_s2f.key_conv.weight       5.4e-4 / 2.9e-4   (median HIP 2.5e-4)
    ghostnet_w2_s64       s2_fuse.bn_s2f.weight                               3.2e-4 / 2.1e-4   (median HIP 3.1e-5)
    shufflenetv2_cfg1     s3.pathway1_channel_8.features.0.banch1.1.bias      1.3e-5 / 1.4e-5   (median HIP 3.3e-7)
    mobilenetv2_w1_s64    s3_fuse.attention_spatial_s2f.query_conv.weight     3.6e-6 / 9.8e-7   (median HIP 4.8e-7)
("worst" = largest ratio of the HIP error to its bound; every one is below the 1e-3 floor of the rule.)"""
import contextlib
import io
import os
import sys

import pytest
import torch

import _frozen
from _util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3  # test_gradcam_models_gpu.py::TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(line):
    from test_gradcam_models_gpu import _report as report
    report(line)


def _build(name):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta, sd, xs = _frozen.case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    missing = model.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def _freeze(model, only=None):
    """model.train(); misc.frozen_bn_stats — on the whole model, or on the top-level children named in `only`; Sub-BN
    wrappers follow their inner layers into eval()."""
    from slowfast.models.batchnorm_helper import SubBatchNorm3d
    from slowfast.utils import misc
    model.train()
    roots = [model] if only is None else [m for n, m in model.named_children() if n in only]
    for r in roots:
        misc.frozen_bn_stats(r)
        for m in r.modules():
            if isinstance(m, SubBatchNorm3d):
                m.eval()
    return model


def _step(model, name):
    z, meta, sd, xs = _frozen.case(name)
    labels = torch.from_numpy(z["train/labels"]).long().cuda()
    model.zero_grad(set_to_none=True)
    logits = model([x.cuda() for x in xs])
    torch.nn.functional.cross_entropy(logits, labels).backward()
    torch.cuda.synchronize()
    return logits.detach()


def _buffers(model):
    return {k: v.detach().clone() for k, v in model.named_buffers()}


@pytest.mark.parametrize("name", _frozen.FIXTURES)
def test_frozen_step_matches_the_oracle_and_leaves_the_statistics(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    z, meta, sd, xs = _frozen.case(name)
    model = _freeze(_build(name))
    before = _buffers(model)
    logits = _step(model, name)
    assert model.training and not any(m.training for m in model.modules() if isinstance(m, torch.nn.BatchNorm3d))
    # forward: the running statistics were used
    e_log = rel_err(logits.reshape(meta["batch"], -1).cpu().numpy(), z["eval/logits_full"])
    _report("%-22s frozen-bn logits %.3e" % (name, e_log))
    assert e_log < TOL, e_log
    # no BN buffer moved (running_mean, running_var, num_batches_tracked)
    after = _buffers(model)
    assert before and all(torch.equal(before[k], after[k]) for k in before)
    # gradients
    g64, _ = _frozen.oracle_grads(name, torch.float64)
    g32, _ = _frozen.oracle_grads(name, torch.float32)
    tiny = set(_frozen.tiny_parameters(name))
    top = max(float(g.norm()) for g in g64.values())
    params = dict(model.named_parameters())
    assert set(params) == set(g64)
    worst, failures, ratios = (0.0, 0.0, 0.0, ""), [], []
    for k, p in params.items():
        assert p.grad is not None, k
        g = p.grad.detach().double().cpu().reshape(g64[k].shape)
        assert bool(torch.isfinite(g).all()), k
        if k in tiny:
            a = float(g.norm())
            _report("%-22s frozen-bn tiny %-50s |g| %.3e of top %.3e" % (name, k, a, top))
            if a > 1e-5 * top:
                failures.append((k, "tiny", a, top))
            continue
        ref = g64[k]
        e_hip = float((g - ref).norm() / ref.norm())
        e_ref = float((g32[k] - ref).norm() / ref.norm())
        bound = max(1e-3, 4.0 * e_ref)
        ratios.append(e_hip)
        if e_hip / bound > worst[0]:
            worst = (e_hip / bound, e_hip, e_ref, k)
        if e_hip > bound:
            failures.append((k, e_hip, e_ref))
    ratios.sort()
    line = "%-22s frozen-bn grads: median HIP %.3e, worst against its bound %s: HIP %.3e, oracle fp32 %.3e" % (
        name, ratios[len(ratios) // 2], worst[3], worst[1], worst[2])
    _report(line)
    print(line)
    assert not failures, failures


def test_mixed_frozen_and_training_layers():
    """Only the BNs of s1 .. s3 (and their fusions) frozen: those keep their buffers, the others update theirs."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    name = "dual_r50_s64"
    frozen = ("s1", "s1_fuse", "s2", "s2_fuse", "s3", "s3_fuse")
    model = _freeze(_build(name), only=frozen)
    bns = [(n, m) for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm3d)]
    assert any(m.training for _, m in bns) and any(not m.training for _, m in bns)
    before = _buffers(model)
    _step(model, name)
    after = _buffers(model)
    kept = moved = 0
    for k in before:
        if k.rsplit(".", 1)[-1] not in ("running_mean", "running_var", "num_batches_tracked"):
            continue
        if k.split(".")[0] in frozen:
            assert torch.equal(before[k], after[k]), k
            kept += 1
        else:
            assert not torch.equal(before[k], after[k]), k
            moved += 1
    assert kept > 0 and moved > 0
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


def test_train_step_and_eval_forward_keep_their_bits_around_a_frozen_step():
    """A plain eval forward and a fully train-mode step give the same bits before and after a frozen-BN step, which also
    repeats bit for bit; with the gradient sink the frozen step gives the bits it gives without."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from slowfast.models import engine
    name = "dual_r50_s64"
    z, meta, sd, xs = _frozen.case(name)
    model = _build(name)
    clips = [x.cuda() for x in xs]

    def reset():
        model.load_state_dict(sd)
        model.zero_grad(set_to_none=True)
        model.eval()

    def phase():
        reset()
        with torch.no_grad():
            out = model([c.clone() for c in clips]).clone()
        model.train()
        _step(model, name)
        g = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
        return out, g, _buffers(model)

    def frozen_step(sink=False):
        reset()
        _freeze(model)
        if sink:
            model.zero_grad(set_to_none=True)
            for p in model.parameters():
                p.grad = torch.zeros_like(p)
            engine.set_grad_sink(True)
            try:
                labels = torch.from_numpy(z["train/labels"]).long().cuda()
                torch.nn.functional.cross_entropy(model([c.clone() for c in clips]), labels).backward()
                torch.cuda.synchronize()
            finally:
                engine.set_grad_sink(False)
        else:
            _step(model, name)
        return {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    before = phase()
    f1 = frozen_step()
    f2 = frozen_step()
    f3 = frozen_step(sink=True)
    assert all(torch.equal(f1[k], f2[k]) for k in f1)
    bn_params = [k for k in f1 if "bn" in k and (k.endswith(".weight") or k.endswith(".bias"))]
    assert bn_params and all(torch.equal(f1[k], f3[k]) for k in bn_params)  # in-kernel accumulation into a zero .grad
    model.train()  # (every BN back in training mode)
    after = phase()
    assert torch.equal(before[0], after[0])
    assert all(torch.equal(before[1][k], after[1][k]) for k in before[1])
    assert all(torch.equal(before[2][k], after[2][k]) for k in before[2])


def test_graph_replay_of_a_frozen_step_equals_the_eager_step():
    """The pattern of tests/test_graph_train_gpu.py with every BN frozen: one replay == one eager step, bit for bit
    (parameters, buffers, momentum, flat gradient, loss), and the BN buffers do not move at all."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, ROOT)
    import bench
    from slowfast.models import engine
    from slowfast.utils import misc
    from test_graph_train_gpu import _state
    try:
        dev = torch.device("cuda", 0)
        with contextlib.redirect_stdout(io.StringIO()):
            cfg, model, _, _ = bench.build("shufflenetv2", dev)
        xs = bench.synthetic_clips(cfg, 2, dev, 11)
        labels = torch.randint(0, cfg.MODEL.NUM_CLASSES, (2,), device=dev,
                               generator=torch.Generator(device=dev).manual_seed(3))
        step, flat, opt = bench.make_train_step(model, xs, labels, overlap_allreduce=True, lr=0.02)
        misc.frozen_bn_stats(model)
        assert model.training and not any(m.training for m in model.modules() if isinstance(m, torch.nn.BatchNorm3d))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):      # momentum buffers, packed-weight caches, allocator pools
                step()
        torch.cuda.synchronize()
        state = _state(model, opt)
        snap = [v.detach().clone() for _, v in state]

        def restore():
            with torch.no_grad():
                for (_, v), s in zip(state, snap):
                    v.copy_(s)
            torch.cuda.manual_seed(4242)
            torch.cuda.synchronize()

        def result(loss):
            torch.cuda.synchronize()
            return [v.detach().clone() for _, v in state], flat.flat.detach().clone(), loss.detach().clone()

        restore()
        with torch.cuda.stream(side):
            loss = step().detach().clone()
        eager = result(loss)

        restore()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            static_loss = step()
        restore()
        with torch.cuda.stream(side):
            engine.replay(g)
        replay = result(static_loss)

        assert bool(torch.isfinite(eager[2]).all()) and bool(torch.isfinite(eager[1]).all())
        assert torch.equal(eager[2], replay[2]), ("loss", eager[2].tolist(), replay[2].tolist())
        assert torch.equal(eager[1], replay[1]), "flat gradient"
        moved = 0
        for (k, _), a, b, s in zip(state, eager[0], replay[0], snap):
            assert torch.equal(a, b), k
            if k.startswith("b/"):
                assert torch.equal(a, s), k  # frozen statistics
            else:
                moved += int(not torch.equal(a, s))
        assert moved > 0.9 * sum(1 for k, _ in state if not k.startswith("b/"))
    finally:
        engine.set_grad_sink(False)
