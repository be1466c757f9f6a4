"""Grad-CAM through whole models (slowfast/models/gradcam.py) against the oracle's eval forward.

Gradient parity: the oracle is evaluated with the HIP path's own target activations as autograd leaves
(sd["__override__"], as tests/_stage.py does), once in float64 and once in float32, and out[n, cls[n]] is
back-propagated to them.  Per pathway, as relative L2 over the tensor:
    err(HIP, fp64) <= max(1e-3, 4 x err(oracle fp32, fp64))
— the rule of test_fullsize_gpu.py::test_cfg1_every_gradient_within_the_reference_own_fp32_noise.  Forward parity keeps
the 1e-3 max-norm relative tolerance of test_models_gpu.py::test_eval_forward_matches_reference_golden.  The maps are
compared with a numpy restatement of the reference's gradcam_video.py:159-179 on class_gradients' own acts / grads.

Observed on an MI355X (HIP vs fp64 / oracle fp32 vs fp64): dual_r50_s64 s5 5.4e-7 / 2.6e-6, s3_fuse 5.1e-5 / 4.1e-5 and
1.5e-6 / 3.3e-6, s2 6.2e-5 / 9.8e-4; slowfast_r50_s64 s4_fuse 4.4e-7 / 4.7e-7; slow_r18_s64 s3 9.7e-7 / 1.4e-6;
dual_r18_gray_tired_s64 s5 1.6e-6 / 4.6e-7 (every run appends its values to models_report.txt through _report)."""
import contextlib
import io

import numpy as np
import pytest
import torch

from _util import case_inputs, load_case, rel_err, sample_activation, seeded_state_dict

TOL = 1e-3  # test_models_gpu.py::TOL
GRAD_CASES = [("dual_r50_s64", "s5"), ("dual_r50_s64", "s3_fuse"), ("dual_r50_s64", "s2"),
              ("slowfast_r50_s64", "s4_fuse"), ("slow_r18_s64", "s3"), ("dual_r18_gray_tired_s64", "s5")]
# targets where the seeded fixtures' maps are not flat (earlier targets: gradients of order 1e-4, nearly every frame
# below the 1e-3 range threshold); held by test_fixtures_have_few_degenerate_frames_by_the_oracle_alone
CAM_CASES = [("dual_r50_s64", "s5"), ("slowfast_r50_s64", "s4_fuse"), ("slow_r18_s64", "s5")]
DEGENERATE = 1e-3  # a frame whose fp64 range is below this fraction of its map's maximum is not compared


def _report(line):
    """One line per figure in models_report.txt, beside the other model-level reports."""
    from test_models_gpu import _report as report
    report(line)


def _inputs(meta):
    if meta["cfg_dump"]["DATA"]["INPUT_CHANNEL_NUM"][0] == 1:
        from _gray import gray_inputs
        return gray_inputs(meta)
    return case_inputs(meta)


_CASES = {}


def _case(name):
    """(z, meta, state_dict, clips) of a fixture, loaded once."""
    if name not in _CASES:
        z, meta = load_case(name)
        sd = seeded_state_dict(z["sd_keys"], z["sd_shapes"], meta["param_seed"])
        _CASES[name] = (z, meta, sd, _inputs(meta))
    return _CASES[name]


def _build(name):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta, sd, xs = _case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    missing = model.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return model.eval()


def _oracle_grads(name, target, leaves, cls, dtype):
    """(d out[n, cls[n]] / d leaves, out) of the oracle's eval forward with `leaves` substituted at `target`."""
    from oracle import slowfast_oracle as oracle
    z, meta, sd, xs = _case(name)
    sdr = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    lv = [torch.as_tensor(a).to(dtype).clone().requires_grad_(True) for a in leaves]
    sdr["__override__"] = {target: lv}
    acts = oracle.FORWARDS[meta["model"]](sdr, [x.to(dtype) for x in xs], meta["hparams"], training=False)
    out = acts["out"]
    if cls is None:
        cls = out.detach().argmax(1)
    out[torch.arange(out.shape[0]), cls].sum().backward()
    return [l.grad.detach().double() for l in lv], out.detach(), cls


def _cams_ref(acts, grads):
    """float64 restatement of gradcam_video.py:159-179 per sample: [(cam [N,T,H,W], per-frame range, map maximum)]."""
    res = []
    for a, g in zip(acts, grads):
        a, g = np.asarray(a, np.float64), np.asarray(g, np.float64)
        w = g.mean(axis=(3, 4))                                   # [N, C, T]
        abar = a.mean(axis=2)                                     # [N, C, H, W]
        cam = np.maximum(1.0 + np.einsum("nct,nchw->nthw", w, abar), 0.0)
        lo = cam.min(axis=(2, 3), keepdims=True)
        rng = cam.max(axis=(2, 3), keepdims=True) - lo
        norm = np.where(rng > 0, (cam - lo) / np.where(rng > 0, rng, 1.0), 0.0)
        res.append((norm, rng[:, :, 0, 0], cam.max(axis=(2, 3))))
    return res


def _degenerate(rng, top):
    return rng < DEGENERATE * np.maximum(top, 1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize("name,target", GRAD_CASES)
def test_class_gradients_match_the_oracle(name, target):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from slowfast.models import gradcam
    z, meta, sd, xs = _case(name)
    model = _build(name)
    acts, grads, out, cls = gradcam.class_gradients(model, [x.cuda() for x in xs], target)
    torch.cuda.synchronize()
    assert len(acts) == len(grads) == len(xs)
    assert torch.equal(cls, out.argmax(1)) and cls.dtype == torch.int64 and tuple(cls.shape) == (out.shape[0],)
    # forward parity: the target's outputs and the eval output against the reference's recorded ones
    for i, a in enumerate(acts):
        tag = "eval/%s/%d" % (target, i)
        assert a.dtype == torch.float32 and a.is_cuda and tuple(a.shape) == tuple(z[tag + "/shape"]), tag
        assert tuple(grads[i].shape) == tuple(a.shape)
        s, _, _ = sample_activation(a.cpu().numpy())
        e = rel_err(s, z[tag])
        _report("%-26s gradcam %-8s p%d forward %.3e" % (name, target, i, e))
        assert e < TOL, (tag, e)
    e_out = rel_err(out.cpu().numpy(), z["eval/out"])
    assert e_out < TOL, e_out
    with torch.no_grad():
        plain = model([x.cuda() for x in xs])
    assert rel_err(out.cpu().numpy(), plain.cpu().numpy()) < TOL
    # gradient parity
    leaves = [a.cpu() for a in acts]
    c = cls.cpu()
    g64, o64, _ = _oracle_grads(name, target, leaves, c, torch.float64)
    g32, _, _ = _oracle_grads(name, target, leaves, c, torch.float32)
    for i, g in enumerate(grads):
        ref = g64[i]
        assert float(ref.norm()) > 0
        e_hip = float((g.cpu().double() - ref).norm() / ref.norm())
        e_ref = float((g32[i] - ref).norm() / ref.norm())
        _report("%-26s gradcam %-8s p%d grad vs oracle fp64: HIP %.3e, oracle fp32 %.3e" % (name, target, i, e_hip, e_ref))
        print("%s %s p%d: HIP %.3e oracle-fp32 %.3e" % (name, target, i, e_hip, e_ref))
        assert bool(torch.isfinite(g).all())
        assert e_hip <= max(1e-3, 4.0 * e_ref), (name, target, i, e_hip, e_ref)


@pytest.mark.gpu
def test_target_class_is_broadcast_and_batch_of_one_runs():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from slowfast.models import gradcam
    name, target = "slow_r18_s64", "s3"
    z, meta, sd, xs = _case(name)
    model = _build(name)
    k = int(z["eval/out"].shape[1]) - 1
    acts, grads, out, cls = gradcam.class_gradients(model, [x[:1].cuda() for x in xs], target, target_class=k)
    torch.cuda.synchronize()
    assert cls.tolist() == [k] and out.shape[0] == 1 and acts[0].shape[0] == 1
    assert bool(torch.isfinite(grads[0]).all()) and float(grads[0].abs().max()) > 0
    both = gradcam.class_gradients(model, [x.cuda() for x in xs], target, target_class=torch.tensor([k, 0]))
    assert both[3].tolist() == [k, 0]
    bcast = gradcam.class_gradients(model, [x.cuda() for x in xs], target, target_class=k)
    assert bcast[3].tolist() == [k, k]


@pytest.mark.gpu
@pytest.mark.parametrize("name,target", CAM_CASES)
def test_generate_cam_videos_matches_the_reference_arithmetic(name, target):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from slowfast.models import gradcam
    z, meta, sd, xs = _case(name)
    model = _build(name).train()
    cam = gradcam.GradVideoCam(model, target)
    assert not model.training  # the constructor calls model.eval(), as the reference does
    clips = [x.cuda() for x in xs]
    cams = cam.generate_cam_videos(clips)
    again = cam.generate_cam_videos(clips)
    acts, grads, out, cls = gradcam.class_gradients(model, clips, target)
    torch.cuda.synchronize()
    assert len(cams) == len(xs)
    frames = skipped = 0
    for p, (ref, rng, top) in enumerate(_cams_ref([a.cpu().numpy() for a in acts], [g.cpu().numpy() for g in grads])):
        got = cams[p]
        n, c, t, h, w = acts[p].shape
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (n, t, h, w)
        assert torch.equal(got, again[p])
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
        keep = ~_degenerate(rng, top)
        frames += keep.size
        skipped += int((~keep).sum())
        e = float(np.abs(got.cpu().numpy().astype(np.float64) - ref)[keep].max())
        _report("%-26s gradcam %-8s p%d cam abs %.3e (%d of %d frames degenerate)" % (
            name, target, p, e, int((~keep).sum()), keep.size))
        assert e <= 1e-5, (p, e)
    assert skipped * 10 <= frames, (skipped, frames)


@pytest.mark.parametrize("name,target", CAM_CASES)
def test_fixtures_have_few_degenerate_frames_by_the_oracle_alone(name, target):
    """CPU: with the oracle's own activations and float32 gradients, the frames whose range is below 1e-3 of their map's
    maximum (the ones the GPU comparison skips) are at most a tenth."""
    from oracle import slowfast_oracle as oracle
    z, meta, sd, xs = _case(name)
    with torch.no_grad():
        own = oracle.FORWARDS[meta["model"]](dict(sd), [x.clone() for x in xs], meta["hparams"], training=False)[target]
    grads, out, cls = _oracle_grads(name, target, [a.detach() for a in own], None, torch.float32)
    frames = skipped = 0
    for ref, rng, top in _cams_ref([a.detach().numpy() for a in own], [g.numpy() for g in grads]):
        bad = _degenerate(rng, top)
        frames += bad.size
        skipped += int(bad.sum())
    assert frames > 0 and skipped * 10 <= frames, (skipped, frames)


@pytest.mark.gpu
def test_gradcam_has_no_side_effects():
    """A plain eval forward and one training step give the same bits before and after a Grad-CAM call; the call leaves
    parameters, buffers and every p.grad (None) as they were; two calls are bit-identical."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from slowfast.models import gradcam
    name, target = "dual_r50_s64", "s3_fuse"
    z, meta, sd, xs = _case(name)
    model = _build(name)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    clips = [x.cuda() for x in xs]
    labels = torch.from_numpy(z["train/labels"]).cuda()

    def reset():
        model.load_state_dict(sd)
        model.zero_grad(set_to_none=True)
        model.eval()

    def phase():
        reset()
        with torch.no_grad():
            out = model([c.clone() for c in clips]).clone()
        model.train()
        logits = model([c.clone() for c in clips])
        torch.nn.functional.cross_entropy(logits, labels).backward()
        torch.cuda.synchronize()
        g = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        return out, logits.detach().clone(), g, state

    before = phase()
    reset()
    state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    first = gradcam.class_gradients(model, clips, target)
    second = gradcam.class_gradients(model, clips, target)
    torch.cuda.synchronize()
    assert not model.training
    assert all(p.grad is None for p in model.parameters())
    assert all(torch.equal(v, state0[k]) for k, v in model.state_dict().items())
    for a, b in zip(first[0] + first[1] + [first[2], first[3]], second[0] + second[1] + [second[2], second[3]]):
        assert torch.equal(a, b)
    model.train()  # a training-mode model is evaluated in eval mode and handed back in training mode
    third = gradcam.class_gradients(model, clips, target)
    assert model.training and torch.equal(third[2], first[2]) and torch.equal(third[1][0], first[1][0])
    assert all(p.grad is None for p in model.parameters())
    assert all(torch.equal(v, state0[k]) for k, v in model.state_dict().items())
    after = phase()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert all(torch.equal(before[2][k], after[2][k]) for k in before[2])
    assert all(torch.equal(before[3][k], after[3][k]) for k in before[3])
