"""Grad-CAM through SlowFastShuffleNet (GROUPS 1 and 3) and SlowFastMoibleNetV2 against the oracle's eval forward: the
cases of tests/test_gradcam_models_gpu.py for the efficient backbones, with that file's helpers and rules.

Gradient parity, per pathway as relative L2:  err(HIP, fp64) <= max(1e-3, 4 x err(oracle fp32, fp64)), the oracle
evaluated with the HIP path's own target activations as leaves (an activation at a ReLU / ReLU6 edge may fall on the
other side in fp32).  Forward parity keeps that file's TOL.  The CAM comparison leaves out a frame only when the
oracle's own map range is below DEGENERATE of its maximum, and at most a quarter of the frames; a CPU test holds that
for the fixture with the oracle alone.

Observed on an MI355X (HIP vs fp64 / oracle fp32 vs fp64, slow then fast): shufflenet_g1_s64 s2 1.4e-4 / 3.4e-5 and
6.5e-5 / 1.5e-5, s4_fuse 7.0e-7 / 1.9e-6 and 7.3e-7 / 2.0e-6; shufflenet_w2_g3_s64 s3 1.2e-4 / 1.6e-4 and 2.1e-4 / 5.0e-5,
s1_fuse 2.0e-4 / 4.1e-4 and 2.2e-4 / 3.9e-4; mobilenetv2_w1_s64 s8 2.6e-7 / 4.6e-7 and 1.4e-7 / 3.8e-7, s5_fuse 5.5e-7 /
8.1e-7 and 4.2e-7 / 5.2e-7, s2 7.2e-7 / 9.1e-7 and 6.7e-7 / 7.9e-7 (every run appends its values to models_report.txt
through _report).  shufflenet_g1_s64 s2 crosses s3_fuse's 36-channel attention over 64 positions: the case that found the
padded-key overflow of attn_bwd_bx2_kernel (NaN in dQ where a query's log-sum-exp is below -127)."""
import numpy as np
import pytest
import torch

from test_gradcam_models_gpu import (TOL, _build, _cams_ref, _case, _degenerate, _oracle_grads, _report)
from _util import rel_err, sample_activation

GRAD_CASES = [("shufflenet_g1_s64", "s2"), ("shufflenet_g1_s64", "s4_fuse"),
              ("shufflenet_w2_g3_s64", "s3"),       # crosses grouped convs and their shuffled stores
              ("shufflenet_w2_g3_s64", "s1_fuse"),  # every stage: the stride-2 Bottlenecks' relu(cat[conv3, shortcut]) tails
              ("mobilenetv2_w1_s64", "s8"), ("mobilenetv2_w1_s64", "s5_fuse"),
              ("mobilenetv2_w1_s64", "s2")]         # crosses strided depthwise convs and the expand-ratio-1 block
CAM_CASE = ("shufflenet_g1_s64", "s4_fuse")


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
    assert all(p.grad is None for p in model.parameters())
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
    g64, _, _ = _oracle_grads(name, target, leaves, c, torch.float64)
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
def test_generate_cam_videos_matches_the_reference_arithmetic():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from slowfast.models import gradcam
    name, target = CAM_CASE
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
    # which frames are degenerate is decided by the ORACLE's own maps (its fp64 gradients at these activations)
    leaves = [a.cpu() for a in acts]
    g64, _, _ = _oracle_grads(name, target, leaves, cls.cpu(), torch.float64)
    own = _cams_ref([a.numpy() for a in leaves], [g.numpy() for g in g64])
    frames = skipped = 0
    for p, (ref, rng, top) in enumerate(_cams_ref([a.numpy() for a in leaves], [g.cpu().numpy() for g in grads])):
        got = cams[p]
        n, c, t, h, w = acts[p].shape
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (n, t, h, w)
        assert torch.equal(got, again[p])
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
        keep = ~_degenerate(own[p][1], own[p][2])
        frames += keep.size
        skipped += int((~keep).sum())
        e = float(np.abs(got.cpu().numpy().astype(np.float64) - ref)[keep].max())
        _report("%-26s gradcam %-8s p%d cam abs %.3e (%d of %d frames degenerate)" % (
            name, target, p, e, int((~keep).sum()), keep.size))
        assert e <= 1e-5, (p, e)
    assert skipped * 4 <= frames, (skipped, frames)


def test_cam_fixture_has_few_degenerate_frames_by_the_oracle_alone():
    """CPU: with the oracle's own activations and float32 gradients, the frames whose range is below DEGENERATE of
    their map's maximum (the ones the GPU comparison may leave out) are at most a quarter."""
    from oracle import slowfast_oracle as oracle
    name, target = CAM_CASE
    z, meta, sd, xs = _case(name)
    with torch.no_grad():
        own = oracle.FORWARDS[meta["model"]](dict(sd), [x.clone() for x in xs], meta["hparams"], training=False)[target]
    grads, out, cls = _oracle_grads(name, target, [a.detach() for a in own], None, torch.float32)
    frames = skipped = 0
    for ref, rng, top in _cams_ref([a.detach().numpy() for a in own], [g.numpy() for g in grads]):
        bad = _degenerate(rng, top)
        frames += bad.size
        skipped += int(bad.sum())
    assert frames > 0 and skipped * 4 <= frames, (skipped, frames)


@pytest.mark.gpu
def test_gradcam_has_no_side_effects_on_a_shufflenet():
    """A plain eval forward and one training step of a grouped ShuffleNet give the same bits before and after a
    Grad-CAM call; the call leaves parameters, buffers and every p.grad (None) as they were; two calls are
    bit-identical."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from slowfast.models import gradcam
    name, target = "shufflenet_w2_g3_s64", "s2_fuse"
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
    after = phase()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert all(torch.equal(before[2][k], after[2][k]) for k in before[2])
    assert all(torch.equal(before[3][k], after[3][k]) for k in before[3])
