"""The input step for grayscale clips (sf_clip_prologue_gray through datasets.utils.gpu_input_step): uint8 [T,H,W]
clips -> one-channel PackedClips, against a CPU restatement of the reference's per-clip step with torch ops
(tensor_normalize, datasets/utils.py:298-315; F.interpolate(mode="bilinear", align_corners=False) as
transform.py:329-337 calls it; crop; flip; pack_pathway_output's linspace frame selection, datasets/utils.py:93-104)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _gray import build_gray

pytestmark = pytest.mark.gpu
TOL_ABS = 2e-6  # the RGB kernel's bound, tests/test_input_step.py:88
MEAN, STD = [0.45], [0.225]
CROP = 32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _reference(clip_thw, p, alpha):
    """[slow, fast] ([fast] with alpha None) as [1, T', crop, crop] float tensors."""
    x = (clip_thw.float() / 255.0 - torch.tensor(MEAN)) / torch.tensor(STD)   # tensor_normalize
    x = x.unsqueeze(0)                                                            # THWC -> CTHW with C = 1
    if (p.new_h, p.new_w) != tuple(x.shape[2:]):
        x = F.interpolate(x, size=(p.new_h, p.new_w), mode="bilinear", align_corners=False)
    x = x[:, :, p.y:p.y + p.crop, p.x:p.x + p.crop]
    if p.flip:
        x = x.flip(-1)
    if alpha is None:
        return [x]
    idx = torch.linspace(0, x.shape[1] - 1, x.shape[1] // alpha).long()
    return [torch.index_select(x, 1, idx), x]


def _clips(t, seed, sizes=((40, 52), (36, 36))):
    rs = np.random.RandomState(seed)
    return [torch.from_numpy(rs.randint(0, 256, (t,) + hw).astype(np.uint8)) for hw in sizes]


def _params():
    from slowfast.datasets import utils as ds
    # clip 0: short side 40 -> 36 (bilinear), crop at (3, 9), mirrored; clip 1: identity scale, crop at (2, 4)
    return [ds.SpatialParams(36, 46, 3, 9, True, CROP), ds.SpatialParams(36, 36, 2, 4, False, CROP)]


@pytest.mark.parametrize("alpha", [4, None])
def test_gray_input_step_matches_cpu_restatement(alpha):
    from slowfast.datasets import utils as ds
    dev = _dev()
    clips, params = _clips(9, 5), _params()
    on_dev = [clips[0].to(dev), clips[1].unsqueeze(-1).contiguous().to(dev)]  # both accepted forms: [T,H,W], [T,H,W,1]
    ph, pw, wp = 3, 3, 38  # engine.stem_geometry of a 7x7 / stride 2 / padding 3 stem at 32 x 32
    packed = ds.gpu_input_step(on_dev, params, MEAN, STD, alpha, pad=(ph, pw), wp=wp)
    torch.cuda.synchronize()
    assert len(packed) == (1 if alpha is None else 2)
    frames = [9] if alpha is None else [2, 9]
    worst = 0.0
    for k, pc in enumerate(packed):
        assert pc.shape == (2, 1, frames[k], CROP, CROP) and pc.C == 1
        assert tuple(pc.buf.shape) == (2, frames[k], CROP + 2 * ph, wp, 1)
        got = pc.to_ncthw().cpu()
        for b in range(2):
            ref = _reference(clips[b], params[b], alpha)[k]
            e = float((got[b] - ref).abs().max())
            worst = max(worst, e)
            assert e < TOL_ABS, (alpha, k, b, e)
        buf = pc.buf.cpu()
        assert float(buf[:, :, :ph].abs().max()) == 0.0 and float(buf[:, :, ph + CROP:].abs().max()) == 0.0
        assert float(buf[:, :, :, :pw].abs().max()) == 0.0 and float(buf[:, :, :, pw + CROP:].abs().max()) == 0.0
    print("gray input step alpha %s: max abs error %.3e" % (alpha, worst))
    # a three-element mean is the RGB form: refused for a one-channel clip
    with pytest.raises(AssertionError):
        ds.gpu_input_step(on_dev, params, [0.45] * 3, [0.225] * 3, alpha, pad=(ph, pw), wp=wp)


@pytest.mark.parametrize("name", ["fast_r18_gray_s64", "dual_r18_gray_s64"])
def test_gray_models_accept_packed_clips(name):
    """model(PackedClips) == model(their to_ncthw()), within 1e-5 relative."""
    from slowfast.datasets import utils as ds
    dev = _dev()
    model, sd, z, meta, cfg = build_gray(name)
    model.eval()
    crop, t = meta["size"], meta["t"]
    alpha = None if meta.get("single") else cfg.SLOWFAST.ALPHA
    clips = [c.to(dev) for c in _clips(t, 6, ((crop + 8, crop + 24), (crop + 4, crop + 4)))]
    # clip 0: short side crop + 8 -> crop + 2 (bilinear), mirrored; clip 1: identity scale
    params = [ds.SpatialParams(crop + 2, (crop + 24) * (crop + 2) // (crop + 8), 1, 11, True, crop),
              ds.SpatialParams(crop + 4, crop + 4, 2, 4, False, crop)]
    ph, pw, wp = ds.stem_input_geometry(model, crop)
    packed = ds.gpu_input_step(clips, params, cfg.DATA.MEAN, cfg.DATA.STD, alpha, pad=(ph, pw), wp=wp)
    dense = [p.to_ncthw() for p in packed]
    assert [tuple(d.shape) for d in dense] == [p.shape for p in packed]
    with torch.no_grad():
        a = model(list(packed))
        b = model([d.clone() for d in dense])
    torch.cuda.synchronize()
    e = float((a - b).abs().max() / b.abs().max())
    assert e < 1e-5, e
    wrong = ds.gpu_input_step(clips, params, cfg.DATA.MEAN, cfg.DATA.STD, alpha, pad=(ph + 1, pw), wp=wp)
    with pytest.raises(ValueError):
        model(list(wrong))
