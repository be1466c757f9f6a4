"""Action detection (ResNetRoIHead) without a GPU: the models built from the AVA fixtures' cfg dumps carry the
reference's state_dict, children and head layout; the efficient backbones still refuse DETECTION.ENABLE; and the
float64 RoIAlign restatement (tests/_roi_align_ref.py) the fixtures and the GPU tests rely on is pinned against
analytic cases."""
import contextlib
import io
import json

import pytest
import torch
import torch.nn as nn

from _roi_align_ref import roi_align
from _util import load_case

DET_CASES = ["slowfast_r50_ava_s64", "slow_r50_ava_s64", "dual_r50_ava_s64"]


def _cfg(meta):
    from slowfast.config.defaults import get_cfg
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 0
    return cfg


def _build(cfg):
    from slowfast.models import build_model
    with contextlib.redirect_stdout(io.StringIO()):
        return build_model(cfg)


@pytest.mark.parametrize("name", DET_CASES)
def test_detection_model_matches_reference_layout(name):
    z, meta = load_case(name)
    model = _build(_cfg(meta))
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in z["sd_keys"]]
    assert [list(v.shape) for v in sd.values()] == [json.loads(str(s)) for s in z["sd_shapes"]]
    assert [n for n, _ in model.named_children()] == [str(c) for c in z["children"]]
    head = model.head
    assert [n for n, _ in head.named_children()] == [str(c) for c in z["head_children"]]
    assert [type(m).__name__ for _, m in head.named_children()] == [str(c) for c in z["head_children_types"]]
    assert [k for k in sd if k.startswith("head.")] == ["head.projection.weight", "head.projection.bias"]


@pytest.mark.parametrize("name", DET_CASES)
def test_roi_head_children_attributes(name):
    from slowfast.models.head_helper import ROIAlign, ResNetRoIHead
    z, meta = load_case(name)
    cfg = _cfg(meta)
    head = _build(cfg).head
    assert isinstance(head, ResNetRoIHead)
    R = cfg.DETECTION.ROI_XFORM_RESOLUTION
    T = cfg.DATA.NUM_FRAMES
    tpools = [T // cfg.SLOWFAST.ALPHA, T] if head.num_pathways == 2 else [T]
    for p in range(head.num_pathways):
        tp, roi, sp = (getattr(head, "s%d_%s" % (p, k)) for k in ("tpool", "roi", "spool"))
        assert isinstance(tp, nn.AvgPool3d) and list(tp.kernel_size) == [tpools[p], 1, 1] and tp.stride == 1
        assert isinstance(roi, ROIAlign) and not list(roi.parameters())
        assert list(roi.output_size) == [R, R] and roi.sampling_ratio == 0 and roi.aligned is True
        assert roi.spatial_scale == pytest.approx(1.0 / cfg.DETECTION.SPATIAL_SCALE_FACTOR)
        assert isinstance(sp, nn.MaxPool2d) and list(sp.kernel_size) == [R, R] and sp.stride == 1
    assert isinstance(head.dropout, nn.Dropout) and head.dropout.p == cfg.MODEL.DROPOUT_RATE
    assert isinstance(head.projection, nn.Linear) and head.projection.out_features == cfg.MODEL.NUM_CLASSES
    assert isinstance(head.act, nn.Sigmoid)


def test_aligned_flag_reaches_the_head():
    z, meta = load_case("slowfast_r50_ava_s64")
    cfg = _cfg(meta)
    cfg.DETECTION.ALIGNED = False
    head = _build(cfg).head
    assert head.s0_roi.aligned is False and head.s1_roi.aligned is False


@pytest.mark.parametrize("model_name", ["SlowFastShuffleNetV2", "SlowFastShuffleNet", "SlowFastMoibleNetV2"])
def test_efficient_models_still_refuse_detection(model_name):
    from slowfast.config.defaults import get_cfg
    cfg = get_cfg()
    cfg.NUM_GPUS = 0
    cfg.MODEL.MODEL_NAME = model_name
    cfg.DETECTION.ENABLE = True
    with pytest.raises(NotImplementedError):
        _build(cfg)


def test_softmax_head_act_with_detection_raises():
    z, meta = load_case("slowfast_r50_ava_s64")
    cfg = _cfg(meta)
    cfg.MODEL.HEAD_ACT = "softmax"
    with pytest.raises(NotImplementedError, match="softmax"):
        _build(cfg)


# ------------------------------------------------------------------------------ the float64 restatement
def _box(n, x1, y1, x2, y2):
    return torch.tensor([[n, x1, y1, x2, y2]], dtype=torch.float64)


@pytest.mark.parametrize("aligned", [True, False])
def test_restatement_constant_map(aligned):
    x = torch.full((2, 3, 6, 5), 2.5, dtype=torch.float64)
    out = roi_align(x, _box(1, 8.0, 4.0, 56.0, 60.0), 7, 1.0 / 16, 0, aligned)
    assert out.shape == (1, 3, 7, 7)
    assert torch.allclose(out, torch.full_like(out, 2.5), rtol=0, atol=1e-12)


@pytest.mark.parametrize("aligned", [True, False])
def test_restatement_affine_ramp_gives_bin_centroid(aligned):
    """An affine map a + b*h + c*w, sampled where every sample is inside [0, H-1] x [0, W-1]: bilinear interpolation
    is exact, so each bin is the ramp at the mean of its sample points = the bin centre."""
    H, W, R = 12, 10, 4
    a, b, c = 0.3, 1.25, -0.7
    hh = torch.arange(H, dtype=torch.float64).view(H, 1)
    ww = torch.arange(W, dtype=torch.float64).view(1, W)
    x = (a + b * hh + c * ww).view(1, 1, H, W)
    scale, off = 0.5, (0.5 if aligned else 0.0)
    x1, y1, x2, y2 = 4.0, 3.0, 15.0, 19.0  # map coordinates 2..7.5 x 1.5..9.5, inside
    out = roi_align(x, _box(0, x1, y1, x2, y2), R, scale, 0, aligned)[0, 0]
    sh, sw = y1 * scale - off, x1 * scale - off
    bh, bw = (y2 - y1) * scale / R, (x2 - x1) * scale / R
    for ph in range(R):
        for pw in range(R):
            cy, cx = sh + (ph + 0.5) * bh, sw + (pw + 0.5) * bw
            assert float(out[ph, pw]) == pytest.approx(a + b * cy + c * cx, abs=1e-12)


def test_restatement_box_outside_is_zero():
    x = torch.randn(1, 4, 8, 8, dtype=torch.float64)
    out = roi_align(x, _box(0, 400.0, 400.0, 480.0, 470.0), 7, 1.0 / 16, 0, True)
    assert float(out.abs().max()) == 0.0
    out = roi_align(x, _box(0, -300.0, -300.0, -100.0, -120.0), 7, 1.0 / 16, 0, False)
    assert float(out.abs().max()) == 0.0


def test_restatement_batch_index_out_of_range_is_zero():
    x = torch.randn(2, 4, 8, 8, dtype=torch.float64)
    rois = torch.tensor([[2, 0, 0, 64, 64], [-1, 0, 0, 64, 64], [1, 0, 0, 64, 64]], dtype=torch.float64)
    out = roi_align(x, rois, 7, 1.0 / 8, 0, True)
    assert float(out[:2].abs().max()) == 0.0 and float(out[2].abs().max()) > 0


def test_restatement_aligned_vs_legacy_offset():
    """A one-pixel box at map pixel (2, 3) (scale 1), R = 1, on a map that is 1 at that pixel only: aligned shifts by
    -0.5 so its single sample lands exactly on the pixel centre (value 1); legacy samples at (2.5, 3.5), half-way
    between four pixels (value 1/4)."""
    x = torch.zeros(1, 1, 6, 6, dtype=torch.float64)
    x[0, 0, 2, 3] = 1.0
    box = _box(0, 3.0, 2.0, 4.0, 3.0)
    assert float(roi_align(x, box, 1, 1.0, 0, True)) == pytest.approx(1.0, abs=1e-12)
    assert float(roi_align(x, box, 1, 1.0, 0, False)) == pytest.approx(0.25, abs=1e-12)


def test_restatement_zero_size_aligned_box_is_zero():
    """aligned: no clamp of the extent, so a zero-size box has an empty sampling grid (count 1, sum 0)."""
    x = torch.randn(1, 2, 8, 8, dtype=torch.float64)
    out = roi_align(x, _box(0, 40.0, 40.0, 40.0, 40.0), 7, 1.0 / 8, 0, True)
    assert float(out.abs().max()) == 0.0
    legacy = roi_align(x, _box(0, 40.0, 40.0, 40.0, 40.0), 7, 1.0 / 8, 0, False)  # extent clamped to 1 cell
    assert float(legacy.abs().max()) > 0


def test_restatement_gradient_is_the_transposed_weights():
    x = torch.randn(1, 3, 5, 7, dtype=torch.float64, requires_grad=True)
    rois = torch.tensor([[0, 6.0, -8.0, 70.0, 50.0]], dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda t: roi_align(t, rois, 3, 0.125, 0, True), (x,))
