"""Grayscale input and the Fast-only ResNet, host side (no GPU): MODEL.ARCH fast builds with the reference's
state_dict, the one-channel entry points are declared / exported / bound, and the one-channel PackedClip keeps the
reference's logical shape and is refused by a stem it was not packed for."""
import ctypes
import json
import os
import re

import pytest
import torch

from _gray import build_gray


def _keys_and_shapes(z):
    return [str(k) for k in z["sd_keys"]], [tuple(json.loads(str(s))) for s in z["sd_shapes"]]


def test_fast_arch_builds_with_the_reference_state_dict():
    """ResNet, MODEL.ARCH fast (reference video_model_builder.py:73-79, :89), WIDTH_PER_GROUP 16, DEPTH 18, one input
    channel: state_dict keys, shapes and child order are the reference's."""
    model, sd, z, meta, cfg = build_gray("fast_r18_gray_s64")
    assert cfg.MODEL.ARCH == "fast" and cfg.RESNET.WIDTH_PER_GROUP == 16 and cfg.RESNET.DEPTH == 18
    keys, shapes = _keys_and_shapes(z)
    got = model.state_dict()
    assert list(got.keys()) == keys
    assert [tuple(v.shape) for v in got.values()] == shapes
    assert [n for n, _ in model.named_children()] == [str(c) for c in z["children"]]
    assert tuple(got["s1.pathway0_stem.conv.weight"].shape) == (16, 1, 5, 7, 7)
    for st in ("s2", "s3", "s4", "s5"):  # temporal-3 `a` convs in every stage
        assert tuple(getattr(model, st).pathway0_res0.branch2.a.kernel_size) == (3, 1, 1)
    assert any(k.startswith("grad/s1.pathway0_stem.conv.weight") for k in z.files)


def test_dual_gray_state_dict_matches_reference():
    model, sd, z, meta, cfg = build_gray("dual_r18_gray_s64")
    keys, shapes = _keys_and_shapes(z)
    got = model.state_dict()
    assert list(got.keys()) == keys
    assert [tuple(v.shape) for v in got.values()] == shapes
    assert [n for n, _ in model.named_children()] == [str(c) for c in z["children"]]
    assert tuple(got["s1.pathway0_stem.conv.weight"].shape) == (64, 1, 1, 7, 7)
    assert tuple(got["s1.pathway1_stem.conv.weight"].shape) == (8, 1, 5, 7, 7)
    for k in ("s1.pathway0_stem.conv.weight", "s1.pathway1_stem.conv.weight"):
        assert "grad/" + k in z.files


NEW_SYMBOLS = ["sf_stem1_accepts", "sf_stem1_fwd", "sf_stem1_wgrad_ws_floats", "sf_stem1_wgrad", "sf_ncthw1_pack",
               "sf_clip_prologue_gray"]


def test_gray_entry_points_are_declared_exported_and_bound(repo_root):
    import sfhip
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    txt = open(os.path.join(repo_root, "include", "sfhip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", txt))
    L = sfhip.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, "include/sfhip.h does not declare %s" % s
        assert hasattr(L, s), "libsfhip.so does not export %s" % s
        assert s in sfhip.EXPORTS and getattr(L, s).argtypes is not None, s
    assert L.sf_stem1_wgrad_ws_floats.restype is ctypes.c_long
    for f in ("ncthw1_pack", "stem1_accepts", "stem1_fwd", "stem1_wgrad", "clip_prologue"):
        assert callable(getattr(sfhip, f))


def test_stem1_range_and_workspace_queries_are_host_only():
    """Cout in {8, 16, 64}, kT <= 5, 7x7 / stride (1,2,2); anything else is left to the padded route.  The workspace of
    the weight gradient is one [Cout][kT*49] partial per workgroup."""
    import sfhip
    L = sfhip.lib()
    for cout, kT in ((8, 5), (16, 5), (64, 1), (64, 5), (8, 3)):
        assert sfhip.stem1_accepts(118, 118, cout, (kT, 7, 7), (1, 2, 2)), (cout, kT)
        n = L.sf_stem1_wgrad_ws_floats(8, 16, 118, 118, cout, kT, kT // 2)
        assert n > 0 and n % (cout * kT * 49) == 0, (cout, kT, n)
    assert not sfhip.stem1_accepts(118, 118, 12, (5, 7, 7), (1, 2, 2))
    assert not sfhip.stem1_accepts(118, 118, 8, (7, 7, 7), (1, 2, 2))
    assert not sfhip.stem1_accepts(118, 118, 8, (5, 3, 3), (1, 2, 2))
    assert not sfhip.stem1_accepts(118, 118, 8, (5, 7, 7), (1, 1, 1))
    assert not sfhip.stem1_accepts(118, 118, 8, (5, 7, 7), (1, 2, 2), dilation=(1, 2, 2))
    assert L.sf_stem1_wgrad_ws_floats(8, 16, 118, 118, 12, 5, 2) == 0


def test_one_channel_packed_clip_reports_the_reference_shape():
    import sfhip
    buf = torch.arange(2 * 16 * 70 * 70, dtype=torch.float32).view(2, 16, 70, 70, 1)
    pc = sfhip.PackedClip(buf, 1, 64, 64, 3, 3)
    assert pc.shape == (2, 1, 16, 64, 64) and pc.Wp == 70 and pc.C == 1
    dense = pc.to_ncthw()
    assert tuple(dense.shape) == pc.shape
    assert torch.equal(dense[:, 0], buf[:, :, 3:67, 3:67, 0])
    with pytest.raises(ValueError):
        sfhip.PackedClip(torch.zeros(2, 16, 70, 70, 4), 1, 64, 64, 3, 3)
    with pytest.raises(ValueError):
        sfhip.PackedClip(torch.zeros(2, 16, 70, 70, 1), 3, 64, 64, 3, 3)


def test_packed_clip_channel_or_geometry_mismatch_raises():
    import sfhip
    from slowfast.models import engine
    gray_conv = torch.nn.Conv3d(1, 8, (5, 7, 7), stride=(1, 2, 2), padding=(2, 3, 3), bias=False)
    rgb_conv = torch.nn.Conv3d(3, 8, (5, 7, 7), stride=(1, 2, 2), padding=(2, 3, 3), bias=False)
    bn = torch.nn.BatchNorm3d(8).eval()
    assert engine.stem_geometry(gray_conv, 64, 64) == (3, 3, 70)
    gray = sfhip.PackedClip(torch.zeros(2, 4, 70, 70, 1), 1, 64, 64, 3, 3)
    rgb = sfhip.PackedClip(torch.zeros(2, 4, 70, 70, 4), 3, 64, 64, 3, 3)
    with pytest.raises(ValueError):
        engine.stem_conv_bn_relu(rgb, gray_conv, bn)     # 3-channel clip, 1-channel stem
    with pytest.raises(ValueError):
        engine.stem_conv_bn_relu(gray, rgb_conv, bn)     # and the reverse
    with pytest.raises(ValueError):                       # right channel count, wrong row pitch
        engine.stem_conv_bn_relu(sfhip.PackedClip(torch.zeros(2, 4, 70, 72, 1), 1, 64, 64, 3, 3), gray_conv, bn)
    with pytest.raises(ValueError):                       # ... wrong border
        engine.stem_conv_bn_relu(sfhip.PackedClip(torch.zeros(2, 4, 68, 70, 1), 1, 64, 64, 2, 3), gray_conv, bn)
