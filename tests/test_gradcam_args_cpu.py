"""The Grad-CAM entries without a GPU: sf_epilogue_bwd, sf_head_act_mean_bwd, sf_cam_weights and sf_cam_map are
declared in include/sfhip.h, exported by the library and bound with the header's signatures; every call below must be
refused with SF_EINVAL before any launch, so no call here passes a valid argument set and the host memory behind the
pointers is never touched.  models/gradcam.py refuses unknown layers and uncovered models before any GPU call."""
import contextlib
import ctypes
import io
import os
import re

import pytest

from _util import load_case

_buf = (ctypes.c_float * 64)()
_base = ctypes.addressof(_buf)
_base += (-_base) % 16
P = ctypes.c_void_p(_base)  # 16-byte aligned

ENTRIES = ("sf_epilogue_bwd", "sf_head_act_mean_bwd", "sf_cam_weights", "sf_cam_map_ws_floats", "sf_cam_map")


def _lib():
    import sfhip
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return sfhip.lib()


def _epi(L, **kw):
    """N1 T2 H3 W5 C8 in pitch-16 buffers at offset 4, ReLU + scale + residual: valid until `kw` breaks it."""
    f = dict(dy=P, dy_cs=16, dy_coff=4, y=P, y_cs=16, y_coff=4, N=1, T=2, H=3, W=5, C=8, rep=1, scale=P, relu=1, dz=P,
             dz_cs=16, dz_coff=4, dz_acc=0, dres=P, dres_cs=16, dres_coff=4, dres_acc=0)
    f.update(kw)
    return L.sf_epilogue_bwd(f["dy"], f["dy_cs"], f["dy_coff"], f["y"], f["y_cs"], f["y_coff"], f["N"], f["T"], f["H"],
                             f["W"], f["C"], f["rep"], f["scale"], f["relu"], f["dz"], f["dz_cs"], f["dz_coff"],
                             f["dz_acc"], f["dres"], f["dres_cs"], f["dres_coff"], f["dres_acc"], None)


def _head(L, **kw):
    f = dict(logits=P, dout=P, B=2, P=3, K=5, act=3, dl=P, acc=0)
    f.update(kw)
    return L.sf_head_act_mean_bwd(f["logits"], f["dout"], f["B"], f["P"], f["K"], f["act"], f["dl"], f["acc"], None)


def _weights(L, **kw):
    f = dict(g=P, cs=16, coff=4, N=2, T=2, H=3, W=5, C=8, w=P)
    f.update(kw)
    return L.sf_cam_weights(f["g"], f["cs"], f["coff"], f["N"], f["T"], f["H"], f["W"], f["C"], f["w"], None)


def _map(L, **kw):
    f = dict(a=P, cs=16, coff=4, w=P, N=2, T=2, H=3, W=5, C=8, ws=P, raw=P, cam=P)
    f.update(kw)
    return L.sf_cam_map(f["a"], f["cs"], f["coff"], f["w"], f["N"], f["T"], f["H"], f["W"], f["C"], f["ws"], f["raw"],
                        f["cam"], None)


def test_entries_are_declared_exported_and_bound(repo_root):
    """Header, library and ctypes binding agree: same names, and as many bound arguments as the header declares, pointers
    bound as pointers."""
    import sfhip
    L = _lib()
    txt = open(os.path.join(repo_root, "include", "sfhip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert name in sfhip.EXPORTS and hasattr(L, name), name
        m = re.search(r"\b(int|long)\s+%s\s*\((.*?)\)\s*;" % name, txt, re.S)
        assert m, "%s is not declared in sfhip.h" % name
        params = [p.strip() for p in m.group(2).split(",")]
        fn = getattr(L, name)
        assert len(fn.argtypes) == len(params), (name, len(fn.argtypes), params)
        for p, a in zip(params, fn.argtypes):
            want = ctypes.c_void_p if "*" in p else (ctypes.c_float if p.startswith("float ") else ctypes.c_int)
            assert a is want, (name, p, a)
        assert fn.restype is (ctypes.c_long if m.group(1) == "long" else ctypes.c_int), name
    assert sfhip._SIGNATURES["sf_cam_map_ws_floats"][0] is ctypes.c_long


def test_null_pointers_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    assert _epi(L, dy=None) == E and _epi(L, dz=None) == E and _epi(L, y=None) == E  # relu needs y
    assert _head(L, logits=None) == E and _head(L, dout=None) == E and _head(L, dl=None) == E
    assert _weights(L, g=None) == E and _weights(L, w=None) == E
    for name in ("a", "w", "ws", "cam"):
        assert _map(L, **{name: None}) == E, name


def test_non_positive_sizes_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for bad in (0, -1):
        for name in ("N", "T", "H", "W", "C", "rep"):
            assert _epi(L, **{name: bad}) == E, (name, bad)
        for name in ("B", "P", "K"):
            assert _head(L, **{name: bad}) == E, (name, bad)
        for name in ("N", "T", "H", "W", "C"):
            assert _weights(L, **{name: bad}) == E, (name, bad)
            assert _map(L, **{name: bad}) == E, (name, bad)
        assert L.sf_cam_map_ws_floats(2, 3, 5, bad) == 0 and L.sf_cam_map_ws_floats(bad, 3, 5, 8) == 0
    assert L.sf_cam_map_ws_floats(2, 3, 5, 8) == 2 * 3 * 5 * 8


def test_channel_slices_outside_their_pitch_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for kw in (dict(dy_coff=12), dict(dy_coff=-4), dict(dy_cs=4), dict(y_coff=12), dict(y_cs=0), dict(dz_coff=12),
               dict(dz_cs=4), dict(dres_coff=12), dict(dres_coff=-1), dict(dres_cs=7)):
        assert _epi(L, **kw) == E, kw
    for kw in (dict(coff=12), dict(coff=-4), dict(cs=4), dict(cs=0)):
        assert _weights(L, **kw) == E, kw
        assert _map(L, **kw) == E, kw


def test_residual_gradient_with_a_repeat_and_unknown_activations_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    assert _epi(L, rep=4) == E  # dres only with rep == 1
    for act in (-1, 4, 5, 9):   # hard sigmoid / ReLU6 / unknown: the head never applies them
        assert _head(L, act=act) == E, act


def _model(name, **over):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta = load_case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 0
    with contextlib.redirect_stdout(io.StringIO()):
        return build_model(cfg)


def test_unknown_layer_raises_value_error_listing_the_valid_ones():
    from slowfast.models import gradcam
    model = _model("dual_r50_s64")
    for bad in ("s6", "head", "pathway0_pool", ""):
        with pytest.raises(ValueError) as e:
            gradcam.class_gradients(model, [], bad)
        assert "s1, s1_fuse, s2, s2_fuse, s3, s3_fuse, s4, s4_fuse, s5" in str(e.value)
        with pytest.raises(ValueError):
            gradcam.GradVideoCam(model, bad)
    single = _model("slow_r18_s64")
    with pytest.raises(ValueError) as e:
        gradcam.class_gradients(single, [], "s2_fuse")
    assert "s1, s2, s3, s4, s5" in str(e.value) and "fuse" not in str(e.value).split("valid targets are")[1]
    assert gradcam.target_layers(single) == ("s1", "s2", "s3", "s4", "s5")


def test_uncovered_models_raise_not_implemented():
    from slowfast.models import gradcam
    for name in ("ghostnet_w2_s64", "slowfast_r50_ava_s64"):  # an efficient backbone; a DETECTION.ENABLE model
        model = _model(name)
        with pytest.raises(NotImplementedError):
            gradcam.class_gradients(model, [], "s5")
        with pytest.raises(NotImplementedError):
            gradcam.GradVideoCam(model, "s5")


def test_constructor_puts_the_model_in_eval_mode():
    from slowfast.models import gradcam
    model = _model("slow_r18_s64").train()
    gradcam.GradVideoCam(model, "s3")
    assert not model.training
