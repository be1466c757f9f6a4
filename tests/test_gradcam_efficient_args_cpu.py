"""Grad-CAM for SlowFastShuffleNet / SlowFastMoibleNetV2 without a GPU: gradcam.target_layers lists the children in
front of `head`, unknown layers are refused with that list, and the two C entries behind the new routes
(sf_epilogue_bwd_act, sf_dwconv_dgrad_epi) are declared, exported, bound, and refuse inconsistent arguments with
SF_EINVAL before any launch — no call below passes a valid argument set, so the host memory behind the pointers is
never touched."""
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

ENTRIES = ("sf_epilogue_bwd_act", "sf_dwconv_dgrad_epi")
SHUFFLENET = ("s1", "s1_fuse", "s2", "s2_fuse", "s3", "s3_fuse", "s4", "s4_fuse")
MOBILENETV2 = ("s1", "s2", "s3_fuse", "s4", "s4_fuse", "s5", "s5_fuse", "s6", "s7", "s7_fuse", "s8")
TARGETS = {"shufflenet_g1_s64": SHUFFLENET, "shufflenet_w2_g3_s64": SHUFFLENET, "mobilenetv2_w1_s64": MOBILENETV2}


def _lib():
    import sfhip
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return sfhip.lib()


def _epi(L, **kw):
    """N1 T2 H3 W5 C12 in pitch-16 buffers at offset 4, ReLU6 + scale, 3 groups: valid until `kw` breaks it."""
    f = dict(dy=P, dy_cs=16, dy_coff=4, y=P, y_cs=16, y_coff=4, N=1, T=2, H=3, W=5, C=12, rep=1, scale=P, act=5,
             groups=3, dz=P, dz_cs=16, dz_coff=4, dz_acc=0, dres=None, dres_cs=0, dres_coff=0, dres_acc=0)
    f.update(kw)
    return L.sf_epilogue_bwd_act(f["dy"], f["dy_cs"], f["dy_coff"], f["y"], f["y_cs"], f["y_coff"], f["N"], f["T"],
                                 f["H"], f["W"], f["C"], f["rep"], f["scale"], f["act"], f["groups"], f["dz"],
                                 f["dz_cs"], f["dz_coff"], f["dz_acc"], f["dres"], f["dres_cs"], f["dres_coff"],
                                 f["dres_acc"], None)


def _dw(L, desc=None, **kw):
    """3x3x3 stride (1,2,2) padding 1 over N1 T2 H5 W5 C8 (dy: T2 H3 W3), pitch-16 buffers at offset 4, ReLU6 + scale."""
    import sfhip
    g = dict(N=1, Ti=2, Hi=5, Wi=5, To=2, Ho=3, Wo=3, k=(3, 3, 3), s=(1, 2, 2), p=(1, 1, 1), dil=(1, 1, 1), wpitch=16)
    g.update(desc or {})
    d = sfhip.ConvDesc(g["N"], g["Ti"], g["Hi"], g["Wi"], 8, 16, 4, g["To"], g["Ho"], g["Wo"], 8, 0, 0, 1,
                       g["k"][0], g["k"][1], g["k"][2], g["s"][0], g["s"][1], g["s"][2], g["p"][0], g["p"][1],
                       g["p"][2], g["dil"][0], g["dil"][1], g["dil"][2], g["wpitch"], 0, 0, 0, 0)
    f = dict(d=ctypes.byref(d), dy=P, dy_cs=16, dy_coff=4, y=P, y_cs=16, y_coff=4, w=P, scale=P, act=5, dx=P,
             dx_cs=16, dx_coff=4, C=8, acc=0)
    f.update(kw)
    return L.sf_dwconv_dgrad_epi(f["d"], f["dy"], f["dy_cs"], f["dy_coff"], f["y"], f["y_cs"], f["y_coff"], f["w"],
                                 f["scale"], f["act"], f["dx"], f["dx_cs"], f["dx_coff"], f["C"], f["acc"], None)


def test_entries_are_declared_exported_and_bound(repo_root):
    """Header, library and ctypes binding agree on the two names: as many bound arguments as the header declares,
    pointers bound as pointers; the header cites the reference lines each entry serves."""
    import sfhip
    L = _lib()
    raw = open(os.path.join(repo_root, "include", "sfhip.h")).read()
    for cite in ("mobilenetv2_helper.py:30-68", "shufflenet_helper.py:22-79", "gradcam_video.py:143-157"):
        assert cite in raw, cite
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ENTRIES:
        assert name in sfhip.EXPORTS and hasattr(L, name), name
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, txt, re.S)
        assert m, "%s is not declared in sfhip.h" % name
        params = [p.strip() for p in m.group(1).split(",")]
        fn = getattr(L, name)
        assert len(fn.argtypes) == len(params), (name, len(fn.argtypes), params)
        for p, a in zip(params, fn.argtypes):
            if "sf_conv_desc" in p:
                assert a is ctypes.POINTER(sfhip.ConvDesc), (name, p, a)
                continue
            want = ctypes.c_void_p if "*" in p else ctypes.c_int
            assert a is want, (name, p, a)
        assert fn.restype is ctypes.c_int, name
    assert callable(sfhip.dwconv_dgrad_epi) and callable(sfhip.epilogue_bwd)


def test_null_pointers_and_non_positive_sizes_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    assert _epi(L, dy=None) == E and _epi(L, dz=None) == E and _epi(L, y=None) == E  # an activation needs y
    assert _epi(L, y=None, act=1) == E
    for name in ("dy", "w", "dx", "y", "d"):
        assert _dw(L, **{name: None}) == E, name
    assert _dw(L, y=None, act=1) == E
    for bad in (0, -1):
        for name in ("N", "T", "H", "W", "C", "rep", "groups"):
            assert _epi(L, **{name: bad}) == E, (name, bad)
        assert _dw(L, C=bad) == E
        for name in ("N", "Ti", "Hi", "Wi", "To", "Ho", "Wo"):
            assert _dw(L, {name: bad}) == E, (name, bad)
        assert _dw(L, dict(k=(3, bad, 3))) == E and _dw(L, dict(s=(1, 2, bad))) == E and _dw(L, dict(dil=(bad, 1, 1))) == E
    assert _dw(L, dict(p=(1, -1, 1))) == E


def test_channel_slices_outside_their_pitch_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for kw in (dict(dy_coff=8), dict(dy_coff=-4), dict(dy_cs=8), dict(y_coff=8), dict(y_cs=0), dict(dz_coff=8),
               dict(dz_cs=4), dict(dz_coff=-1)):
        assert _epi(L, **kw) == E, kw
    for kw in (dict(dres=P, dres_cs=16, dres_coff=12, groups=1), dict(dres=P, dres_cs=7, dres_coff=0, groups=1)):
        assert _epi(L, **kw) == E, kw
    for kw in (dict(dy_coff=12), dict(dy_coff=-4), dict(dy_cs=4), dict(y_coff=12), dict(y_cs=0), dict(dx_coff=12),
               dict(dx_cs=4), dict(dx_coff=-1)):
        assert _dw(L, **kw) == E, kw
    assert _dw(L, dict(wpitch=4)) == E  # the packed weight's pitch holds fewer than C channels


def test_shuffled_form_needs_one_repeat_no_residual_and_divisible_channels():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    assert _epi(L, rep=2) == E                                        # groups > 1 with rep != 1
    assert _epi(L, dres=P, dres_cs=16, dres_coff=4) == E              # groups > 1 with a residual gradient
    assert _epi(L, C=8) == E and _epi(L, groups=5) == E               # C % groups != 0
    assert _epi(L, groups=1, rep=4, dres=P, dres_cs=16, dres_coff=4) == E  # dres only with rep == 1, as sf_epilogue_bwd
    for act in (-1, 2, 3, 4, 9):  # sigmoid / softmax / hard sigmoid / unknown: no conv epilogue applies them
        assert _epi(L, act=act) == E, act
        assert _dw(L, act=act) == E, act


def test_depthwise_output_dims_must_be_the_convs():
    """dy's dims are the conv's output dims: anything else could index rows dy does not have."""
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    assert _dw(L, dict(Ho=4)) == E and _dw(L, dict(Wo=2)) == E and _dw(L, dict(To=3)) == E
    assert _dw(L, dict(s=(1, 1, 1))) == E  # stride 1 would give 5 x 5 outputs, not 3 x 3
    assert _dw(L, dict(Hi=1, Ho=1, k=(3, 5, 3), p=(1, 1, 1))) == E  # a kernel larger than the padded input


def _model(name):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta = load_case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 0
    with contextlib.redirect_stdout(io.StringIO()):
        return build_model(cfg)


@pytest.mark.parametrize("name", sorted(TARGETS))
def test_target_layers_are_the_children_in_front_of_head(name):
    from slowfast.models import gradcam
    model = _model(name)
    want = TARGETS[name]
    assert gradcam.target_layers(model) == want
    assert [n for n, _ in model.named_children()] == list(want) + ["head"]
    for bad in ("head", "s9", "s3_fuse" if "s3_fuse" not in want else "s2_fuse" if "s2_fuse" not in want else "s5", ""):
        with pytest.raises(ValueError) as e:
            gradcam.class_gradients(model, [], bad)
        assert ", ".join(want) in str(e.value), str(e.value)
        with pytest.raises(ValueError) as e:
            gradcam.GradVideoCam(model, bad)
        assert ", ".join(want) in str(e.value)
    model.train()
    gradcam.GradVideoCam(model, want[-1])
    assert not model.training  # the constructor calls model.eval(), as the reference's does


def test_uncovered_models_name_what_is_covered():
    from slowfast.models import gradcam
    for name in ("ghostnet_w2_s64", "shufflenetv2_cfg1"):
        with pytest.raises(NotImplementedError) as e:
            gradcam.target_layers(_model(name))
        for covered in ("SlowFast", "SlowFastDualAttention", "ResNet", "SlowFastShuffleNet", "SlowFastMoibleNetV2"):
            assert covered in str(e.value), str(e.value)
