"""Frozen-BN training without a GPU: sf_bn_frozen_bwd is declared, exported and bound with one signature; the entry and
its ctypes wrapper refuse inconsistent arguments before any launch (no call below passes a valid argument set, so the
host memory behind the pointers is never touched); utils.misc.frozen_bn_stats puts the BatchNorm3d layers — and only
them — into eval(); and, by the oracle alone, which parameters of the fixtures have a gradient too small to be compared
relatively (tests/test_frozen_bn_models_gpu.py bounds those absolutely)."""
import contextlib
import ctypes
import io
import os
import re

import pytest
import torch

import _frozen
from _util import load_case

_buf = (ctypes.c_float * 64)()
_base = ctypes.addressof(_buf)
_base += (-_base) % 16
P = ctypes.c_void_p(_base)  # 16-byte aligned

KEY_BIAS = "attention_spatial_s2f.key_conv.bias"
# fixtures of the issue's table: the tiny list is exactly the four key_conv.bias (none on the single-pathway model)
TABLE = ["slow_r18_s64", "dual_r50_s64", "dual_r50_subbn_s64", "shufflenet_w2_g3_s64", "ghostnet_w2_s64"]
# the other two: the same four biases; cfg #1 also has one dead Fast-pathway branch (its ReLU passes nothing at this seed)
EXTRA = {"shufflenetv2_cfg1": ["s3.pathway1_channel_8.features.7.banch2.0.weight",
                               "s3.pathway1_channel_8.features.7.banch2.1.weight",
                               "s3.pathway1_channel_8.features.7.banch2.4.weight",
                               "s3.pathway1_channel_8.features.7.banch2.6.weight"],
         "mobilenetv2_w1_s64": []}


def _lib():
    import sfhip
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return sfhip.lib()


def _call(L, **kw):
    """N1 T2 H3 W5 C8 in pitch-16 buffers at offset 4, ReLU from y, affine, residual accumulated, sums wanted: valid
    until `kw` breaks it."""
    f = dict(dy=P, dy_cs=16, dy_coff=4, y=P, y_cs=16, y_coff=4, z=P, z_cs=16, z_coff=4, N=1, T=2, H=3, W=5, C=8, rep=1,
             relu=1, mean=P, invstd=P, gamma=P, dz=P, dz_cs=16, dz_coff=4, dres=P, dres_cs=16, dres_coff=4, dres_acc=1,
             dbeta=P, dgamma=P, ws=P)
    f.update(kw)
    return L.sf_bn_frozen_bwd(f["dy"], f["dy_cs"], f["dy_coff"], f["y"], f["y_cs"], f["y_coff"], f["z"], f["z_cs"],
                              f["z_coff"], f["N"], f["T"], f["H"], f["W"], f["C"], f["rep"], f["relu"], f["mean"],
                              f["invstd"], f["gamma"], f["dz"], f["dz_cs"], f["dz_coff"], f["dres"], f["dres_cs"],
                              f["dres_coff"], f["dres_acc"], f["dbeta"], f["dgamma"], f["ws"], None)


def test_entry_is_declared_exported_and_bound(repo_root):
    """Header, library and binding agree: as many bound arguments as the header declares, pointers bound as pointers;
    the header cites the reference lines and the torch semantics the entry serves."""
    import sfhip
    L = _lib()
    raw = open(os.path.join(repo_root, "include", "sfhip.h")).read()
    for cite in ("misc.py:246-254", "torch.nn.BatchNorm3d eval"):
        assert cite in raw, cite
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    name = "sf_bn_frozen_bwd"
    assert name in sfhip.EXPORTS and hasattr(L, name)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, txt, re.S)
    assert m, "%s is not declared in sfhip.h" % name
    params = [p.strip() for p in m.group(1).split(",")]
    fn = getattr(L, name)
    assert len(fn.argtypes) == len(params) == 30, (len(fn.argtypes), params)
    for p, a in zip(params, fn.argtypes):
        assert a is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, a)
    assert fn.restype is ctypes.c_int
    assert callable(sfhip.bn_frozen_bwd)
    audit = open(os.path.join(repo_root, "tools", "isa_audit.py")).read()
    assert "bn_frozen_bwd_kernel" in audit  # on the hot list: scratch or flat accesses fail the build


def test_null_pointers_and_non_positive_sizes_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for name in ("dy", "z", "dz", "mean", "invstd", "y"):  # (y: an activation needs it)
        assert _call(L, **{name: None}) == E, name
    assert _call(L, dbeta=None) == E and _call(L, dgamma=None) == E  # the two sums come together
    assert _call(L, ws=None) == E                                    # ... and need the workspace
    for bad in (0, -1):
        for name in ("N", "T", "H", "W", "C", "rep"):
            assert _call(L, **{name: bad}) == E, (name, bad)
    for relu in (-1, 4, 9):
        assert _call(L, relu=relu) == E, relu


def test_channel_slices_outside_their_pitch_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for kw in (dict(dy_coff=12), dict(dy_coff=-4), dict(dy_cs=4), dict(y_coff=12), dict(y_cs=0), dict(z_coff=12),
               dict(z_cs=7), dict(z_coff=-1), dict(dz_coff=9), dict(dz_cs=4), dict(dz_coff=-1), dict(dres_coff=12),
               dict(dres_cs=7, dres_coff=0), dict(dres_coff=-4)):
        assert _call(L, **kw) == E, kw


def test_repeat_with_a_residual_and_bad_masks_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    assert _call(L, rep=4) == E and _call(L, rep=2, dres_acc=0) == E   # rep > 1 requires dres == NULL
    # the byte mask: rep 1, C % 4 == 0, pitch C/4 at offset 0, float4-addressable views
    assert _call(L, relu=3, y_cs=2, y_coff=0, rep=2, dres=None) == E
    assert _call(L, relu=3, y_cs=16, y_coff=4) == E
    assert _call(L, relu=3, y_cs=2, y_coff=0, C=6, dy_cs=8, z_cs=8, dz_cs=8, dres=None) == E
    assert _call(L, relu=3, y_cs=2, y_coff=0, dy_coff=2) == E          # scalar-form views have no byte mask


def test_wrapper_refuses_cpu_tensors_missing_tensors_and_a_repeat_with_a_residual():
    import sfhip
    from sfhip import Act
    a = lambda t=2, c=8: Act(torch.zeros(1, t, 3, 5, c))
    v = torch.zeros(8)
    with pytest.raises(sfhip.SfhipError, match="no CPU fallback"):
        sfhip.bn_frozen_bwd(a(), a(), a(), v, v, v, True)
    with pytest.raises(sfhip.SfhipError, match="required"):
        sfhip.bn_frozen_bwd(None, None, a(), v, v, v, False)
    with pytest.raises(sfhip.SfhipError, match="required"):
        sfhip.bn_frozen_bwd(a(), None, None, v, v, v, False)
    with pytest.raises(sfhip.SfhipError):
        sfhip.bn_frozen_bwd(a(4), a(4), a(), v, v, v, True, rep=2, dres=a())  # CPU tensors / rep > 1 with dres


def _model(name):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta = load_case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 0
    with contextlib.redirect_stdout(io.StringIO()):
        return build_model(cfg)


@pytest.mark.parametrize("name", ["slow_r18_s64", "dual_r50_subbn_s64", "ghostnet_w2_s64"])
def test_frozen_bn_stats_leaves_every_other_module_in_train_mode(name):
    from slowfast.utils import misc
    model = _model(name).train()
    misc.frozen_bn_stats(model)
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm3d)]
    assert bns and not any(m.training for m in bns)
    rest = [m for m in model.modules() if not isinstance(m, torch.nn.BatchNorm3d)]
    assert rest and all(m.training for m in rest)
    assert model.training
    assert all(p.requires_grad for p in model.parameters())  # eval() freezes statistics, not gamma / beta


@pytest.mark.parametrize("name", _frozen.FIXTURES)
def test_tiny_gradient_parameters_by_the_oracle_alone(name):
    """fp64 oracle, eval forward, parameters as leaves: every float parameter receives a gradient, and the ones whose
    gradient norm is below 1e-6 of the largest are exactly the SpatialAttention key biases (softmax is invariant to a
    per-query constant) — plus, on cfg #1, one dead Fast-pathway branch."""
    g64, logits = _frozen.oracle_grads(name, torch.float64)
    assert all(g is not None for g in g64.values())
    assert bool(torch.isfinite(logits).all())
    tiny = _frozen.tiny_parameters(name)
    keys = [k for k in tiny if k.endswith(KEY_BIAS)]
    other = [k for k in tiny if not k.endswith(KEY_BIAS)]
    if name == "slow_r18_s64":
        assert tiny == []
    else:
        assert len(keys) == 4, tiny
        assert other == (EXTRA[name] if name not in TABLE else []), other
