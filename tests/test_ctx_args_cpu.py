"""ChannelAttention / ContextBlock3D and their entry points without a GPU: the two modules carry the reference's
state_dict keys and shapes (the lists recorded in tests/golden/ctx_blocks.npz), ContextBlock3D's constructor checks fire,
'channel_mul' raises from forward, a CPU tensor is refused (no fallback), and sf_ctx_pool_* / sf_sample_affine_* return
SF_EINVAL before any launch — no call below passes a valid argument set, so the host memory behind the pointers is
never touched."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _ctx_ref

_buf = (ctypes.c_float * 64)()
_base = ctypes.addressof(_buf)
_base += (-_base) % 16
P = ctypes.c_void_p(_base)  # 16-byte aligned


def _lib():
    import sfhip
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return sfhip.lib()


def _cases(repo_root):
    z = np.load(os.path.join(repo_root, "tests", "golden", "ctx_blocks.npz"))
    return json.loads(str(z["meta"]))


def test_state_dict_keys_and_shapes_are_the_reference_s(repo_root):
    cases = _cases(repo_root)
    assert [c["name"] for c in cases] == ["ca_c8_r16", "ca_c64_r16", "gc_att_c32_r1", "gc_att_c32_r025",
                                          "gc_avg_c30_r05"]
    for case in cases:
        sd = _ctx_ref.build_block(case).state_dict()
        assert list(sd.keys()) == case["sd_keys"], case["name"]
        assert [list(v.shape) for v in sd.values()] == case["sd_shapes"], case["name"]
    ca = _ctx_ref.build_block(cases[0])
    assert ca.conv_du[0].out_channels == 2  # channel // reduction == 0 -> 2
    assert isinstance(ca.avg_pool, torch.nn.AdaptiveAvgPool3d)


def test_channel_mul_keeps_the_reference_s_keys():
    from slowfast.models.wdf_attention_helper import ContextBlock3D
    m = ContextBlock3D(8, ratio=0.5, pooling_type="att", fusion_types=("channel_add", "channel_mul"))
    keys = list(m.state_dict().keys())
    assert keys == ["conv_mask.weight", "conv_mask.bias"] + [
        "%s.%d.%s" % (b, i, p) for b in ("channel_add_conv", "channel_mul_conv") for i in (0, 1, 3)
        for p in ("weight", "bias")]
    assert tuple(m.channel_add_conv[1].weight.shape) == (4, 1, 1, 1)
    assert tuple(m.channel_mul_conv[1].weight.shape) == (4, 1, 1)  # the reference's mismatched LayerNorm, kept
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        m(torch.zeros(1, 8, 2, 2, 2))
    only_mul = ContextBlock3D(8, fusion_types=("channel_mul",))
    assert only_mul.channel_add_conv is None
    with pytest.raises(NotImplementedError):
        only_mul(torch.zeros(1, 8, 2, 2, 2))


def test_a_fresh_context_block_is_initialised_as_the_reference():
    from slowfast.models.wdf_attention_helper import ContextBlock3D
    torch.manual_seed(3)
    m = ContextBlock3D(64, ratio=0.25)
    assert m.planes == 16
    last = m.channel_add_conv[3]
    assert not bool(last.weight.detach().any()) and not bool(last.bias.detach().any())
    assert not bool(m.conv_mask.bias.detach().any())
    # kaiming normal, fan_in, ReLU gain: std = sqrt(2 / 64); 64 samples -> within a factor of 1.5
    s = float(m.conv_mask.weight.detach().std())
    assert (2.0 / 64) ** 0.5 / 1.5 < s < (2.0 / 64) ** 0.5 * 1.5, s
    avg = ContextBlock3D(8, pooling_type="avg")
    assert not hasattr(avg, "conv_mask") and isinstance(avg.avg_pool, torch.nn.AdaptiveAvgPool3d)


def test_constructor_assertions_fire():
    from slowfast.models.wdf_attention_helper import ContextBlock3D
    with pytest.raises(AssertionError):
        ContextBlock3D(8, pooling_type="max")
    with pytest.raises(AssertionError):
        ContextBlock3D(8, fusion_types="channel_add")
    with pytest.raises(AssertionError):
        ContextBlock3D(8, fusion_types=("channel_sub",))
    with pytest.raises(AssertionError, match="at least one fusion"):
        ContextBlock3D(8, fusion_types=())


def test_a_cpu_tensor_is_refused():
    import sfhip
    from slowfast.models.wdf_attention_helper import ChannelAttention, ContextBlock3D
    x = torch.zeros(1, 8, 2, 3, 3)
    for m in (ChannelAttention(8), ContextBlock3D(8), ContextBlock3D(8, pooling_type="avg")):
        with pytest.raises(sfhip.SfhipError, match="no CPU fallback"):
            m(x)
    a = sfhip.Act(torch.zeros(1, 2, 3, 3, 8))
    v = torch.zeros(1, 8)
    with pytest.raises(sfhip.SfhipError):
        sfhip.ctx_pool(a, torch.zeros(8), torch.zeros(1))
    with pytest.raises(sfhip.SfhipError):
        sfhip.ctx_pool_bwd(a, torch.zeros(8), torch.zeros(1), torch.zeros(1), v, v, a)
    with pytest.raises(sfhip.SfhipError):
        sfhip.sample_affine(a, mul=v)
    with pytest.raises(sfhip.SfhipError):
        sfhip.sample_affine_bwd(a, a, x=a, mul=v, want_dmul=True)


def _pool_fwd(L, **kw):
    f = dict(x=P, cs=16, coff=4, N=2, rows=30, C=8, w=P, b=P, ctx=P, lse=P, ws=P)
    f.update(kw)
    return L.sf_ctx_pool_fwd(f["x"], f["cs"], f["coff"], f["N"], f["rows"], f["C"], f["w"], f["b"], f["ctx"],
                             f["lse"], f["ws"], None)


def _pool_bwd(L, **kw):
    f = dict(x=P, cs=16, coff=4, N=2, rows=30, C=8, w=P, b=P, lse=P, ctx=P, dctx=P, dx=P, dx_cs=16, dx_coff=4, acc=1,
             dw=P, db=P, dw_acc=0, ws=P)
    f.update(kw)
    return L.sf_ctx_pool_bwd(f["x"], f["cs"], f["coff"], f["N"], f["rows"], f["C"], f["w"], f["b"], f["lse"],
                             f["ctx"], f["dctx"], f["dx"], f["dx_cs"], f["dx_coff"], f["acc"], f["dw"], f["db"],
                             f["dw_acc"], f["ws"], None)


def _aff_fwd(L, **kw):
    f = dict(x=P, cs=16, coff=4, N=2, rows=30, C=8, mul=P, add=P, out=P, out_cs=16, out_coff=4)
    f.update(kw)
    return L.sf_sample_affine_fwd(f["x"], f["cs"], f["coff"], f["N"], f["rows"], f["C"], f["mul"], f["add"],
                                  f["out"], f["out_cs"], f["out_coff"], None)


def _aff_bwd(L, **kw):
    f = dict(dy=P, dy_cs=16, dy_coff=4, x=P, x_cs=16, x_coff=4, N=2, rows=30, C=8, mul=P, dx=P, dx_cs=16, dx_coff=4,
             acc=1, dmul=P, dadd=P, ws=P)
    f.update(kw)
    return L.sf_sample_affine_bwd(f["dy"], f["dy_cs"], f["dy_coff"], f["x"], f["x_cs"], f["x_coff"], f["N"],
                                  f["rows"], f["C"], f["mul"], f["dx"], f["dx_cs"], f["dx_coff"], f["acc"],
                                  f["dmul"], f["dadd"], f["ws"], None)


def test_null_pointers_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for name in ("x", "w", "ctx", "lse", "ws"):
        assert _pool_fwd(L, **{name: None}) == E, name
    for name in ("x", "w", "lse", "ctx", "dctx", "dx"):
        assert _pool_bwd(L, **{name: None}) == E, name
    assert _pool_bwd(L, ws=None) == E            # dw needs the workspace
    assert _pool_bwd(L, dw=None) == E            # db comes with dw
    for name in ("x", "out"):
        assert _aff_fwd(L, **{name: None}) == E, name
    for name in ("dy", "dx"):
        assert _aff_bwd(L, **{name: None}) == E, name
    assert _aff_bwd(L, x=None) == E              # dmul needs x
    assert _aff_bwd(L, ws=None) == E and _aff_bwd(L, ws=None, dmul=None) == E  # either sum needs the workspace


def test_non_positive_and_out_of_range_sizes_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for call in (_pool_fwd, _pool_bwd, _aff_fwd, _aff_bwd):
        for bad in (0, -1):
            for name in ("N", "rows", "C"):
                assert call(L, **{name: bad}) == E, (call.__name__, name, bad)
        assert call(L, N=65536) == E, call.__name__
    # more channels than the kernels' lane layout covers (the pitch follows, so only C is out of range)
    assert _pool_fwd(L, C=2052, cs=2052, coff=0) == E
    assert _pool_bwd(L, C=2052, cs=2052, coff=0, dx_cs=2052, dx_coff=0) == E
    assert _aff_fwd(L, C=2052, cs=2052, coff=0, out_cs=2052, out_coff=0) == E
    assert _aff_bwd(L, C=2052, dy_cs=2052, dy_coff=0, x_cs=2052, x_coff=0, dx_cs=2052, dx_coff=0) == E
    assert L.sf_ctx_pool_ws_floats(0, 30, 8) == 0 and L.sf_ctx_pool_ws_floats(2, 0, 8) == 0
    assert L.sf_ctx_pool_ws_floats(2, 30, 0) == 0 and L.sf_sample_affine_ws_floats(2, -1, 8) == 0
    assert L.sf_ctx_pool_parts(0) == 0 and L.sf_ctx_pool_parts(-5) == 0


def test_channel_slices_outside_their_pitch_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for kw in (dict(coff=12), dict(coff=-4), dict(cs=4), dict(cs=0)):
        assert _pool_fwd(L, **kw) == E, kw
        assert _pool_bwd(L, **kw) == E, kw
        assert _aff_fwd(L, **kw) == E, kw
    for kw in (dict(dx_coff=12), dict(dx_coff=-1), dict(dx_cs=7)):
        assert _pool_bwd(L, **kw) == E, kw
        assert _aff_bwd(L, **kw) == E, kw
    for kw in (dict(out_coff=9), dict(out_coff=-4), dict(out_cs=4)):
        assert _aff_fwd(L, **kw) == E, kw
    for kw in (dict(dy_coff=12), dict(dy_cs=4), dict(x_coff=12), dict(x_cs=7, x_coff=0), dict(x_coff=-4)):
        assert _aff_bwd(L, **kw) == E, kw


def test_partition_and_workspace_sizes():
    """What the GPU tests read their shapes from: a workgroup owns at most 128 positions until a sample would need more
    than 1024 of them; no workgroup is left without a position."""
    L = _lib()
    assert [L.sf_ctx_pool_parts(r) for r in (1, 63, 128, 129, 300, 384, 385)] == [1, 1, 1, 2, 3, 3, 4]
    assert L.sf_ctx_pool_parts(128 * 1024) == 1024 and L.sf_ctx_pool_parts(128 * 1024 + 1) <= 1024
    for rows in (131073, 140000, 1047553, 5000000):
        p = L.sf_ctx_pool_parts(rows)
        run = -(-rows // p)
        assert p <= 1024 and (p - 1) * run < rows <= p * run, (rows, p, run)
    assert L.sf_ctx_pool_ws_floats(3, 300, 30) == 3 * 3 * 33
    assert L.sf_sample_affine_ws_floats(3, 300, 30) == 3 * 3 * 60


def test_wrappers_and_audit_list(repo_root):
    import sfhip
    for name in ("ctx_pool", "ctx_pool_bwd", "sample_affine", "sample_affine_bwd"):
        assert callable(getattr(sfhip, name)), name
    for name in ("sf_ctx_pool_parts", "sf_ctx_pool_ws_floats", "sf_ctx_pool_fwd", "sf_ctx_pool_bwd",
                 "sf_sample_affine_ws_floats", "sf_sample_affine_fwd", "sf_sample_affine_bwd"):
        assert name in sfhip.EXPORTS and hasattr(_lib(), name), name
    audit = open(os.path.join(repo_root, "tools", "isa_audit.py")).read()
    for k in ("ctx_pool_fwd_kernel", "ctx_pool_bwd_kernel", "sample_affine_fwd_kernel", "sample_affine_bwd_kernel"):
        assert k in audit, k  # on the hot list: scratch or flat accesses fail the build
