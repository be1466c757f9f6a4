"""NonLocalBlock / Stripe_NonLocalBlock and the stripe entry points without a GPU: the two modules carry the reference's
constructors, attributes, state_dict keys and shapes (the lists recorded in tests/golden/nl_blocks.npz); the float64
restatement of tests/_nlblock_ref.py reproduces what the reference's own classes computed (output 1e-5, dL/dx 1e-4,
parameter gradients 1e-3 — the bounds test_ctx_modules_gpu.py holds its restatement to); a CPU tensor is refused (no
fallback); and sf_stripe_* return SF_EINVAL before any launch — no call below passes a valid argument set, so the host
memory behind the pointers is never touched."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _nlblock_ref as R

_buf = (ctypes.c_float * 64)()
_base = ctypes.addressof(_buf)
_base += (-_base) % 16
P = ctypes.c_void_p(_base)  # 16-byte aligned
NAMES = ["st_mean_soft_s3", "st_meanmax_dot_s2", "st_max_soft_s1_c73", "st_max_dot_s6", "nl_soft", "nl_dot_sub",
         "nl_soft_sub_nobn"]


def _lib():
    import sfhip
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return sfhip.lib()


def _fixture(repo_root):
    z = np.load(os.path.join(repo_root, "tests", "golden", "nl_blocks.npz"))
    return z, json.loads(str(z["meta"]))


def test_state_dict_keys_and_shapes_are_the_reference_s(repo_root):
    _, cases = _fixture(repo_root)
    assert [c["name"] for c in cases] == NAMES
    for case in cases:
        m = R.build_block(case)
        sd = m.state_dict()
        assert list(sd.keys()) == case["sd_keys"], case["name"]
        assert [list(v.shape) for v in sd.values()] == case["sd_shapes"], case["name"]
        assert m.inter_channels == case["inter_channels"] and m.in_channels == case["C"]
        assert m.instance == case["instance"]
    by = {c["name"]: c for c in cases}
    assert by["nl_dot_sub"]["sd_keys"][:2] == ["g.0.weight", "g.0.bias"] and "phi.0.weight" in by["nl_dot_sub"]["sd_keys"]
    assert "W.weight" in by["nl_soft_sub_nobn"]["sd_keys"] and "W.1.running_var" in by["nl_soft"]["sd_keys"]
    assert by["st_meanmax_dot_s2"]["sd_shapes"][0] == [16, 64, 1, 1, 1]  # the in_channels *= 2 quirk: g takes 2C


def test_constructors_and_attributes():
    from slowfast.models.wdf_attention_helper import NonLocalBlock, Stripe_NonLocalBlock
    m = NonLocalBlock(1)
    assert m.inter_channels == 1 and m.sub_sample is False and isinstance(m.W, torch.nn.Sequential)
    assert not bool(m.W[1].weight.detach().any()) and not bool(m.W[1].bias.detach().any())  # a fresh block: identity
    m = NonLocalBlock(8, inter_channels=3, sub_sample=True, bn_layer=False, instance="dot")
    assert m.inter_channels == 3 and isinstance(m.W, torch.nn.Conv3d) and not bool(m.W.weight.detach().any())
    assert isinstance(m.g, torch.nn.Sequential) and isinstance(m.g[1], torch.nn.MaxPool3d)
    assert m.g[1] is m.phi[1] and tuple(m.g[1].kernel_size) == (1, 2, 2) and isinstance(m.theta, torch.nn.Conv3d)
    s = Stripe_NonLocalBlock(4, 8, pool_type="meanmax", instance="dot")
    assert (s.stripe, s.in_channels, s.inter_channels, s.pool_type, s.instance) == (4, 8, 4, "meanmax", "dot")
    assert s.g.in_channels == 16 and s.W[0].out_channels == 8 and not bool(s.W[1].weight.detach().any())
    assert isinstance(s.avgpool, torch.nn.AdaptiveAvgPool2d) and isinstance(s.maxpool, torch.nn.AdaptiveMaxPool2d)
    assert isinstance(Stripe_NonLocalBlock(2, 8, pool_type="max").pool, torch.nn.AdaptiveMaxPool2d)
    assert Stripe_NonLocalBlock(2, 8, inter_channels=5).inter_channels == 5


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference_fixture(repo_root, name):
    z, cases = _fixture(repo_root)
    case = {c["name"]: c for c in cases}[name]
    x, g = R.case_tensors(case)
    assert abs(float(x.double().sum()) - case["input_sum"]) < 1e-6
    m = R.fill_case(R.build_block(case), case)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    r = R.module_ref(case, sd, x, g, torch.float64)
    assert R.rel_l2(torch.from_numpy(z[name + "/out"]), R.stored(r["out"])) < 1e-5
    assert R.rel_l2(torch.from_numpy(z[name + "/eval_out"]), R.stored(r["eval_out"])) < 1e-5
    assert R.rel_l2(torch.from_numpy(z[name + "/dx"]), R.stored(r["dx"])) < 1e-4
    assert sorted(r["grads"]) == sorted(k for k in sd if R.is_param(k))
    for k, v in r["grads"].items():
        assert R.grad_err(torch.from_numpy(z[name + "/grad/" + k]), r["grads"], k) < 1e-3, k
    if r["running_mean"] is not None:
        assert R.rel_l2(torch.from_numpy(z[name + "/after/W.1.running_mean"]), r["running_mean"]) < 1e-5
        assert R.rel_l2(torch.from_numpy(z[name + "/after/W.1.running_var"]), r["running_var"]) < 1e-5
    else:
        assert name == "nl_soft_sub_nobn"


def test_restated_ops_ties_and_the_query_count():
    x = torch.zeros(1, 1, 4, 3, 2)
    x[0, 0, 1, 2, 0] = x[0, 0, 2, 0, 0] = x[0, 0, 3, 1, 0] = 5.0   # channel 0: equal maxima at 5, 6 and 10
    out, arg = R.stripe_pool_ref(x, 1, "max")
    assert arg[0, 0, 0].tolist() == [5, 0] and out[0, 0, 0].tolist() == [5.0, 0.0]  # the first wins; all-equal: 0
    out, arg = R.stripe_pool_ref(x, 2, "meanmax")
    assert tuple(out.shape) == (1, 1, 2, 4) and arg[0, 0, :, 0].tolist() == [5, 0]
    assert out[0, 0, :, 0].tolist() == [5.0 / 6, 10.0 / 6] and out[0, 0, :, 2].tolist() == [5.0, 5.0]
    dx = R.stripe_pool_bwd_ref(x.shape, 2, dmean=torch.full((1, 1, 2, 2), 6.0), dmax=torch.ones(1, 1, 2, 2), arg=arg)
    assert dx[0, 0, :, :, 0].tolist() == [[1, 1, 1], [1, 1, 2], [2, 1, 1], [1, 1, 1]]
    z = R.stripe_add_ref(x, torch.tensor([1.0, 2.0, 3.0, 4.0]).view(1, 1, 2, 2))
    assert z[0, 0, :, 0, 1].tolist() == [2.0, 2.0, 4.0, 4.0]
    th, ph, g = torch.randn(1, 8, 4), torch.randn(1, 4, 2), torch.randn(1, 2, 4)
    assert torch.allclose(R._attend(th, ph, g, "dot"), R._attend(th, ph, g, "dot", scale_by_keys=True) / 4)


def test_a_cpu_tensor_is_refused():
    import sfhip
    from slowfast.models.wdf_attention_helper import NonLocalBlock, Stripe_NonLocalBlock
    x = torch.zeros(1, 8, 2, 4, 3)
    for m in (NonLocalBlock(8), Stripe_NonLocalBlock(2, 8)):
        with pytest.raises(sfhip.SfhipError, match="no CPU fallback"):
            m(x)
    a, v = sfhip.Act(torch.zeros(1, 2, 4, 3, 8)), sfhip.Act(torch.zeros(1, 2, 2, 1, 8))
    with pytest.raises(sfhip.SfhipError):
        sfhip.stripe_pool(a, 2, "mean")
    with pytest.raises(sfhip.SfhipError):
        sfhip.stripe_add(a, v)
    with pytest.raises(sfhip.SfhipError):
        sfhip.stripe_pool_bwd(a, 2, dz=a)


def _pool(L, **kw):
    f = dict(x=P, cs=16, coff=4, N=2, T=2, H=6, W=5, C=8, S=3, mode=2, out=P, out_cs=24, out_coff=4, arg=P)
    f.update(kw)
    return L.sf_stripe_pool_fwd(f["x"], f["cs"], f["coff"], f["N"], f["T"], f["H"], f["W"], f["C"], f["S"], f["mode"],
                                f["out"], f["out_cs"], f["out_coff"], f["arg"], None)


def _add(L, **kw):
    f = dict(x=P, cs=16, coff=4, v=P, v_cs=12, v_coff=4, N=2, T=2, H=6, W=5, C=8, S=3, z=P, z_cs=16, z_coff=8)
    f.update(kw)
    return L.sf_stripe_add_fwd(f["x"], f["cs"], f["coff"], f["v"], f["v_cs"], f["v_coff"], f["N"], f["T"], f["H"],
                               f["W"], f["C"], f["S"], f["z"], f["z_cs"], f["z_coff"], None)


def _bwd(L, **kw):
    f = dict(dz=P, dz_cs=16, dz_coff=4, dmean=P, dmean_cs=16, dmean_coff=0, dmax=P, dmax_cs=16, dmax_coff=8, arg=P, N=2,
             T=2, H=6, W=5, C=8, S=3, dx=P, dx_cs=16, dx_coff=4, acc=1)
    f.update(kw)
    return L.sf_stripe_pool_bwd(f["dz"], f["dz_cs"], f["dz_coff"], f["dmean"], f["dmean_cs"], f["dmean_coff"],
                                f["dmax"], f["dmax_cs"], f["dmax_coff"], f["arg"], f["N"], f["T"], f["H"], f["W"],
                                f["C"], f["S"], f["dx"], f["dx_cs"], f["dx_coff"], f["acc"], None)


def test_stripes_that_do_not_divide_the_height_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for call in (_pool, _add, _bwd):
        for S in (4, 5, 7, 12):
            assert call(L, S=S) == E, (call.__name__, S)
        assert call(L, H=7) == E and call(L, H=2) == E, call.__name__


def test_null_pointers_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for name in ("x", "out", "arg"):
        assert _pool(L, **{name: None}) == E, name
    assert _pool(L, mode=1, arg=None) == E         # both max modes need the positions
    for name in ("x", "v", "z"):
        assert _add(L, **{name: None}) == E, name
    assert _bwd(L, dx=None) == E
    assert _bwd(L, arg=None) == E                  # dmax needs the positions
    assert _bwd(L, dx=None, dz=None, dmean=None, dmax=None, arg=None) == E


def test_non_positive_sizes_and_unknown_modes_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for call in (_pool, _add, _bwd):
        for bad in (0, -1):
            for name in ("N", "T", "H", "W", "C", "S"):
                assert call(L, **{name: bad}) == E, (call.__name__, name, bad)
    for mode in (-1, 4, 17):
        assert _pool(L, mode=mode) == E, mode
    # N*T*S stripe units or hs*W positions past 2^31
    assert _pool(L, N=65536, T=65536, H=6, S=3) == E and _add(L, N=65536, T=65536) == E
    assert _bwd(L, H=65536 * 3, W=65536, S=3) == E


def test_channel_slices_outside_their_pitch_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for kw in (dict(coff=12), dict(coff=-4), dict(cs=4), dict(cs=0)):
        assert _pool(L, **kw) == E, kw
        assert _add(L, **kw) == E, kw
    # meanmax writes 2C = 16 channels: [4, 20) of a pitch of 24 fits, an offset of 12 or a pitch of 16 does not
    for kw in (dict(out_coff=12), dict(out_coff=-4), dict(out_cs=16), dict(mode=0, out_cs=8, out_coff=4)):
        assert _pool(L, **kw) == E, kw
    for kw in (dict(v_coff=8), dict(v_coff=-1), dict(v_cs=7, v_coff=0), dict(z_coff=12), dict(z_coff=-8), dict(z_cs=4)):
        assert _add(L, **kw) == E, kw
    for kw in (dict(dz_coff=12), dict(dz_cs=4), dict(dmean_coff=9), dict(dmean_cs=7), dict(dmax_coff=12),
               dict(dmax_coff=-8), dict(dx_coff=12), dict(dx_coff=-1), dict(dx_cs=7)):
        assert _bwd(L, **kw) == E, kw


def test_wrappers_table_and_audit_list(repo_root):
    import sfhip
    for name in ("stripe_pool", "stripe_add", "stripe_pool_bwd"):
        assert callable(getattr(sfhip, name)), name
    for name in ("sf_stripe_pool_fwd", "sf_stripe_add_fwd", "sf_stripe_pool_bwd"):
        assert name in sfhip.EXPORTS and hasattr(_lib(), name), name
    assert sfhip.STRIPE_MODES == {"mean": 0, "max": 1, "meanmax": 2, "sum": 3}
    assert _lib().sf_abi_version() == 1
    audit = open(os.path.join(repo_root, "tools", "isa_audit.py")).read()
    for k in ("stripe_pool_fwd_kernel", "stripe_bcast_kernel"):
        assert k in audit, k  # on the hot list: scratch or flat accesses fail the build
    a = sfhip.Act(torch.zeros(1, 2, 5, 3, 8))
    with pytest.raises(sfhip.SfhipError):
        sfhip.stripe_pool(a, 2)


def test_dense_attention_keeps_its_default_scale():
    import inspect
    from slowfast.models.nonlocal_helper import dense_attention, materialised_attention
    for fn in (dense_attention, materialised_attention):
        assert inspect.signature(fn).parameters["dot_scale"].default is None  # None = 1 / N_k: existing callers' bits
