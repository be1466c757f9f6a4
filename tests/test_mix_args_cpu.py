"""Host side of soft-target training (sf_ce_mix, sf_clip_batch_mix, sf_clip_batch_mix_gray; slowfast/models/step_tail.py,
slowfast/datasets/utils.py): the binding's rows, every refusal — decided before any launch, so callable without a GPU —
the mix-row table, upstream's mix decision (`sample_mix_params`), and the numpy restatement of the loss
(tests/_mix_ref.py) against F.cross_entropy with dense probability targets in float64."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _mix_ref as ref

FAKE = 0x7f0000001000  # a non-null, 16-byte aligned "device address": a refused call never dereferences it
ONE = 0x3f800000       # 1.0f


def _st():
    from slowfast.models import step_tail
    return step_tail


def _ds():
    from slowfast.datasets import utils
    return utils


def _ring():
    return _st().StatsRing(4, device="cpu")


# ------------------------------------------------------------------------------------------------ the binding
def test_signature_table_has_the_new_symbols():
    import sfhip
    vp, ci, cf, pi = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_int)
    want = {"sf_ce_mix": (ci, [vp, ci, vp, vp, vp, ci, ci, ci, cf, vp, vp, pi, ci, vp, vp]),
            "sf_clip_batch_mix": sfhip._SIGNATURES["sf_clip_batch"],
            "sf_clip_batch_mix_gray": sfhip._SIGNATURES["sf_clip_batch_gray"]}
    for name, sig in want.items():
        assert sfhip._SIGNATURES[name] == sig, name
        assert name in sfhip.EXPORTS and hasattr(sfhip.lib(), name)
    assert sfhip.SF_MIX_ROW == 7 == ref.MIX_ROW
    assert sfhip.lib().sf_abi_version() == 1
    assert callable(sfhip.clip_batch_mix) and callable(_st().ce_mix) and callable(_ds().gpu_train_batch_mix)


# ------------------------------------------------------------------------------------------------ C refusals: the loss
def _good_rows(N):
    rows = torch.zeros((N, 7), dtype=torch.int64)
    rows[:, 0] = torch.arange(N - 1, -1, -1)
    rows[:, 1] = 1
    rows[:, 2] = ref.lam_bits(0.3)
    return rows


def _ce_mix_rc(N=4, K=10, k_hi=5, ld=None, cap=3, eps=0.1, rows="good", dev=True, null=None):
    import sfhip
    p = ctypes.c_void_p(FAKE)
    cnt = ctypes.cast(ctypes.c_void_p(FAKE), sfhip._pi)
    if isinstance(rows, str):
        rows = _good_rows(max(N, 1))
    host = ctypes.c_void_p(rows.data_ptr()) if rows is not None else None
    args = [p, K if ld is None else ld, p, host, p if dev else None, N, K, k_hi, eps, p, p, cnt, cap, p, None]
    if null is not None:
        args[null] = None
    return sfhip.lib().sf_ce_mix(*args)


def _edited(rows, r, c, v):
    out = rows.clone()
    out[r, c] = v
    return out


def test_ce_mix_refusals():
    import sfhip
    E = sfhip.SF_EINVAL
    # everything sf_ce_topk refuses
    assert _ce_mix_rc(k_hi=11) == E and _ce_mix_rc(k_hi=0) == E
    assert _ce_mix_rc(N=0) == E and _ce_mix_rc(N=-1) == E
    assert _ce_mix_rc(K=0, k_hi=0) == E and _ce_mix_rc(K=-3, k_hi=1) == E
    assert _ce_mix_rc(cap=0) == E and _ce_mix_rc(cap=-1) == E
    assert _ce_mix_rc(ld=9) == E
    for null in (0, 2, 9, 10, 11, 13):  # logits, labels, dlogits, ring, counter, loss_out
        assert _ce_mix_rc(null=null) == E, null
        assert _ce_mix_rc(null=null, rows=None, dev=False) == E, null
    # smoothing outside [0, 1), NaN
    for eps in (-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        assert _ce_mix_rc(eps=eps) == E, eps
        assert _ce_mix_rc(eps=eps, rows=None, dev=False) == E, eps
    # exactly one of mix / mix_host
    assert _ce_mix_rc(rows=None, dev=True) == E and _ce_mix_rc(dev=False) == E
    # a host row: the partner outside [0, N), the mode outside {0, 1, 2}, lam outside [0, 1]
    good = _good_rows(4)
    for r, c, v in ((0, 0, 4), (3, 0, -1), (1, 0, 1 << 40), (2, 1, 3), (2, 1, -1),
                    (1, 2, ref.lam_bits(1.5)), (1, 2, ref.lam_bits(-0.25)), (0, 2, ref.lam_bits(float("nan"))),
                    (0, 2, ref.lam_bits(float("inf"))), (3, 2, ONE + (1 << 32)), (3, 2, -1)):
        assert _ce_mix_rc(rows=_edited(good, r, c, v)) == E, (r, c, v)


# ------------------------------------------------------------------------------------------------ C refusals: the batch
def _batch_inputs():
    ds = _ds()
    videos = [torch.zeros(5, 20, 28, 3, dtype=torch.uint8), torch.zeros(8, 24, 24, 3, dtype=torch.uint8)]
    samples = [(torch.tensor([0, 1, 3, 4]), ds.SpatialParams(10, 14, 1, 3, False, 8)),
               (torch.tensor([2, 2, 7, 7]), ds.SpatialParams(24, 24, 16, 0, True, 8))]
    mix = ds.MixParams((1, 0), ds.MIX_CUTMIX, 0.75, (2, 0, 6, 4))
    tab = torch.cat([ds.batch_table(videos, samples, ds.slow_frame_indices(4, 2)), ds.mix_rows(mix).flatten()])
    return tab.contiguous()


def test_clip_batch_mix_argument_checks_are_host_only():
    import sfhip
    L = sfhip.lib()
    tab = _batch_inputs()
    assert tab.numel() == 2 * 9 + 2 * 4 + 2 + 2 * 7
    MIX0 = 28  # the first mix row
    m3 = (ctypes.c_float * 3)(0.45, 0.45, 0.45)
    mp = ctypes.cast(m3, ctypes.c_void_p)
    fake = ctypes.c_void_p(4096)

    def call(gray, tab=tab, table=fake, fast=fake, slow=fake, B=2, n_fast=4, n_slow=2, crop=8, pw=0, wp=8, mean=mp):
        host = ctypes.c_void_p(tab.data_ptr()) if tab is not None else None
        if gray:
            return L.sf_clip_batch_mix_gray(host, table, B, n_fast, n_slow, crop, 0.45, 0.225, fast, slow, 0, pw, wp,
                                            None)
        return L.sf_clip_batch_mix(host, table, B, n_fast, n_slow, crop, 0, mean, mp, fast, slow, 0, pw, wp, None)

    def edited(pos, val):
        bad = tab.clone()
        bad[pos] = val
        return bad

    refusals = [
        # sf_clip_batch's list
        dict(tab=None), dict(table=None), dict(fast=None), dict(B=0), dict(B=-1), dict(n_fast=0), dict(crop=0),
        dict(pw=-1), dict(tab=edited(1, 0)), dict(tab=edited(9 + 2, 0)), dict(tab=edited(3, -28)),
        dict(tab=edited(4, 0)), dict(tab=edited(9 + 5, -24)), dict(tab=edited(9, 0)),
        dict(tab=edited(6, 3)), dict(tab=edited(7, 7)), dict(tab=edited(6, -1)), dict(tab=edited(9 + 6, 17)),
        dict(tab=edited(18 + 3, 5)), dict(tab=edited(18 + 4, -1)), dict(tab=edited(18 + 7, 8)),
        dict(n_slow=5), dict(tab=edited(27, 4)), dict(tab=edited(26, -1)), dict(tab=edited(27, 0)),
        dict(tab=edited(26, 3)), dict(slow=None), dict(pw=1), dict(wp=7), dict(B=65536), dict(n_fast=65536),
        # the mix rows: partner, mode, lam
        dict(tab=edited(MIX0 + 0, 2)), dict(tab=edited(MIX0 + 7, -1)),
        dict(tab=edited(MIX0 + 1, 3)), dict(tab=edited(MIX0 + 8, -1)),
        dict(tab=edited(MIX0 + 2, ref.lam_bits(1.25))), dict(tab=edited(MIX0 + 9, ref.lam_bits(float("nan")))),
        dict(tab=edited(MIX0 + 2, ONE + (1 << 32))), dict(tab=edited(MIX0 + 2, ref.lam_bits(-0.5))),
        # the box: 0 <= y0 <= y1 <= crop, 0 <= x0 <= x1 <= crop (the row holds y0 = 2, x0 = 0, y1 = 6, x1 = 4)
        dict(tab=edited(MIX0 + 3, -1)), dict(tab=edited(MIX0 + 3, 7)), dict(tab=edited(MIX0 + 5, 9)),
        dict(tab=edited(MIX0 + 4, -1)), dict(tab=edited(MIX0 + 4, 5)), dict(tab=edited(MIX0 + 6, 9)),
        dict(tab=edited(MIX0 + 7 + 5, 1)),
    ]
    for gray in (False, True):
        for kw in refusals:
            assert call(gray, **kw) == sfhip.SF_EINVAL, (gray, kw)
    assert call(False, mean=None) == sfhip.SF_EINVAL
    for kw in (dict(fast=ctypes.c_void_p(4096 + 4)), dict(slow=ctypes.c_void_p(4096 + 8))):
        assert call(False, **kw) == sfhip.SF_EINVAL, kw
    for kw in (dict(fast=ctypes.c_void_p(4096 + 2)), dict(slow=ctypes.c_void_p(4096 + 1))):
        assert call(True, **kw) == sfhip.SF_EINVAL, kw
    # no CPU fallback in the wrappers
    ds = _ds()
    with pytest.raises(sfhip.SfhipError):
        sfhip.clip_batch_mix(tab, tab, 2, 8, [0.45] * 3, [0.225] * 3, torch.zeros(2, 4, 8, 8, 4))
    videos = [torch.zeros(5, 20, 28, 3, dtype=torch.uint8), torch.zeros(8, 24, 24, 3, dtype=torch.uint8)]
    samples = [(torch.tensor([0, 1, 3, 4]), ds.SpatialParams(10, 14, 1, 3, False, 8)),
               (torch.tensor([2, 2, 7, 7]), ds.SpatialParams(24, 24, 16, 0, True, 8))]
    with pytest.raises(sfhip.SfhipError):
        ds.gpu_train_batch_mix(videos, samples, ds.MixParams((1, 0), 1, 0.5, (0, 0, 0, 0)), [0.45] * 3, [0.225] * 3, 2)
    with pytest.raises(ValueError, match="mix rows"):
        ds.gpu_train_batch_mix(videos, samples, ds.MixParams((2, 1, 0), 1, 0.5, (0, 0, 0, 0)), [0.45] * 3,
                               [0.225] * 3, 2)


# ------------------------------------------------------------------------------------------------ Python refusals
def test_python_refusals_come_before_the_gpu_is_needed():
    import sfhip
    st = _st()
    ring, out = _ring(), torch.zeros(2)
    x, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    rows = _good_rows(4)
    # weight together with smoothing, weight together with mix rows
    with pytest.raises(ValueError, match="weight"):
        st.HipCrossEntropy(2, ring, weight=[1.0, 2.0, 3.0], label_smoothing=0.1)
    with pytest.raises(ValueError, match="weight"):
        st.HipCrossEntropy(2, ring, weight=[1.0, 2.0, 3.0])(x, y, mix=(rows, rows))
    # smoothing outside [0, 1)
    for eps in (-0.1, 1.0, 2.0, float("nan"), "a lot", None):
        with pytest.raises(ValueError, match="smoothing"):
            st.HipCrossEntropy(2, ring, label_smoothing=eps)
        with pytest.raises(ValueError, match="smoothing"):
            st.ce_mix(x, y, 2, ring, out, smoothing=eps)
    with pytest.raises(ValueError, match="smoothing"):
        st.HipMixUp(label_smoothing=1.0)
    # wrong shapes and dtypes of the rows; one of the pair missing; a host copy that is not on the host
    bad = {"dtype": rows.to(torch.int32), "rows": _good_rows(5), "columns": torch.zeros((4, 6), dtype=torch.int64),
           "flat": rows.flatten(), "strided": torch.zeros((4, 14), dtype=torch.int64)[:, ::2], "not a tensor": [[0] * 7] * 4}
    for what, r in bad.items():
        with pytest.raises(ValueError, match="mix"):
            st.ce_mix(x, y, 2, ring, out, mix_host=rows, mix=r)
        with pytest.raises(ValueError, match="mix_host"):
            st.ce_mix(x, y, 2, ring, out, mix_host=r, mix=rows)
    with pytest.raises(ValueError, match="pair"):
        st.ce_mix(x, y, 2, ring, out, mix=rows)
    with pytest.raises(ValueError, match="pair"):
        st.ce_mix(x, y, 2, ring, out, mix_host=rows)
    with pytest.raises(ValueError, match="HOST"):
        st.ce_mix(x, y, 2, ring, out, mix_host=rows.to("meta"), mix=rows)
    with pytest.raises(ValueError):
        st.ce_mix(x, torch.zeros(5, dtype=torch.int64), 2, ring, out)
    with pytest.raises(ValueError, match="mix"):
        st.HipCrossEntropy(2, ring)(x, y, mix="rows")
    with pytest.raises(ValueError, match="pair"):
        st.HipCrossEntropy(2, ring)(x, y, mix=(rows, rows, rows))
    # good arguments on CPU predictions: no fallback
    with pytest.raises(sfhip.SfhipError):
        st.ce_mix(x, y, 2, ring, out, mix_host=rows, mix=rows, smoothing=0.1)
    with pytest.raises(sfhip.SfhipError):
        st.HipCrossEntropy(2, ring, label_smoothing=0.1)(x, y)
    with pytest.raises(sfhip.SfhipError):
        st.HipCrossEntropy(2, ring)(x, y, mix=rows)
    # without smoothing and mix the object is what it was
    ce = st.HipCrossEntropy(2, ring)
    assert ce.label_smoothing == 0.0 and ce.weight is None
    assert st.HipCrossEntropy(2, ring, label_smoothing=0.1).label_smoothing == 0.1


def test_config_keys_are_read_with_get():
    st = _st()
    from slowfast.config.defaults import get_cfg
    cfg = get_cfg()
    assert "MIXUP" not in cfg  # config/defaults.py keeps the reference's key set
    cfg.MODEL.LOSS_FUNC, cfg.MODEL.NUM_CLASSES, cfg.TRAIN.TOPK = "cross_entropy", 3, 2
    assert st.construct_hip_mixup(cfg) is None
    assert st.get_hip_loss_func(cfg, _ring()).label_smoothing == 0.0
    cfg.MIXUP = type(cfg)({"ENABLE": True, "ALPHA": 0.4, "CUTMIX_ALPHA": 0.0, "PROB": 0.5, "LABEL_SMOOTH_VALUE": 0.2})
    m = st.construct_hip_mixup(cfg)
    assert (m.mixup_alpha, m.cutmix_alpha, m.prob, m.switch_prob, m.label_smoothing) == (0.4, 0.0, 0.5, 0.5, 0.2)
    f = st.get_hip_loss_func(cfg, _ring())
    assert type(f) is st.HipCrossEntropy and f.label_smoothing == 0.2 and f.topk == 2
    with pytest.raises(ValueError, match="weight"):
        st.get_hip_loss_func(cfg, _ring(), class_weights=[1.0, 2.0, 3.0])
    np.random.seed(5)
    mix = m.sample(4, 16)
    assert mix.mode in (0, 1) and tuple(mix.partner) == (3, 2, 1, 0)
    cfg.MIXUP.ENABLE = False
    assert st.construct_hip_mixup(cfg) is None and st.get_hip_loss_func(cfg, _ring()).label_smoothing == 0.0


# ------------------------------------------------------------------------------------------------ the rows
def test_mix_rows_layout():
    ds = _ds()
    rows = ds.mix_rows(ds.MixParams((2, 1, 0), ds.MIX_CUTMIX, 0.75, (1, 2, 5, 6)))
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (3, 7) and rows.is_contiguous()
    assert rows.tolist() == [[2, 2, 0x3f400000, 1, 2, 5, 6], [1, 2, 0x3f400000, 1, 2, 5, 6], [0, 2, 0x3f400000, 1, 2, 5, 6]]
    # per-row values; lam is stored as the float32 nearest to the Python float
    rows = ds.mix_rows(ds.MixParams((1, 0), (0, 1), (1.0, 0.3), ((0, 0, 0, 0), (0, 0, 0, 0))))
    assert rows[0].tolist() == [1, 0, ONE, 0, 0, 0, 0]
    assert rows[1].tolist() == [0, 1, int(np.float32(0.3).view(np.uint32)), 0, 0, 0, 0]
    assert np.array_equal(rows.numpy(), ref.make_rows((1, 0), (0, 1), (1.0, 0.3)))
    assert float(ref.lam_of(rows[1, 2])) == float(np.float32(0.3))
    for bad in (ds.MixParams((1, 0), 3, 0.5, (0, 0, 0, 0)), ds.MixParams((1, 0), 1, 1.5, (0, 0, 0, 0)),
                ds.MixParams((1, 0), 1, float("nan"), (0, 0, 0, 0)), ds.MixParams((1, 0), (1,), 0.5, (0, 0, 0, 0)),
                ds.MixParams((1, 0), 1, 0.5, (0, 0, 0)), ds.MixParams((), 1, 0.5, (0, 0, 0, 0))):
        with pytest.raises(ValueError, match="mix_rows"):
            ds.mix_rows(bad)


def test_sample_mix_params_follows_upstreams_rule():
    ds = _ds()
    seen = set()
    for seed in range(60):
        B, crop = 2 + seed % 5, 7 + 3 * (seed % 4)
        np.random.seed(seed)
        mix = ds.sample_mix_params(B, crop, 0.8, 1.0, 1.0, 0.5)
        np.random.seed(seed)
        again = ds.sample_mix_params(B, crop, 0.8, 1.0, 1.0, 0.5)
        assert mix == again  # seeded draws are reproducible
        seen.add(mix.mode)
        assert tuple(mix.partner) == tuple(B - 1 - b for b in range(B)) and all(0 <= p < B for p in mix.partner)
        y0, x0, y1, x1 = mix.box
        assert 0 <= y0 <= y1 <= crop and 0 <= x0 <= x1 <= crop
        assert isinstance(mix.lam, float) and 0.0 <= mix.lam <= 1.0
        if mix.mode == ds.MIX_CUTMIX:
            assert mix.lam == 1.0 - (y1 - y0) * (x1 - x0) / float(crop * crop)  # the corrected lam, exactly
        else:
            assert mix.box == (0, 0, 0, 0)
        ds.mix_rows(mix)  # every draw gives rows the entries accept
    assert seen == {ds.MIX_MIXUP, ds.MIX_CUTMIX}
    # the documented order of the draws: rand() < prob, rand() < switch_prob, beta, then cy and cx
    np.random.seed(123)
    mix = ds.sample_mix_params(4, 32, 0.8, 1.0, 1.0, 1.0)  # switch_prob 1: always CutMix
    np.random.seed(123)
    assert np.random.rand() < 1.0 and np.random.rand() < 1.0
    lam = float(np.random.beta(1.0, 1.0))
    cut = int(32 * np.sqrt(1.0 - lam))
    cy, cx = int(np.random.randint(0, 32)), int(np.random.randint(0, 32))
    box = (int(np.clip(cy - cut // 2, 0, 32)), int(np.clip(cx - cut // 2, 0, 32)),
           int(np.clip(cy + cut // 2, 0, 32)), int(np.clip(cx + cut // 2, 0, 32)))
    assert mix.mode == ds.MIX_CUTMIX and mix.box == box
    # prob = 0: mode 0 with lam = 1, and only the first rand() is drawn
    np.random.seed(9)
    none = ds.sample_mix_params(5, 12, 0.8, 1.0, 0.0, 0.5)
    after = np.random.rand()
    np.random.seed(9)
    np.random.rand()
    assert none == ds.MixParams((4, 3, 2, 1, 0), ds.MIX_NONE, 1.0, (0, 0, 0, 0)) and after == np.random.rand()
    assert ds.mix_rows(none)[:, 1:].tolist() == [[0, ONE, 0, 0, 0, 0]] * 5
    # one alpha alone picks its form; neither: nothing is drawn
    np.random.seed(1)
    assert ds.sample_mix_params(3, 8, 0.8, 0.0, 1.0, 0.5).mode == ds.MIX_MIXUP
    assert ds.sample_mix_params(3, 8, 0.0, 1.0, 1.0, 0.5).mode == ds.MIX_CUTMIX
    state = np.random.get_state()[1].copy()
    assert ds.sample_mix_params(3, 8, 0.0, 0.0, 1.0, 0.5).mode == ds.MIX_NONE
    assert np.array_equal(state, np.random.get_state()[1])
    for kw in (dict(B=0), dict(crop=0), dict(mixup_alpha=-1.0), dict(prob=1.5), dict(switch_prob=-0.1)):
        args = dict(B=3, crop=8, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5)
        args.update(kw)
        with pytest.raises(ValueError, match="sample_mix_params"):
            ds.sample_mix_params(**args)


# ------------------------------------------------------------------------------------------------ the restatement
def _case(N, K, eps, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, K, generator=g, dtype=torch.float64) * 3.0
    y = torch.randint(0, K, (N,), generator=g)
    partner = torch.randperm(N, generator=g).tolist()
    lam = torch.rand(N, generator=g).tolist()
    if N > 1:
        lam[0], lam[1] = 0.0, 1.0
    rows = ref.make_rows(partner, 1, lam)
    return x, y, rows


@pytest.mark.parametrize("N", [1, 3, 65])
@pytest.mark.parametrize("K", [2, 27, 400])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_restatement_is_cross_entropy_with_dense_targets(N, K, eps):
    x, y, rows = _case(N, K, eps, N * 1000 + K)
    for r in (None, rows):
        t = torch.from_numpy(ref.dense_targets(y.numpy(), r, K, eps))
        assert torch.allclose(t.sum(dim=1), torch.ones(N, dtype=torch.float64), atol=1e-14)
        xr = x.clone().requires_grad_(True)
        want = F.cross_entropy(xr, t)
        want.backward()
        want = want.detach()
        loss, d, bad = ref.ce_mix(x.numpy(), y.numpy(), r, eps)
        assert bad == 0
        assert abs(loss - float(want)) <= 1e-13 * max(1.0, abs(float(want)))
        assert float(np.abs(d - xr.grad.numpy()).max()) <= 1e-15
        # upstream's form: lam CE(a) + (1 - lam) CE(b), each with label_smoothing = eps
        if r is not None:
            lam = torch.tensor([float(ref.lam_of(b)) for b in r[:, 2]], dtype=torch.float64)
            yb = y[torch.from_numpy(r[:, 0])]
            up = (lam * F.cross_entropy(x, y, label_smoothing=eps, reduction="none") +
                  (1.0 - lam) * F.cross_entropy(x, yb, label_smoothing=eps, reduction="none")).mean()
            assert abs(loss - float(up)) <= 1e-13 * max(1.0, abs(float(up)))
    # without mixing and smoothing: plain cross-entropy, and the hits are torch.topk's
    if eps == 0.0:
        loss, _, _ = ref.ce_mix(x.numpy(), y.numpy(), None, 0.0)
        assert abs(loss - float(F.cross_entropy(x, y))) <= 1e-13 * max(1.0, loss)
        k = min(5, K)
        top = torch.topk(x, k, dim=1).indices
        h1 = int((top[:, 0] == y).sum())
        hk = int((top == y[:, None]).any(dim=1).sum())
        assert ref.hit_counts(x.numpy(), y.numpy(), None, k) == (h1, hk)


def test_restatement_of_bad_rows_and_of_pixel_mixing():
    x = np.arange(12, dtype=np.float64).reshape(3, 4) / 7.0
    y = np.array([1, 9, 2])
    rows = ref.make_rows([1, 0, 5], 1, [0.25, 0.5, 0.5])
    loss, d, bad = ref.ce_mix(x, y, rows, 0.1)
    assert bad == 3 and loss == 0.0 and not d.any()  # row 0: b = 9; row 1: a = 9; row 2: partner 5 of 3 rows
    assert ref.hit_counts(x, y, rows, 2) == (0, 0)
    rows = ref.make_rows([2, 1, 0], 1, [0.25, 0.5, 0.75])
    y = np.array([1, 3, 2])
    assert ref.dominant_labels(y, rows).tolist() == [2, 3, 2]  # lam = 0.25: the partner's label; 0.5: its own
    # pixel mixing on a [B, T, Hp, Wp, C] batch: mode 2 moves the box, offset by the border; mode 1 is float32 arithmetic
    xb = np.random.RandomState(0).randn(2, 1, 6, 7, 1).astype(np.float32)
    xb[:, :, :1], xb[:, :, 5:], xb[:, :, :, :2], xb[:, :, :, 6:] = 0, 0, 0, 0  # crop 4, ph 1, pw 2, Wp 7
    cut = ref.mix_batch(xb, ref.make_rows([1, 0], [2, 0], [0.75, 1.0], [(1, 0, 3, 2), (0, 0, 0, 0)]), 4, 1, 2)
    assert np.array_equal(cut[1], xb[1]) and np.array_equal(cut[0, :, 2:4, 2:4], xb[1, :, 2:4, 2:4])
    keep = np.ones_like(xb[0], dtype=bool)
    keep[:, 2:4, 2:4] = False
    assert np.array_equal(cut[0][keep], xb[0][keep])
    mixed = ref.mix_batch(xb, ref.make_rows([1, 0], 1, 0.3), 4, 1, 2)
    lam = np.float32(0.3)
    assert np.array_equal(mixed[0], lam * xb[0] + (np.float32(1) - lam) * xb[1]) and mixed.dtype == np.float32
    assert not mixed[:, :, :1].any() and not mixed[:, :, :, :2].any()
