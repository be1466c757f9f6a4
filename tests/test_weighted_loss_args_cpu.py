"""Host side of the class-weighted losses (sf_ce_topk_w, sf_bce_w, sf_class_weights; slowfast/models/step_tail.py,
DevicePerClassMeter.class_weights): every refusal — decided before any launch, so callable without a GPU — what
get_hip_loss_func returns, the binding's rows, and the numpy restatement of the two weight schemes
(tests/_class_weights_ref.py) against scikit-learn and closed forms."""
import ctypes

import numpy as np
import pytest
import torch

import _class_weights_ref as ref

FAKE = 0x7f0000001000  # a non-null, 16-byte aligned "device address": a refused call never dereferences it


def _st():
    from slowfast.models import step_tail
    return step_tail


def _cfg(name, K=3, topk=2):
    from slowfast.config.defaults import get_cfg
    cfg = get_cfg()
    cfg.MODEL.LOSS_FUNC, cfg.MODEL.NUM_CLASSES, cfg.TRAIN.TOPK = name, K, topk
    return cfg


def _ring():
    return _st().StatsRing(4, device="cpu")


# ------------------------------------------------------------------------------------------------ the binding
def test_signature_table_has_the_new_symbols():
    import sfhip
    vp, ci, pi = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    want = {"sf_ce_topk_w": (ci, [vp, ci, vp, vp, ci, ci, ci, vp, vp, pi, ci, vp, vp]),
            "sf_bce_w": (ci, [vp, ci, vp, ci, vp, vp, ci, ci, ci, vp, vp, pi, ci, vp, vp]),
            "sf_class_weights": (ci, [vp, ci, ci, vp, vp, vp])}
    for name, sig in want.items():
        assert sfhip._SIGNATURES[name] == sig, name
        assert name in sfhip.EXPORTS and hasattr(sfhip.lib(), name)
    assert sfhip.WEIGHT_SCHEMES == {"balanced": 0, "effective": 1}


# ------------------------------------------------------------------------------------------------ C refusals
def _ce_w_rc(N=4, K=10, k_hi=5, ld=None, cap=3, null=None):
    import sfhip
    p = ctypes.c_void_p(FAKE)
    cnt = ctypes.cast(ctypes.c_void_p(FAKE), sfhip._pi)
    args = [p, K if ld is None else ld, p, p, N, K, k_hi, p, p, cnt, cap, p, None]
    if null is not None:
        args[null] = None
    return sfhip.lib().sf_ce_topk_w(*args)


def test_ce_topk_w_refusals():
    import sfhip
    E = sfhip.SF_EINVAL
    assert _ce_w_rc(k_hi=11) == E and _ce_w_rc(k_hi=0) == E
    assert _ce_w_rc(N=0) == E and _ce_w_rc(N=-1) == E
    assert _ce_w_rc(K=0, k_hi=0) == E and _ce_w_rc(K=-3, k_hi=1) == E
    assert _ce_w_rc(cap=0) == E and _ce_w_rc(cap=-1) == E
    assert _ce_w_rc(ld=9) == E
    for null in (0, 2, 3, 7, 8, 9, 11):  # logits, labels, weight, dlogits, ring, counter, loss_out
        assert _ce_w_rc(null=null) == E, null


def _bce_w_rc(N=4, K=10, ldx=None, ldy=None, cap=3, from_logits=1, weight=True, pos=True, null=None):
    import sfhip
    p = ctypes.c_void_p(FAKE)
    cnt = ctypes.cast(ctypes.c_void_p(FAKE), sfhip._pi)
    args = [p, K if ldx is None else ldx, p, K if ldy is None else ldy, p if weight else None, p if pos else None, N, K,
            from_logits, p, p, cnt, cap, p, None]
    if null is not None:
        args[null] = None
    return sfhip.lib().sf_bce_w(*args)


def test_bce_w_refusals():
    import sfhip
    E = sfhip.SF_EINVAL
    assert _bce_w_rc(N=0) == E and _bce_w_rc(K=0) == E and _bce_w_rc(cap=0) == E
    assert _bce_w_rc(ldx=9) == E and _bce_w_rc(ldy=9) == E
    assert _bce_w_rc(from_logits=2) == E and _bce_w_rc(from_logits=-1) == E
    for null in (0, 2, 9, 10, 11, 13):  # x, y, dx, ring, counter, loss_out — the two weight vectors may be null
        assert _bce_w_rc(null=null) == E, null
    # pos_weight on probabilities: torch has no such thing — refused whether or not a weight comes with it
    assert _bce_w_rc(from_logits=0, pos=True) == E and _bce_w_rc(from_logits=0, pos=True, weight=False) == E


def _cw_rc(K=3, scheme=0, beta=0.99, conf=FAKE, w=FAKE):
    import sfhip
    b = ctypes.c_double(beta) if beta is not None else None
    return sfhip.lib().sf_class_weights(ctypes.c_void_p(conf) if conf else None, K, scheme,
                                        ctypes.byref(b) if b is not None else None,
                                        ctypes.c_void_p(w) if w else None, None)


def test_class_weights_refusals():
    import sfhip
    E = sfhip.SF_EINVAL
    assert _cw_rc(K=0) == E and _cw_rc(K=-1) == E and _cw_rc(K=1025) == E
    assert _cw_rc(conf=0) == E and _cw_rc(w=0) == E
    assert _cw_rc(scheme=2) == E and _cw_rc(scheme=-1) == E
    for beta in (None, 0.0, 1.0, -0.5, 1.5, float("nan")):
        assert _cw_rc(scheme=1, beta=beta) == E, beta
    assert _cw_rc(conf=FAKE + 4) == sfhip.SF_EALIGN and _cw_rc(w=FAKE + 2) == sfhip.SF_EALIGN
    # the Python wrappers: the scheme and beta before anything needs the GPU
    conf = torch.zeros((3, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="scheme"):
        sfhip.class_weights(conf, scheme="inverse")
    for beta in (None, 0.0, 1.0, 2.0):
        with pytest.raises(ValueError, match="beta"):
            sfhip.class_weights(conf, scheme="effective", beta=beta)
    with pytest.raises(ValueError, match="beta"):
        sfhip.class_weights(conf, scheme="balanced", beta=0.9)
    with pytest.raises(ValueError):
        sfhip.class_weights(torch.zeros((3, 4), dtype=torch.int64))
    with pytest.raises(sfhip.SfhipError):  # counters on the CPU: there is no fallback
        sfhip.class_weights(conf)
    from slowfast.utils.meters import DevicePerClassMeter
    m = DevicePerClassMeter(3, 2, device="cpu")
    with pytest.raises(ValueError, match="scheme"):
        m.class_weights(scheme="nope")
    with pytest.raises(sfhip.SfhipError):
        m.class_weights()
    assert "all_reduce" in DevicePerClassMeter.class_weights.__doc__


# ------------------------------------------------------------------------------------------------ Python refusals
def test_weight_tensors_are_checked_before_the_gpu_is_needed():
    import sfhip
    st = _st()
    ring, out = _ring(), torch.zeros(2)
    x, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    t = torch.zeros(4, 3)
    bad = {"dtype": torch.ones(3, dtype=torch.float64), "length": torch.ones(4), "shape": torch.ones(3, 1),
           "strided": torch.ones(6)[::2], "device": torch.ones(3, device="meta"), "not a tensor": [1.0, 1.0, 1.0]}
    for what, w in bad.items():
        with pytest.raises(ValueError, match="weight"):
            st.ce_topk_w(x, y, w, 2, ring, out)
        with pytest.raises(ValueError, match="weight"):
            st.bce_w(x, t, True, ring, out, weight=w)
        with pytest.raises(ValueError, match="pos_weight"):
            st.bce_w(x, t, True, ring, out, pos_weight=w)
    with pytest.raises(ValueError, match="pos_weight"):
        st.bce_w(x, t, False, ring, out, pos_weight=torch.ones(3))
    with pytest.raises(ValueError):
        st.ce_topk_w(x, torch.zeros(5, dtype=torch.int64), torch.ones(3), 2, ring, out)
    with pytest.raises(ValueError):
        st.bce_w(x, torch.zeros(4, 2), True, ring, out, weight=torch.ones(3))
    # good weights on CPU predictions: the same refusal ce_topk / bce give — no fallback
    with pytest.raises(sfhip.SfhipError):
        st.ce_topk_w(x, y, torch.ones(3), 2, ring, out)
    with pytest.raises(sfhip.SfhipError):
        st.bce_w(x, t, True, ring, out, weight=torch.ones(3), pos_weight=torch.ones(3))


def test_loss_objects_check_their_weights_at_construction():
    st = _st()
    ring = _ring()
    for cls, args in ((st.HipCrossEntropy, (2, ring)), (st.HipBCE, (ring,)), (st.HipBCEWithLogits, (ring,))):
        for w in (torch.ones(3, dtype=torch.float64), torch.ones(3, 1), torch.ones(6)[::2], torch.ones(3, device="meta"),
                  [1.0, -0.5, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf")], np.array([[1.0, 2.0]]), [], "abc"):
            with pytest.raises(ValueError, match="weight"):
                cls(*args, weight=w)
    for w in ([1.0, -1.0], torch.ones(2, dtype=torch.float16)):
        with pytest.raises(ValueError, match="pos_weight"):
            st.HipBCEWithLogits(ring, pos_weight=w)
    with pytest.raises(ValueError, match="pos_weight"):
        st.HipBCE(ring, pos_weight=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="topk"):
        st.HipCrossEntropy(0, ring, weight=[1.0])
    # a tensor is kept by reference, a host sequence is uploaded once as float32
    w = torch.tensor([2.0, 3.0, 1.0])
    ce = st.HipCrossEntropy(2, ring, weight=w)
    assert ce.weight is w
    up = st.HipCrossEntropy(2, ring, weight=np.array([2, 3, 1]))
    assert up.weight.dtype == torch.float32 and up.weight.tolist() == [2.0, 3.0, 1.0]
    assert st.HipCrossEntropy(2, ring, weight=[0.0, 1.0]).weight.tolist() == [0.0, 1.0]  # zero is a legal weight
    # set_weight is a copy_ into the same storage; another shape is refused
    ce.set_weight(torch.tensor([1.0, 1.0, 5.0]))
    assert ce.weight is w and w.tolist() == [1.0, 1.0, 5.0]
    with pytest.raises(ValueError, match="shape"):
        ce.set_weight(torch.ones(4))
    with pytest.raises(ValueError):
        st.HipCrossEntropy(2, ring).set_weight(torch.ones(3))
    b = st.HipBCEWithLogits(ring, weight=[1.0, 2.0], pos_weight=[3.0, 4.0])
    b.set_weight(torch.tensor([5.0, 6.0]))
    b.set_pos_weight(torch.tensor([7.0, 8.0]))
    assert b.weight.tolist() == [5.0, 6.0] and b.pos_weight.tolist() == [7.0, 8.0]
    with pytest.raises(ValueError):
        st.HipBCEWithLogits(ring, weight=[1.0, 2.0]).set_pos_weight(torch.ones(2))
    # without weights the objects hold none: they launch what they launched before
    assert st.HipCrossEntropy(2, ring).weight is None
    assert st.HipBCE(ring).weight is None and st.HipBCE(ring).pos_weight is None
    assert "DDP" in st.HipCrossEntropy.__doc__


def test_get_hip_loss_func_with_and_without_weights():
    st = _st()
    ring = _ring()
    kinds = {"cross_entropy": st.HipCrossEntropy, "bce": st.HipBCE, "bce_logit": st.HipBCEWithLogits}
    for name, cls in kinds.items():
        f = st.get_hip_loss_func(_cfg(name), ring)
        assert type(f) is cls and f.weight is None
        g = st.get_hip_loss_func(_cfg(name), ring, class_weights=[2.0, 3.0, 1.0])
        assert type(g) is cls and g.weight.tolist() == [2.0, 3.0, 1.0]
    f = st.get_hip_loss_func(_cfg("cross_entropy"), ring)
    assert f.topk == 2
    w = torch.tensor([2.0, 3.0, 1.0])
    f = st.get_hip_loss_func(_cfg("cross_entropy_weighted"), ring, class_weights=w)
    assert type(f) is st.HipCrossEntropy and f.weight is w and f.topk == 2
    with pytest.raises(ValueError, match="class_weights"):
        st.get_hip_loss_func(_cfg("cross_entropy_weighted"), ring)
    f = st.get_hip_loss_func(_cfg("bce_logit"), ring, pos_weight=[1.0, 2.0, 3.0])
    assert type(f) is st.HipBCEWithLogits and f.weight is None and f.pos_weight.tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="pos_weight"):
        st.get_hip_loss_func(_cfg("bce"), ring, pos_weight=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="pos_weight"):
        st.get_hip_loss_func(_cfg("cross_entropy"), ring, pos_weight=[1.0, 2.0, 3.0])
    for name in kinds:  # a length other than MODEL.NUM_CLASSES
        with pytest.raises(ValueError, match="NUM_CLASSES"):
            st.get_hip_loss_func(_cfg(name), ring, class_weights=[1.0, 2.0])
    with pytest.raises(NotImplementedError, match="Loss focal is not supported"):
        st.get_hip_loss_func(_cfg("focal"), ring)
    # no config key was added for the weights
    from slowfast.config.defaults import get_cfg
    assert not any("WEIGHT" in k and "CLASS" in k for k in get_cfg().MODEL)


# ------------------------------------------------------------------------------------------------ the weight schemes
SUPPORTS = [[5, 1, 0, 14], [3, 3, 3], [0, 0, 7], [1], [1000000, 1, 20, 0, 0, 300]]


@pytest.mark.parametrize("support", SUPPORTS, ids=[str(s) for s in SUPPORTS])
def test_balanced_restatement_is_scikit_learns(support):
    from sklearn.utils.class_weight import compute_class_weight
    support = np.asarray(support)
    present = np.nonzero(support)[0]
    y = np.repeat(np.arange(len(support)), support)
    want = compute_class_weight("balanced", classes=present, y=y)
    got = ref.balanced(support)
    assert got.dtype == np.float32 and got.shape == support.shape
    assert np.array_equal(got[present], want.astype(np.float32))
    assert np.all(got[support == 0] == 0.0)


def test_balanced_and_effective_of_nothing_are_zero():
    assert ref.balanced([0, 0, 0]).tolist() == [0.0, 0.0, 0.0]
    assert ref.effective([0, 0, 0], 0.9).tolist() == [0.0, 0.0, 0.0]


def test_effective_restatement_against_closed_forms():
    # equal supports: every class with support weighs 1, whatever beta
    for beta in (0.5, 0.9, 0.999):
        w = ref.effective([7, 0, 7, 7], beta)
        assert w.dtype == np.float32 and w.tolist() == [1.0, 0.0, 1.0, 1.0]
    # supports 1 and 2 at beta = 1/2: e = (1, 2/3) -> weights (6/5, 4/5)
    w = ref.effective([1, 2], 0.5)
    assert w.tolist() == [float(np.float32(1.2)), float(np.float32(0.8))]
    # supports 1, 3 and nothing at beta = 1/2: e = (1, 4/7) -> 2 / (11/7) * e = (14/11, 8/11)
    w = ref.effective([1, 0, 3], 0.5)
    assert np.array_equal(w, np.array([14.0 / 11.0, 0.0, 8.0 / 11.0]).astype(np.float32))
    # the weights over the classes with support sum to their number; rarer classes weigh more
    sup = np.array([1000, 10, 0, 1, 250])
    for beta in (0.9, 0.99, 0.9999):
        w = ref.effective(sup, beta).astype(np.float64)
        assert abs(w.sum() - 4.0) < 1e-6 and w[2] == 0.0
        assert w[3] > w[1] > w[4] >= w[0] > 0.0
    # beta -> 1 approaches inverse frequency (= balanced); beta -> 0 approaches uniform
    near1 = ref.effective(sup, 1.0 - 1e-9).astype(np.float64)
    inv = np.where(sup > 0, 1.0 / np.maximum(sup, 1), 0.0)
    assert np.allclose(near1, inv * 4.0 / inv.sum(), rtol=1e-4)
    assert np.allclose(ref.effective(sup, 1e-9)[sup > 0], 1.0, rtol=1e-6)
