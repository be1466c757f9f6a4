"""sf_ce_topk_w, sf_bce_w and sf_class_weights on the GPU (csrc/step_tail.hip, csrc/class_report.hip) through
slowfast/models/step_tail.py, sfhip.class_weights and DevicePerClassMeter.class_weights.

Parity is against float64 on the CPU; the bound is the project's rule from test_step_tail_ops_gpu.py: what torch's own
float32 GPU kernels (F.cross_entropy(weight=), F.binary_cross_entropy(weight=),
F.binary_cross_entropy_with_logits(weight=, pos_weight=)) miss the same float64 values by, on the same inputs, times 2 —
measured in the test itself, with no absolute floor (that file has none: where torch is exact, so is this library).
Every case prints both errors and appends them to the run's report (weighted_loss_report.txt beside the other GPU
reports, through test_backward_ops_gpu's helper); the figures measured on an MI355X are in profiles/weighted_loss.txt.  Worst cases there:
    cross-entropy loss      1.5e-6 (torch 2.3e-6) with a row of +-80 at N = 8, K = 400; else 4.6e-7 (4.6e-7) at N = 65, K = 400
    cross-entropy dlogits   2.7e-8 (4.4e-8) at N = 3, K = 400; no case above torch's own error
    BCE loss                6.6e-7 (6.6e-7), logits of +-100 with weight and pos_weight
    BCE gradient            7.1e-7 (1.2e-6), probabilities with weight at 5 x 80; 2.9e2 (2.9e2) on gradients of 1e12 where
                            a probability is exactly 0 or 1 (the 1e-12 clamp of the denominator)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _class_weights_ref as cw_ref

pytestmark = pytest.mark.gpu
MARGIN, SENTINEL = 256, -777.0


def _mods():
    from slowfast.models import step_tail
    return step_tail


def _report(kind, name, e_loss, t_e_loss, e_grad, t_e_grad):
    """Print the case's errors (torch's own in brackets) and keep the four figures in the run's report, where the other
    GPU tests keep theirs."""
    from test_backward_ops_gpu import _report as report
    print("%s %-32s loss err %.3e (torch %.3e)  gradient err %.3e (torch %.3e)" % (kind, name, e_loss, t_e_loss, e_grad,
                                                                                  t_e_grad))
    for what, v in (("loss", e_loss), ("loss (torch)", t_e_loss), ("gradient", e_grad), ("gradient (torch)", t_e_grad)):
        report("%s %s %s" % (kind, name, what), v, "weighted_loss_report.txt")


def _guarded(shape):
    """A NaN-filled buffer of `shape` between two sentinel margins -> (whole allocation, the buffer's view)."""
    n = int(np.prod(shape))
    whole = torch.full((MARGIN + n + MARGIN,), SENTINEL, dtype=torch.float32, device="cuda")
    whole[MARGIN:MARGIN + n] = float("nan")
    return whole, whole[MARGIN:MARGIN + n].view(shape)


def _margins_intact(whole):
    return bool((whole[:MARGIN] == SENTINEL).all()) and bool((whole[-MARGIN:] == SENTINEL).all())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class _Owned(object):
    """dlogits [N, K], ring rows [cap, 8] and out [2] as NaN-filled buffers between sentinel margins."""

    def __init__(self, N, K, cap=3):
        st = _mods()
        self.wd, self.d = _guarded((N, K))
        self.wr, rows = _guarded((cap, 8))
        self.wo, self.out = _guarded((2,))
        self.ring = st.StatsRing(cap)
        self.ring.rows = rows

    def check(self):
        torch.cuda.synchronize()
        assert _margins_intact(self.wd) and _margins_intact(self.wr) and _margins_intact(self.wo)
        return self.d, self.ring, self.out


def _run_ce_w(logits, labels, weight, k_hi, cap=3):
    N, K = logits.shape
    o = _Owned(N, K, cap)
    _mods().ce_topk_w(logits, labels, weight, k_hi, o.ring, o.out, dlogits=o.d)
    return o.check()


def _run_ce(logits, labels, k_hi, cap=3):
    N, K = logits.shape
    o = _Owned(N, K, cap)
    _mods().ce_topk(logits, labels, k_hi, o.ring, o.out, dlogits=o.d)
    return o.check()


def _run_bce_w(x, y, from_logits, weight=None, pos_weight=None, cap=3):
    N, K = x.shape
    o = _Owned(N, K, cap)
    _mods().bce_w(x, y, from_logits, o.ring, o.out, weight=weight, pos_weight=pos_weight, dgrad=o.d)
    return o.check()


def _run_bce(x, y, from_logits, cap=3):
    N, K = x.shape
    o = _Owned(N, K, cap)
    _mods().bce(x, y, from_logits, o.ring, o.out, dgrad=o.d)
    return o.check()


def _weights(K, g):
    return torch.rand(K, generator=g) * 3.75 + 0.25  # [0.25, 4]


# ------------------------------------------------------------------------------------------------ CE parity
def _ce_cases():
    cases = []
    for N in (1, 3, 17, 65):          # 17 and 65 cross the 16-wavefront row stride
        for K in (1, 2, 27, 65, 400):  # 65 crosses the 64-lane sweep
            cases.append(("n%d_k%d" % (N, K), N, K, 0, None))
    cases.append(("n8_k27_stride", 8, 27, 3, None))
    cases.append(("n8_k400_pm80", 8, 400, 0, "big"))
    cases.append(("n17_k27_zero_weight_class", 17, 27, 0, "zero"))
    return cases


@pytest.mark.parametrize("name,N,K,pad,special", _ce_cases(), ids=[c[0] for c in _ce_cases()])
def test_weighted_ce_matches_float64_within_twice_torchs_own_error(name, N, K, pad, special):
    g = torch.Generator().manual_seed(N * 1000 + K)
    x = torch.randn(N, K + pad, generator=g) * 3.0
    if special == "big":  # one row near +-80: exp() of the raw values would overflow float32
        x[2] = torch.where(torch.rand(K, generator=g) < 0.5, torch.tensor(80.0), torch.tensor(-80.0)) + \
            torch.randn(K, generator=g) * 0.01
    y = torch.randint(0, K, (N,), generator=g)
    w = _weights(K, g)
    if special == "zero":  # a class that is present in the batch weighs nothing (other classes are present too)
        w[int(y[0])] = 0.0
        assert int((y != y[0]).sum()) > 0
    x64 = x[:, :K].double().requires_grad_(True)
    ref_loss = F.cross_entropy(x64, y, weight=w.double())
    ref_loss.backward()
    xg = x.cuda()[:, :K].detach().requires_grad_(True)  # the same strided view on the GPU
    t_loss = F.cross_entropy(xg, y.cuda(), weight=w.cuda())
    t_loss.backward()
    d, ring, out = _run_ce_w(x.cuda()[:, :K], y.cuda(), w.cuda(), min(5, K))
    e_loss = abs(float(out[0].double().cpu()) - float(ref_loss.detach()))
    t_e_loss = abs(float(t_loss.detach().double().cpu()) - float(ref_loss.detach()))
    e_grad = float((d.double().cpu() - x64.grad).abs().max())
    t_e_grad = float((xg.grad.double().cpu() - x64.grad).abs().max())
    _report("ce_w", name, e_loss, t_e_loss, e_grad, t_e_grad)
    assert e_loss <= 2 * t_e_loss and e_grad <= 2 * t_e_grad
    if special == "zero":
        zero_rows = (y == y[0]).cuda()
        assert bool((d[zero_rows] == 0).all()) and float(ring.rows[0, 5]) == 0.0  # nothing from them; not "bad"
    row = ring.rows[0].tolist()
    assert row[0] == float(out[0]) and row[3] == 0.0 == float(out[1]) and row[4] == N and row[5] == 0.0
    assert row[6] == 0.0 == row[7]  # KIND_CE
    # the errors are unweighted: what ce_topk counts on the same rows
    _, ring0, _ = _run_ce(x.cuda()[:, :K], y.cuda(), min(5, K))
    assert row[1:3] == ring0.rows[0, 1:3].tolist()


# ------------------------------------------------------------------------------------------------ bitwise identities
@pytest.mark.parametrize("N,K", [(8, 27), (65, 400)])
def test_all_ones_weights_give_ce_topks_bits(N, K):
    g = torch.Generator().manual_seed(N + K)
    x = (torch.randn(N, K, generator=g) * 3.0).cuda()
    y = torch.randint(0, K, (N,), generator=g).cuda()
    d0, ring0, out0 = _run_ce(x, y, 5)
    d1, ring1, out1 = _run_ce_w(x, y, torch.ones(K, device="cuda"), 5)
    assert _same_bits(d0, d1) and _same_bits(out0, out1) and _same_bits(ring0.rows[0], ring1.rows[0])
    assert bool(torch.isnan(ring1.rows[1:]).all())  # only row 0 was written
    # and the same call twice gives equal bits
    w = _weights(K, g).cuda()
    a, b = _run_ce_w(x, y, w, 5), _run_ce_w(x, y, w, 5)
    assert _same_bits(a[0], b[0]) and _same_bits(a[2], b[2]) and _same_bits(a[1].rows[0], b[1].rows[0])
    assert not _same_bits(a[0], d0)


@pytest.mark.parametrize("from_logits", [False, True], ids=["bce", "bce_logit"])
def test_null_or_all_ones_vectors_give_bces_bits(from_logits):
    g = torch.Generator().manual_seed(11)
    N, K = 5, 80
    x = torch.randn(N, K, generator=g) * 3.0
    x = (x if from_logits else torch.sigmoid(x)).cuda()
    y = torch.rand(N, K, generator=g).cuda()
    ones = torch.ones(K, device="cuda")
    d0, ring0, out0 = _run_bce(x, y, from_logits)
    variants = [dict(), dict(weight=ones)]
    if from_logits:
        variants += [dict(pos_weight=ones), dict(weight=ones, pos_weight=ones)]
    for kw in variants:
        d1, ring1, out1 = _run_bce_w(x, y, from_logits, **kw)
        assert _same_bits(d0, d1) and _same_bits(out0, out1) and _same_bits(ring0.rows[0], ring1.rows[0]), kw
    w, p = _weights(K, g).cuda(), _weights(K, g).cuda()
    kw = dict(weight=w, pos_weight=p) if from_logits else dict(weight=w)
    a, b = _run_bce_w(x, y, from_logits, **kw), _run_bce_w(x, y, from_logits, **kw)
    assert _same_bits(a[0], b[0]) and _same_bits(a[2], b[2]) and _same_bits(a[1].rows[0], b[1].rows[0])
    assert not _same_bits(a[0], d0)


# ------------------------------------------------------------------------------------------------ rules
def test_bad_labels_are_left_out_whole_even_with_a_nan_in_their_rows():
    g = torch.Generator().manual_seed(6)
    N, K = 6, 27
    x = torch.randn(N, K, generator=g)
    y = torch.randint(0, K, (N,), generator=g)
    w = _weights(K, g)
    w[0], w[K - 1] = 1000.0, 1000.0  # would show in W if index -1 / K were clamped into the vector
    xb, yb = x.clone(), y.clone()
    yb[1], yb[4] = -1, K
    xb[1, 3], xb[4, 0] = float("nan"), float("inf")
    d, ring, out = _run_ce_w(xb.cuda(), yb.cuda(), w.cuda(), 5)
    keep = [0, 2, 3, 5]
    assert bool((d[1] == 0).all()) and bool((d[4] == 0).all())  # zeros, not NaN
    row = ring.rows[0].tolist()
    assert row[5] == 2.0 and row[4] == N
    assert row[3] == 0.0 == float(out[1])  # the flag is not changed by rows that are left out
    x64 = x[keep].double().requires_grad_(True)
    want = F.cross_entropy(x64, y[keep], weight=w.double())  # W is the kept rows' weight alone
    want.backward()
    assert abs(float(out[0]) - float(want.detach())) <= 1e-6 * float(want.detach())
    assert float((d[keep].double().cpu() - x64.grad).abs().max()) <= 1e-7
    # both rows count as wrong: the top-1 error is at least 2 of 6
    assert row[1] >= float((1.0 - torch.tensor(4.0) / N) * 100.0)


def test_zero_total_weight_gives_nan_loss_flag_and_zero_gradient():
    g = torch.Generator().manual_seed(7)
    N, K = 5, 9
    x = torch.randn(N, K, generator=g).cuda()
    y = torch.tensor([2, 2, 7, 2, 7]).cuda()
    w = _weights(K, g)
    w[2], w[7] = 0.0, 0.0  # every class that is present weighs nothing
    assert bool(torch.isnan(F.cross_entropy(x.cpu().double(), y.cpu(), weight=w.double())))  # torch: 0 / 0
    d, ring, out = _run_ce_w(x, y, w.cuda(), 5)
    assert bool(torch.isnan(out[0])) and float(out[1]) == 1.0
    assert bool(torch.isnan(ring.rows[0, 0])) and float(ring.rows[0, 3]) == 1.0 and float(ring.rows[0, 5]) == 0.0
    assert bool((d.view(torch.int32) == 0).all())  # +0.0 everywhere: no NaN reaches a gradient


def test_nan_logit_in_a_valid_row_sets_the_flag():
    g = torch.Generator().manual_seed(8)
    N, K = 4, 27
    x = torch.randn(N, K, generator=g)
    y = torch.randint(0, K, (N,), generator=g)
    w = _weights(K, g).cuda()
    clean = _run_ce_w(x.cuda(), y.cuda(), w, 5)
    assert float(clean[2][1]) == 0.0
    for poison in (float("nan"), float("inf")):
        xb = x.clone()
        xb[1, 3] = poison
        d, ring, out = _run_ce_w(xb.cuda(), y.cuda(), w, 5)
        assert float(out[1]) == 1.0 == float(ring.rows[0, 3]) and float(ring.rows[0, 5]) == 0.0
        assert not bool(torch.isfinite(out[0]))
        assert _same_bits(d[[0, 2, 3]], clean[0][[0, 2, 3]])  # the other rows: the clean run's gradients


def test_ring_counter_advances_and_slots_wrap():
    st = _mods()
    ring = st.StatsRing(3)
    out = torch.zeros(2, device="cuda")
    g = torch.Generator().manual_seed(9)
    w = _weights(9, g).cuda()
    losses = []
    for i in range(4):
        x = torch.randn(4, 9, generator=g)
        y = torch.randint(0, 9, (4,), generator=g)
        st.ce_topk_w(x.cuda(), y.cuda(), w, 5, ring, out)
        assert int(ring.counter[0]) == i + 1
        losses.append(float(out[0]))
    rows = ring.rows.cpu()  # steps 0..3 landed in rows 0, 1, 2, 0
    assert [float(rows[0, 0]), float(rows[1, 0]), float(rows[2, 0])] == [losses[3], losses[1], losses[2]]
    assert len(set(losses)) == 4
    for i in range(4):  # the BCE form shares the protocol (kind 1)
        x = torch.randn(4, 9, generator=g)
        st.bce_w(x.cuda(), torch.rand(4, 9, generator=g).cuda(), True, ring, out, weight=w)
        assert int(ring.counter[0]) == 5 + i and float(ring.rows[(4 + i) % 3, 6]) == 1.0


# ------------------------------------------------------------------------------------------------ BCE parity
BCE_MODES = {"prob_weight": (False, True, False), "logit_weight": (True, True, False),
             "logit_pos": (True, False, True), "logit_both": (True, True, True)}


def _torch_bce(x, y, from_logits, w, p):
    if from_logits:
        return F.binary_cross_entropy_with_logits(x, y, weight=w, pos_weight=p)
    return F.binary_cross_entropy(x, y, weight=w)


def _bce_cases():
    cases = []
    for mode in BCE_MODES:
        for N, K, pad in ((1, 1, 0), (5, 80, 0), (13, 157, 0), (5, 80, 3)):
            cases.append(("%s_n%d_k%d%s" % (mode, N, K, "_stride" if pad else ""), mode, N, K, pad, None))
    cases.append(("prob_weight_p_exactly_0_and_1", "prob_weight", 4, 80, 0, "ends"))
    cases.append(("logit_both_pm100", "logit_both", 5, 80, 0, "big"))
    return cases


@pytest.mark.parametrize("name,mode,N,K,pad,special", _bce_cases(), ids=[c[0] for c in _bce_cases()])
def test_weighted_bce_matches_float64_within_twice_torchs_own_error(name, mode, N, K, pad, special):
    from_logits, has_w, has_p = BCE_MODES[mode]
    g = torch.Generator().manual_seed(N * 1000 + K + len(mode))
    x = torch.randn(N, K + pad, generator=g) * 3.0
    if not from_logits:
        x = torch.sigmoid(x)
    y = (torch.rand(N, K + pad, generator=g) < 0.3).float()
    if special == "ends":  # the -100 clamp of the logs and the 1e-12 clamp of the gradient, against both targets
        x[0, 0:4] = torch.tensor([0.0, 0.0, 1.0, 1.0])
        y[0, 0:4] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    if special == "big":  # exp() of the raw values would overflow float32
        x[2] = torch.where(torch.rand(K + pad, generator=g) < 0.5, torch.tensor(100.0), torch.tensor(-100.0))
    w = _weights(K, g) if has_w else None
    p = _weights(K, g) if has_p else None
    dbl = lambda t: None if t is None else t.double()
    gpu = lambda t: None if t is None else t.cuda()
    x64 = x[:, :K].double().requires_grad_(True)
    ref_loss = _torch_bce(x64, y[:, :K].double(), from_logits, dbl(w), dbl(p))
    ref_loss.backward()
    xg = x.cuda()[:, :K].detach().requires_grad_(True)  # the same strided views on the GPU
    yg = y.cuda()[:, :K]
    t_loss = _torch_bce(xg, yg, from_logits, gpu(w), gpu(p))
    t_loss.backward()
    d, ring, out = _run_bce_w(x.cuda()[:, :K], yg, from_logits, weight=gpu(w), pos_weight=gpu(p))
    e_loss = abs(float(out[0].double().cpu()) - float(ref_loss.detach()))
    t_e_loss = abs(float(t_loss.detach().double().cpu()) - float(ref_loss.detach()))
    e_grad = float((d.double().cpu() - x64.grad).abs().max())
    t_e_grad = float((xg.grad.double().cpu() - x64.grad).abs().max())
    _report("bce_w", name, e_loss, t_e_loss, e_grad, t_e_grad)
    assert e_loss <= 2 * t_e_loss and e_grad <= 2 * t_e_grad
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(out).all())
    row = ring.rows[0].tolist()
    assert row[0] == float(out[0]) and row[3] == 0.0 == float(out[1]) and row[4] == N and row[5] == 0.0
    assert row[1] == 0.0 == row[2] and row[6] == 1.0 and row[7] == 0.0


def test_weight_scales_the_clamped_log_of_a_probability_of_exactly_0_or_1():
    """torch clamps log at -100 in BCELoss and sf_bce does the same; the weight multiplies the clamped value."""
    x = torch.tensor([[0.0, 0.0, 1.0, 1.0]]).cuda()
    y = torch.tensor([[0.0, 1.0, 0.0, 1.0]]).cuda()
    w = torch.tensor([0.5, 2.0, 4.0, 0.25]).cuda()
    d0, _, out0 = _run_bce(x, y, False)
    assert float(out0[0]) == 50.0  # (0 + 100 + 100 + 0) / 4
    d, ring, out = _run_bce_w(x, y, False, weight=w)
    assert float(out[0]) == 150.0  # (0 + 2 * 100 + 4 * 100 + 0) / 4
    assert torch.equal(d, d0 * w)   # powers of two: the products are exact
    assert float(ring.rows[0, 3]) == 0.0 and float(ring.rows[0, 5]) == 0.0


# ------------------------------------------------------------------------------------------------ sf_class_weights
def _counters(K, seed, empty):
    g = torch.Generator().manual_seed(seed)
    conf = torch.randint(0, 40, (K, K), generator=g, dtype=torch.int64)
    conf[torch.rand(K, K, generator=g) < 0.5] = 0
    for c in empty:
        conf[c] = 0
    conf[1] = 0
    conf[1, 0] = 1  # one class with a single sample
    c = 2 if K > 3 else 0
    conf[c, c] += 3  # and one that surely has more
    return conf


def _ulps(a, b):
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


@pytest.mark.parametrize("K", [3, 27, 400])
def test_class_weights_equal_the_numpy_restatement(K):
    import sfhip
    conf = _counters(K, K, empty=(0, K - 1) if K > 3 else (2,))
    support = conf.sum(dim=1).numpy()
    assert int((support == 0).sum()) >= 1 and int((support > 0).sum()) >= 2
    whole, out = _guarded((K,))
    got = sfhip.class_weights(conf.cuda(), out=out)
    torch.cuda.synchronize()
    assert got is out and _margins_intact(whole)
    want = cw_ref.balanced(support)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))  # exact
    assert bool((out.cpu()[torch.from_numpy(support == 0)] == 0).all())
    for beta in (0.9, 0.999, 0.9999):
        whole, out = _guarded((K,))
        sfhip.class_weights(conf.cuda(), scheme="effective", beta=beta, out=out)
        torch.cuda.synchronize()
        assert _margins_intact(whole)
        got, want = out.cpu().numpy(), cw_ref.effective(support, beta)
        assert np.array_equal(got == 0, support == 0)
        assert _ulps(got, want) <= 2, (beta, _ulps(got, want))
        assert abs(float(got.astype(np.float64).sum()) - float((support > 0).sum())) < 1e-4 * K
    # twice the same bits
    a = sfhip.class_weights(conf.cuda(), scheme="effective", beta=0.999)
    b = sfhip.class_weights(conf.cuda(), scheme="effective", beta=0.999)
    assert _same_bits(a, b)


def test_class_weights_of_empty_counters_and_the_class_limit():
    import sfhip
    for scheme, beta in (("balanced", None), ("effective", 0.99)):
        whole, out = _guarded((27,))
        sfhip.class_weights(torch.zeros((27, 27), dtype=torch.int64, device="cuda"), scheme=scheme, beta=beta, out=out)
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == 0).all()) and _margins_intact(whole)
    w = sfhip.class_weights(torch.ones((1024, 1024), dtype=torch.int64, device="cuda"))  # the limit itself
    assert bool((w == 1.0).all())
    with pytest.raises(sfhip.SfhipError, match="SF_EINVAL"):
        sfhip.class_weights(torch.zeros((1025, 1025), dtype=torch.int64, device="cuda"))
    with pytest.raises(sfhip.SfhipError):
        sfhip.class_weights(torch.zeros((3, 3), dtype=torch.int64, device="cuda"),
                            out=torch.zeros(4, device="cuda"))


def test_meter_weights_come_from_its_counters():
    from slowfast.utils.meters import DevicePerClassMeter
    g = torch.Generator().manual_seed(3)
    N, K = 64, 5
    preds = torch.randn(N, K, generator=g).cuda()
    labels = torch.randint(0, K - 1, (N,), generator=g).cuda()  # class K - 1 never occurs
    meter = DevicePerClassMeter(K, 2)
    meter.update(preds, labels)
    w = meter.class_weights()
    support = np.bincount(labels.cpu().numpy(), minlength=K)
    assert np.array_equal(w.cpu().numpy(), cw_ref.balanced(support)) and float(w[K - 1]) == 0.0
    e = meter.class_weights(scheme="effective", beta=0.99)
    assert _ulps(e.cpu().numpy(), cw_ref.effective(support, 0.99)) <= 2


# ------------------------------------------------------------------------------------------------ loss objects, capture
def test_loss_objects_read_their_weights_by_reference():
    st = _mods()
    g = torch.Generator().manual_seed(12)
    N, K = 6, 27
    x = torch.randn(N, K, generator=g).cuda()
    y = torch.randint(0, K, (N,), generator=g).cuda()
    w = _weights(K, g).cuda()
    loss_fun = st.HipCrossEntropy(5, st.StatsRing(4), weight=w)
    a = x.clone().requires_grad_(True)
    loss = loss_fun(a, y)
    loss.backward()
    want = F.cross_entropy(x.double().cpu(), y.cpu(), weight=w.double().cpu())
    assert abs(float(loss.detach()) - float(want)) <= 1e-6 * float(want)
    assert _same_bits(a.grad, loss_fun.dlogits) and float(loss_fun.guard[0]) == 0.0
    w.mul_(2.0)  # all weights doubled, in place: the same loss and gradient (bit for bit: a power of two)
    b = x.clone().requires_grad_(True)
    loss_fun(b, y)
    loss_fun.backward_direct(b)
    assert _same_bits(a.grad, b.grad)
    w2 = _weights(K, g).cuda()
    loss_fun.set_weight(w2)
    assert loss_fun.weight is w and _same_bits(w, w2)
    c = x.clone().requires_grad_(True)
    loss_fun(c, y).backward()
    ref = x.double().cpu().requires_grad_(True)
    F.cross_entropy(ref, y.cpu(), weight=w2.double().cpu()).backward()
    assert float((c.grad.double().cpu() - ref.grad).abs().max()) <= 1e-7
    # a host list is uploaded once; a length that does not match the predictions is refused at the call
    short = st.HipCrossEntropy(5, st.StatsRing(4), weight=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="weight"):
        short(x, y)
    # BCE: weight and pos_weight together through the object
    t = (torch.rand(N, K, generator=g) < 0.3).float().cuda()
    p = _weights(K, g).cuda()
    bl = st.HipBCEWithLogits(st.StatsRing(4), weight=w, pos_weight=p)
    loss = bl(x.clone().requires_grad_(True), t)
    want = F.binary_cross_entropy_with_logits(x.double().cpu(), t.double().cpu(), weight=w.double().cpu(),
                                              pos_weight=p.double().cpu())
    assert abs(float(loss.detach()) - float(want)) <= 1e-6 * float(want)
    assert float(bl.ring.rows[0, 6]) == 1.0


def test_captured_step_follows_weights_refreshed_from_the_counters():
    st = _mods()
    from slowfast.models import engine
    from slowfast.utils.meters import DevicePerClassMeter
    g = torch.Generator().manual_seed(21)
    N, K = 6, 27
    logits0 = torch.randn(N, K, generator=g).cuda()
    labels = torch.randint(0, K, (N,), generator=g).cuda()
    conf_a = _counters(K, 5, empty=(3,)).cuda()
    conf_b = _counters(K, 6, empty=(4, 9)).cuda()
    for c in (conf_a, conf_b):  # every class of the batch has support under both
        c[labels, labels] += 2

    def make(conf):
        logits = logits0.clone().requires_grad_(True)
        meter = DevicePerClassMeter(K, 5)
        meter.conf.copy_(conf)
        w = torch.ones(K, device="cuda")
        loss_fun = st.HipCrossEntropy(5, st.StatsRing(8), weight=w)

        def step():
            if logits.grad is not None:
                logits.grad.zero_()
            meter.class_weights(out=w)
            loss_fun(logits, labels)
            loss_fun.backward_direct(logits)
        torch.cuda.synchronize()
        return logits, meter, w, loss_fun, step

    side = torch.cuda.Stream()

    def warm(step):
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.synchronize()

    # eager, on the second set of counters
    logits, meter, w, loss_fun, step = make(conf_b)
    warm(step)
    eager = (logits.grad.clone(), loss_fun.out.clone(), w.clone())
    assert np.array_equal(w.cpu().numpy(), cw_ref.balanced(conf_b.sum(dim=1).cpu().numpy()))

    # captured on the first set, replayed after the counters changed in place
    logits, meter, w, loss_fun, step = make(conf_a)
    warm(step)
    first = logits.grad.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    with torch.cuda.stream(side):
        engine.replay(graph)
    torch.cuda.synchronize()
    assert _same_bits(logits.grad, first)
    meter.conf.copy_(conf_b)
    before = int(loss_fun.ring.counter[0])
    with torch.cuda.stream(side):
        engine.replay(graph)
    torch.cuda.synchronize()
    assert _same_bits(logits.grad, eager[0]) and _same_bits(loss_fun.out, eager[1]) and _same_bits(w, eager[2])
    assert not _same_bits(logits.grad, first) and int(loss_fun.ring.counter[0]) == before + 1
