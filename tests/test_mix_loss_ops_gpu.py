"""sf_ce_mix on the GPU (csrc/step_tail.hip) through slowfast/models/step_tail.py: the soft-target cross-entropy of label
smoothing, mixup and CutMix — loss, gradient, hit counts, ring row and flag from one launch.

Parity is against float64 on the CPU (tests/_mix_ref.py, itself checked against F.cross_entropy with dense targets in
test_mix_args_cpu.py); the bound is the project's rule from test_step_tail_ops_gpu.py: what torch's own float32 GPU
F.cross_entropy(x, t_dense) misses the same float64 values by, on the same inputs, times 2 — measured in the test itself,
with no absolute floor.  The float64 reference takes lam and eps as the float32 values the kernel is handed (lam travels
as float32 bits in the mix row, eps as a C float); torch's float32 run gets the float64 targets rounded to float32.
Every case prints both errors and appends them to the run's report (mix_loss_report.txt beside the other GPU reports,
through test_backward_ops_gpu's helper); the figures measured on an MI355X are in profiles/mix_loss.txt."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _mix_ref as ref
from test_weighted_loss_ops_gpu import _Owned, _run_ce, _same_bits

pytestmark = pytest.mark.gpu
EPS32 = float(np.float32(0.1))  # what `smoothing = 0.1` is once it is a C float


def _mods():
    from slowfast.models import step_tail
    return step_tail


def _report(name, e_loss, t_e_loss, e_grad, t_e_grad):
    from test_backward_ops_gpu import _report as report
    print("ce_mix %-28s loss err %.3e (torch %.3e)  gradient err %.3e (torch %.3e)" % (name, e_loss, t_e_loss, e_grad,
                                                                                    t_e_grad))
    for what, v in (("loss", e_loss), ("loss (torch)", t_e_loss), ("gradient", e_grad), ("gradient (torch)", t_e_grad)):
        report("ce_mix %s %s" % (name, what), v, "mix_loss_report.txt")


def _run(logits, labels, rows, eps, k_hi, cap=3, dev_rows=None):
    """One sf_ce_mix launch into guarded buffers.  rows: numpy int64 [N, 7] or None; dev_rows: a device copy that differs
    from the host rows (the kernel's own check)."""
    N, K = logits.shape
    o = _Owned(N, K, cap)
    host = dev = None
    if rows is not None:
        host = torch.from_numpy(np.ascontiguousarray(rows))
        dev = (host if dev_rows is None else torch.from_numpy(np.ascontiguousarray(dev_rows))).cuda()
    _mods().ce_mix(logits, labels, k_hi, o.ring, o.out, mix_host=host, mix=dev, smoothing=eps, dlogits=o.d)
    return o.check()


def _pct(hits, n):
    return float((1.0 - torch.tensor(float(hits)) / n) * 100.0)


# ------------------------------------------------------------------------------------------------ bit equality
@pytest.mark.parametrize("N", [1, 3, 65])   # 65: past one wavefront of rows (and past the 16-wavefront row stride)
@pytest.mark.parametrize("K", [2, 27, 400])  # 400: the lane-strided column loop
def test_without_smoothing_and_mix_the_bits_are_ce_topks(N, K):
    g = torch.Generator().manual_seed(N * 1000 + K)
    x = (torch.randn(N, K, generator=g) * 3.0).cuda()
    y = torch.randint(0, K, (N,), generator=g).cuda()
    k_hi = min(5, K)
    d0, ring0, out0 = _run_ce(x, y, k_hi)
    d1, ring1, out1 = _run(x, y, None, 0.0, k_hi)
    assert _same_bits(d0, d1) and _same_bits(out0, out1) and _same_bits(ring0.rows[0], ring1.rows[0])
    assert bool(torch.isnan(ring1.rows[1:]).all())  # only row 0 was written
    # rows that mix nothing (lam = 1, any partner) are the same arithmetic: multiplies by one, exact zeros added
    rows = ref.make_rows([N - 1 - r for r in range(N)], 0, 1.0)
    d2, ring2, out2 = _run(x, y, rows, 0.0, k_hi)
    assert _same_bits(d0, d2) and _same_bits(out0, out2) and _same_bits(ring0.rows[0], ring2.rows[0])


# ------------------------------------------------------------------------------------------------ parity
LAMS = (0.0, 0.3, 0.5, 1.0)


def _parity_cases():
    cases = []
    for eps in (0.0, 0.1):
        for N, K in ((1, 2), (3, 27), (8, 400), (65, 27), (65, 400)):
            cases.append(("n%d_k%d_eps%g" % (N, K, eps), N, K, 0, eps, None))
        cases.append(("n8_k27_stride_eps%g" % eps, 8, 27, 3, eps, None))
        cases.append(("n8_k400_pm80_eps%g" % eps, 8, 400, 0, eps, "big"))
    return cases


@pytest.mark.parametrize("name,N,K,pad,eps,special", _parity_cases(), ids=[c[0] for c in _parity_cases()])
def test_ce_mix_matches_float64_within_twice_torchs_own_error(name, N, K, pad, eps, special):
    g = torch.Generator().manual_seed(N * 1000 + K + int(eps * 10))
    x = torch.randn(N, K + pad, generator=g) * 3.0
    if special == "big":  # one row near +-80: exp() of the raw values would overflow float32
        x[2] = torch.where(torch.rand(K, generator=g) < 0.5, torch.tensor(80.0), torch.tensor(-80.0)) + \
            torch.randn(K, generator=g) * 0.01
    y = torch.randint(0, K, (N,), generator=g)
    partner = torch.randperm(N, generator=g).tolist()
    partner[N - 1] = N - 1  # a row mixed with itself
    lam = [LAMS[r % 4] for r in range(N)]  # every lam of the issue's list, row by row
    rows = ref.make_rows(partner, 1, lam)
    e32 = float(np.float32(eps))
    want_loss, want_d, bad = ref.ce_mix(x[:, :K].double().numpy(), y.numpy(), rows, e32)
    assert bad == 0
    t64 = torch.from_numpy(ref.dense_targets(y.numpy(), rows, K, e32))
    xg = x.cuda()[:, :K].detach().requires_grad_(True)  # the same strided view on the GPU
    t_loss = F.cross_entropy(xg, t64.float().cuda())
    t_loss.backward()
    d, ring, out = _run(x.cuda()[:, :K], y.cuda(), rows, eps, min(5, K))
    e_loss = abs(float(out[0].double().cpu()) - want_loss)
    t_e_loss = abs(float(t_loss.detach().double().cpu()) - want_loss)
    e_grad = float(np.abs(d.double().cpu().numpy() - want_d).max())
    t_e_grad = float(np.abs(xg.grad.double().cpu().numpy() - want_d).max())
    _report(name, e_loss, t_e_loss, e_grad, t_e_grad)
    assert e_loss <= 2 * t_e_loss and e_grad <= 2 * t_e_grad
    row = ring.rows[0].tolist()
    assert row[0] == float(out[0]) and row[3] == 0.0 == float(out[1]) and row[4] == N and row[5] == 0.0
    assert row[6] == 0.0 == row[7]  # KIND_CE; column 7 is sf_grad_norm's
    h1, hk = ref.hit_counts(x[:, :K].numpy(), y.numpy(), rows, min(5, K))
    assert row[1] == _pct(h1, N) and row[2] == _pct(hk, N)


# ------------------------------------------------------------------------------------------------ hit counts
@pytest.mark.parametrize("N,K,k_hi", [(3, 3, 2), (17, 27, 5), (65, 400, 5)])
def test_hits_are_counted_against_the_dominant_label(N, K, k_hi):
    g = torch.Generator().manual_seed(N + K)
    x = torch.randperm(N * K, generator=g).float().view(N, K) / 7.0  # tie-free
    y = torch.randint(0, K, (N,), generator=g)
    partner = torch.randperm(N, generator=g).tolist()
    lam = [(0.0, 0.49, 0.5, 0.51, 1.0)[r % 5] for r in range(N)]
    rows = ref.make_rows(partner, 1, lam)
    dom = torch.from_numpy(ref.dominant_labels(y.numpy(), rows))
    for r in range(N):  # every third row a top-1 hit, every third second in its row; the values stay distinct
        if r % 3 == 0:
            x[r, dom[r]] = float(N * K)
        elif r % 3 == 1:
            x[r, dom[r]] = -1.0
            x[r, dom[r]] = float(x[r].max()) - 0.01
    _, ring, _ = _run(x.cuda(), y.cuda(), rows, 0.1, k_hi)
    h1, hk = ref.hit_counts(x.numpy(), y.numpy(), rows, k_hi)
    assert 0 < h1 < hk
    assert ring.rows[0, 1:3].tolist() == [_pct(h1, N), _pct(hk, N)]
    # and an integer count by torch.topk against the dominant labels
    top = torch.topk(x, k_hi, dim=1).indices
    assert (h1, hk) == (int((top[:, 0] == dom).sum()), int((top == dom[:, None]).any(dim=1).sum()))


def test_ties_go_to_the_lower_index():
    # every row: classes 1, 3 and 4 tie at the top.  Dominant label 1 is first of the tie (top-1 hit), 3 is second
    # (a top-2 hit only), 4 third (no hit at k = 2)
    x = torch.tensor([[0.0, 2.0, 1.0, 2.0, 2.0, -1.0]] * 4).cuda()
    y = torch.tensor([1, 3, 4, 4]).cuda()
    rows = ref.make_rows([0, 1, 2, 1], 1, [1.0, 0.75, 0.5, 0.25])  # row 3: lam < 0.5, so its partner's label 3 counts
    _, ring, _ = _run(x, y, rows, 0.0, 2)
    assert ring.rows[0, 1:3].tolist() == [_pct(1, 4), _pct(3, 4)]
    assert ref.hit_counts(x.cpu().numpy(), y.cpu().numpy(), rows, 2) == (1, 3)


# ------------------------------------------------------------------------------------------------ bad rows
def test_bad_rows_add_nothing_and_are_counted():
    g = torch.Generator().manual_seed(6)
    N, K = 6, 27
    x = torch.randn(N, K, generator=g)
    y = torch.randint(0, K, (N,), generator=g)
    rows = ref.make_rows([5, 4, 3, 2, 1, 0], 1, [0.3, 0.6, 0.5, 0.5, 0.4, 0.7])
    clean = _run(x.cuda(), y.cuda(), rows, EPS32, 5)
    # bad label a in row 1 (which is also row 4's b), a device row with a wild partner (row 0; the host copy is valid),
    # a device lam outside [0, 1] (row 3)
    yb = y.clone()
    yb[1] = K
    dev = rows.copy()
    dev[0, 0] = 1 << 40
    dev[3, 2] = ref.lam_bits(1.5)
    d, ring, out = _run(x.cuda(), yb.cuda(), rows, EPS32, 5, dev_rows=dev)  # (_run checks the sentinel margins)
    for r in (0, 1, 3, 4):
        assert bool((d[r].view(torch.int32) == 0).all()), r  # zeros, not NaN
    row = ring.rows[0].tolist()
    assert row[5] == 4.0 and row[4] == N and row[3] == 0.0 == float(out[1])
    want_loss, want_d, bad = ref.ce_mix(x.double().numpy(), yb.numpy(), dev, EPS32)
    assert bad == 4
    assert abs(float(out[0]) - want_loss) <= 1e-6 * want_loss  # the divisor stays N
    assert float(np.abs(d.double().cpu().numpy() - want_d).max()) <= 1e-7
    assert _same_bits(d[[2, 5]], clean[0][[2, 5]])  # the good rows: the clean run's gradients
    assert row[1] >= _pct(2, N) and row[2] >= _pct(2, N)  # the four bad rows count as wrong
    # a negative label b through a valid partner, and a negative partner on the device
    yb = y.clone()
    yb[5] = -1
    dev = rows.copy()
    dev[2, 0] = -1
    d, ring, out = _run(x.cuda(), yb.cuda(), rows, 0.0, 5, dev_rows=dev)
    assert float(ring.rows[0, 5]) == 3.0  # rows 5 (a), 0 (b) and 2 (partner)
    for r in (0, 2, 5):
        assert bool((d[r].view(torch.int32) == 0).all()), r


def test_nan_logit_sets_the_flag_and_leaves_the_other_rows_clean():
    g = torch.Generator().manual_seed(8)
    N, K = 4, 27
    x = torch.randn(N, K, generator=g)
    y = torch.randint(0, K, (N,), generator=g)
    rows = ref.make_rows([3, 2, 1, 0], 1, 0.3)
    clean = _run(x.cuda(), y.cuda(), rows, EPS32, 5)
    assert float(clean[2][1]) == 0.0
    for poison in (float("nan"), float("inf")):
        xb = x.clone()
        xb[1, 3] = poison
        d, ring, out = _run(xb.cuda(), y.cuda(), rows, EPS32, 5)
        assert float(out[1]) == 1.0 == float(ring.rows[0, 3]) and float(ring.rows[0, 5]) == 0.0
        assert not bool(torch.isfinite(out[0]))
        assert _same_bits(d[[0, 2, 3]], clean[0][[0, 2, 3]])


# ------------------------------------------------------------------------------------------------ ring, determinism
def test_ring_slot_advances_and_two_runs_give_equal_bits():
    st = _mods()
    ring = st.StatsRing(3)
    out = torch.zeros(2, device="cuda")
    g = torch.Generator().manual_seed(9)
    rows = torch.from_numpy(ref.make_rows([3, 2, 1, 0], 1, [0.2, 0.4, 0.6, 0.8]))
    rows_dev = rows.cuda()
    losses = []
    for i in range(4):
        x = torch.randn(4, 9, generator=g)
        y = torch.randint(0, 9, (4,), generator=g)
        st.ce_mix(x.cuda(), y.cuda(), 5, ring, out, mix_host=rows, mix=rows_dev, smoothing=0.1)
        assert int(ring.counter[0]) == i + 1
        losses.append(float(out[0]))
    rows_cpu = ring.rows.cpu()  # steps 0..3 landed in rows 0, 1, 2, 0
    assert [float(rows_cpu[0, 0]), float(rows_cpu[1, 0]), float(rows_cpu[2, 0])] == [losses[3], losses[1], losses[2]]
    assert len(set(losses)) == 4 and bool((rows_cpu[:, 6] == 0).all()) and bool((rows_cpu[:, 7] == 0).all())
    x = (torch.randn(65, 400, generator=g) * 3.0).cuda()
    y = torch.randint(0, 400, (65,), generator=g).cuda()
    big = ref.make_rows(torch.randperm(65, generator=g).tolist(), 1, torch.rand(65, generator=g).tolist())
    a, b = _run(x, y, big, 0.1, 5), _run(x, y, big, 0.1, 5)
    assert _same_bits(a[0], b[0]) and _same_bits(a[2], b[2]) and _same_bits(a[1].rows[0], b[1].rows[0])
    plain = _run(x, y, None, 0.0, 5)
    assert not _same_bits(a[0], plain[0])


def test_loss_object_takes_the_rows_by_reference():
    st = _mods()
    g = torch.Generator().manual_seed(12)
    N, K = 6, 27
    x = torch.randn(N, K, generator=g).cuda()
    y = torch.randint(0, K, (N,), generator=g).cuda()
    rows_a = torch.from_numpy(ref.make_rows([5, 4, 3, 2, 1, 0], 1, 0.3))
    rows_b = torch.from_numpy(ref.make_rows([1, 0, 3, 2, 5, 4], 2, 0.8, (0, 0, 2, 2)))
    loss_fun = st.HipCrossEntropy(5, st.StatsRing(4), label_smoothing=0.1)
    fixed = rows_a.cuda()  # a fixed device tensor, refilled per batch: checked by the kernel alone
    a = x.clone().requires_grad_(True)
    loss = loss_fun(a, y, mix=fixed)
    loss.backward()
    want, want_d, _ = ref.ce_mix(x.double().cpu().numpy(), y.cpu().numpy(), rows_a.numpy(), EPS32)
    assert abs(float(loss.detach()) - want) <= 1e-6 * want
    assert _same_bits(a.grad, loss_fun.dlogits) and float(loss_fun.guard[0]) == 0.0
    assert float(np.abs(a.grad.double().cpu().numpy() - want_d).max()) <= 1e-7
    fixed.copy_(rows_b)
    b = x.clone().requires_grad_(True)
    loss_fun(b, y, mix=fixed)
    loss_fun.backward_direct(b)
    _, want_d, _ = ref.ce_mix(x.double().cpu().numpy(), y.cpu().numpy(), rows_b.numpy(), EPS32)
    assert float(np.abs(b.grad.double().cpu().numpy() - want_d).max()) <= 1e-7
    # a (host, device) pair gives the same bits; without mix the smoothing alone
    c = x.clone().requires_grad_(True)
    loss_fun(c, y, mix=(rows_b, fixed)).backward()
    assert _same_bits(b.grad, c.grad)
    e = x.clone().requires_grad_(True)
    loss = loss_fun(e, y)
    want = float(F.cross_entropy(x.double().cpu(), y.cpu(), label_smoothing=EPS32))
    assert abs(float(loss.detach()) - want) <= 1e-6 * want
    # without smoothing and mix the object launches sf_ce_topk as before
    plain = st.HipCrossEntropy(5, st.StatsRing(4))
    f = x.clone().requires_grad_(True)
    plain(f, y).backward()
    d0, _, out0 = _run_ce(x, y, 5)
    assert _same_bits(f.grad, d0) and _same_bits(plain.out, out0)
