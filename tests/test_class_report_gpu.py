"""sf_confusion_update / sf_class_report (csrc/class_report.hip) on the GPU and DevicePerClassMeter on top of them,
against the brute-force restatement (tests/_class_report_ref.py).

Counts are integers and are compared EXACTLY.  Every ratio (precision, recall, F1, the accuracies) is one fp64
division of exact integers on both sides, so equality is expected and asserted.  The macro means are a fixed-order sum
of at most K such ratios and one division; they are given 4 ulp so that the test does not depend on how either side's
compiler contracts or orders the additions."""
import math

import pytest
import torch

import _class_report_ref as ref
from _host_reads import count_host_reads

pytestmark = pytest.mark.gpu
NAN = float("nan")
MEANS = ("mean_class_accuracy", "macro_precision", "macro_recall", "macro_f1")


# ------------------------------------------------------------------------------------------------ inputs and checks
def _scores(N, K, seed, levels=0):
    """Seeded fp32 scores [N, K] and int64 labels [N] on the host.  levels > 0: scores take `levels` values (ties
    everywhere); 0: continuous, every third row with its label's score raised to the top (so that hits occur at any K),
    then deliberate ties written in — the maximum duplicated at another index (higher or lower) in some rows, the
    label's score duplicated in others, the label's score set to the 5th largest in others."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, K, (N,), generator=g)
    if levels:
        return torch.randint(0, levels, (N, K), generator=g).float() / levels, labels
    preds = torch.rand(N, K, generator=g)
    for r in range(N):
        row, lab = preds[r], int(labels[r])
        other = int(torch.randint(0, K, (1,), generator=g))
        if r % 3 == 0:
            row[lab] += 1.0
        if r % 4 == 0:
            row[other] = row.max()          # the maximum twice: the lower index is predicted
        elif r % 4 == 1:
            row[other] = row[lab]           # a class ties the label: in front of it iff its index is lower
        elif r % 4 == 2 and K > 5:
            row[lab] = row.topk(5).values[4]  # the label's score equals the 5th largest: at the k-th rank's edge
    return preds, labels


def _meter(K, k_hi):
    from slowfast.utils.meters import DevicePerClassMeter
    return DevicePerClassMeter(K, k_hi)


def _state(m):
    return {"conf": m.conf.cpu().tolist(), "hits": m.hits.cpu().tolist(), "refused": m.refused.cpu().tolist()}


def _want(preds, labels, K, k_hi, counts=None):
    return ref.confusion_update(ref.empty_counts(K) if counts is None else counts, preds.tolist(), labels.tolist(),
                                k_hi)


def _close(got, want):
    return abs(got - want) <= 4 * math.ulp(want)


def _check_report(report, counts, K):
    """A finalize() result against the restatement's report of `counts`."""
    summary, table = ref.class_report(counts)
    assert report["confusion"].tolist() == counts["conf"] and report["hits"].tolist() == counts["hits"]
    assert report["confusion"].dtype == torch.int64 and tuple(report["confusion"].shape) == (K, K)
    assert not report["confusion"].is_cuda and not report["per_class"].is_cuda
    assert report["refused"] == {"bad_label": counts["refused"][0], "non_finite": counts["refused"][1]}
    assert report["per_class"].tolist() == table                      # one division each: the same bits
    for name in ref.SUMMARY_FIELDS:
        got, want = report["summary"][name], summary[name]
        print("%-24s %.17g (restatement %.17g)" % (name, got, want))
        if name in MEANS:
            assert _close(got, want), (name, got, want)
        else:
            assert got == want, (name, got, want)


def _run(preds, labels, K, k_hi, view=None):
    """One update of a fresh meter on `view` (default: the rows as they are) and its checked report."""
    m = _meter(K, k_hi)
    m.update(preds.cuda() if view is None else view, labels.cuda())
    want = _want(preds, labels, K, k_hi)
    assert _state(m) == want
    _check_report(m.finalize(allow_refused=True), want, K)
    return m, want


def _padded(preds, ld, offset=0):
    """`preds` [N, K] as a GPU view with row stride `ld` that starts `offset` floats into its storage; every float
    around the rows is NaN.  Returns (view, whole storage)."""
    N, K = preds.shape
    whole = torch.full((offset + N * ld + 8,), NAN, device="cuda")
    view = whole[offset:offset + N * ld].view(N, ld)[:, :K]
    view.copy_(preds.cuda())
    return view, whole


# ------------------------------------------------------------------------------------------------ 1: the fork's 3 classes
@pytest.mark.parametrize("N", [7, 1, 300])
def test_three_classes(N):
    """K = 3 on the LDS route; N = 300 takes two workgroups, so two groups flush into the same counters."""
    preds, labels = _scores(N, 3, 10 + N, levels=4)
    _, want = _run(preds, labels, 3, 2)
    assert sum(map(sum, want["conf"])) == N
    if N == 300:
        assert all(want["conf"][a][b] > 0 for a in range(3) for b in range(3))  # every counter is exercised


@pytest.mark.parametrize("K,ld", [(4, 4), (6, 8), (10, 10), (27, 28)])
def test_small_route_row_forms(K, ld):
    """Rows on 16 bytes (ld % 4 == 0) are read 16 bytes at a time with a scalar tail (K = 6, 27), any other 4."""
    preds, labels = _scores(70, K, 100 + K, levels=0 if K > 5 else 3)
    view, _ = _padded(preds, ld)
    _run(preds, labels, K, min(5, K), view=view)


# ------------------------------------------------------------------------------------------------ 2: the route boundary
@pytest.mark.parametrize("layout", ["rows_on_16_bytes", "dense"])
def test_both_sides_of_the_route_boundary(layout):
    """K = sf_confusion_small_kmax() (thread per row, LDS counters) and K + 1 (wavefront per row) on the same scores."""
    import sfhip
    kmax = sfhip.lib().sf_confusion_small_kmax()
    assert kmax == 201
    wide, labels = _scores(33, kmax + 1, 7)
    labels = labels.clamp(max=kmax - 1)
    states = {}
    for K in (kmax, kmax + 1):
        preds = wide[:, :K].contiguous()
        view = _padded(preds, 204)[0] if layout == "rows_on_16_bytes" else preds.cuda()
        assert view.stride(0) == (204 if layout == "rows_on_16_bytes" else K)
        m, want = _run(preds, labels, K, 5, view=view)
        states[K] = want
    # the last column is one more competitor: a row's prediction moves only if that column wins it
    moved = sum(1 for r in range(33) if ref.row_order(wide[r].tolist())[0] == kmax)
    assert sum(states[kmax + 1]["conf"][c][kmax] for c in range(kmax + 1)) == moved


# ------------------------------------------------------------------------------------------------ 3: Kinetics' 400
def test_400_classes_with_ties():
    preds, labels = _scores(64, 400, 3)
    assert int((preds == preds.max(1, keepdim=True).values).sum()) > 64  # rows with the maximum twice
    _, want = _run(preds, labels, 400, 5)
    assert 0 < sum(h[0] for h in want["hits"]) < sum(h[1] for h in want["hits"]) <= 64


# ------------------------------------------------------------------------------------------------ 4: strided views
@pytest.mark.parametrize("K,N", [(3, 70), (400, 9)])
def test_strided_view_between_nans(K, N):
    """ld = K + 3 and a storage offset of one float: the scalar form of both routes.  The floats around the rows are
    NaN: none may reach the counts (a NaN row would be refused) and none may change."""
    preds, labels = _scores(N, K, 40 + K, levels=4 if K == 3 else 0)
    view, whole = _padded(preds, K + 3, offset=1)
    assert view.data_ptr() % 16 == 4 and view.stride(0) == K + 3
    before = whole.clone()
    m, want = _run(preds, labels, K, min(5, K), view=view)
    assert want["refused"] == [0, 0]
    assert torch.equal(whole.view(torch.int32), before.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 5: refused rows
@pytest.mark.parametrize("K", [3, 400])
def test_refused_rows_move_nothing_else(K):
    preds, labels = _scores(12, K, 50 + K)
    m = _meter(K, 2)
    m.update(preds.cuda(), labels.cuda())
    base = _state(m)
    bad_p = preds[:5].clone()
    bad_l = labels[:5].clone()
    bad_l[0], bad_l[1] = -1, K
    bad_p[2, K - 1] = NAN
    bad_p[3, 0] = float("-inf")
    bad_l[4], bad_p[4, 1] = K + 7, NAN       # both: decided by the label, its scores are never read
    m.update(bad_p.cuda(), bad_l.cuda())
    after = _state(m)
    assert after["refused"] == [3, 2] and after["conf"] == base["conf"] and after["hits"] == base["hits"]
    assert after == _want(bad_p, bad_l, K, 2, counts=_want(preds, labels, K, 2))
    with pytest.raises(ValueError, match=r"3 row\(s\) with a label outside \[0, %d\) and 2 row" % K):
        m.finalize()
    assert m.finalize(allow_refused=True)["refused"] == {"bad_label": 3, "non_finite": 2}


# ------------------------------------------------------------------------------------------------ 6: accumulation
@pytest.mark.parametrize("K", [3, 400])
def test_two_halves_equal_the_whole_and_reset_zeroes(K):
    preds, labels = _scores(64, K, 60 + K, levels=5 if K == 3 else 0)
    whole, want = _run(preds, labels, K, 2)
    m = _meter(K, 2)
    torch.cuda.synchronize()
    with count_host_reads() as seen:
        m.update(preds[:29].cuda(), labels[:29].cuda())
        m.update(preds[29:].cuda(), labels[29:].cuda())
        m.all_reduce()  # world size 1: nothing happens
        assert seen == []
        report = m.finalize()
        assert len(seen) == 1, seen  # the one host read of the epoch
    _check_report(report, want, K)
    assert torch.equal(m._buf, whole._buf)  # the counters and the report's bits
    m.reset()
    assert int(m._buf.count_nonzero()) == 0
    m.update(preds[:29].cuda(), labels[:29].cuda())
    assert _state(m) == _want(preds[:29], labels[:29], K, 2)


# ------------------------------------------------------------------------------------------------ 7: sf_topk_errors
@pytest.mark.parametrize("K,k_hi", [(3, 2), (27, 5), (400, 5)])
def test_counts_reproduce_the_topk_errors_ring_row(K, k_hi):
    """The same batch through the existing kernel: trace(conf) and sum(hits) are the hits behind its two error
    percentages, refused rows included (it counts them as wrong)."""
    from slowfast.models import step_tail as st
    N = 48
    preds, labels = _scores(N, K, 70 + K, levels=6 if K == 3 else 0)
    labels[5] = K
    preds[9, K // 2] = NAN
    m = _meter(K, k_hi)
    m.update(preds.cuda(), labels.cuda())
    ring = st.StatsRing(2)
    st.topk_errors(preds.cuda(), labels.cuda(), k_hi, ring)
    row = ring.rows.cpu()[0].tolist()
    s = _state(m)
    trace = sum(s["conf"][c][c] for c in range(K))
    assert trace == sum(h[0] for h in s["hits"]) and s["refused"] == [1, 1]
    assert sum(map(sum, s["conf"])) == N - 2
    pct = [float((1.0 - torch.tensor(float(c)) / N) * 100.0) for c in (trace, sum(h[1] for h in s["hits"]))]
    assert row == [0.0, pct[0], pct[1], 1.0, float(N), 1.0, 2.0, 0.0], (row, pct)
    assert pct[1] < pct[0] < 100.0


# ------------------------------------------------------------------------------------------------ 8: capture
def test_update_inside_a_captured_graph():
    """One update captured on one stream (no parallel branches) and replayed twice = two eager updates."""
    preds, labels = _scores(20, 3, 80, levels=4)
    p, lab = preds.cuda(), labels.cuda()
    eager = _meter(3, 2)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eager.update(p, lab)
        eager.update(p, lab)
    torch.cuda.synchronize()
    m = _meter(3, 2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        m.update(p, lab)
    torch.cuda.synchronize()
    assert int(m.state.count_nonzero()) == 0  # captured, not run
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(m.state, eager.state)
    once = _want(preds, labels, 3, 2)
    assert _state(m) == _want(preds, labels, 3, 2, counts=once)


# ------------------------------------------------------------------------------------------------ 9: the meters
class _Cfg(object):
    def __init__(self, topk):
        self.LOG_PERIOD, self.NUM_GPUS = 2, 1
        self.SOLVER = type("S", (), {"MAX_EPOCH": 1})()
        self.DATA = type("D", (), {"MULTI_LABEL": False})()
        self.TRAIN = type("T", (), {"TOPK": topk})()


def test_val_meter_feeds_the_per_class_meter_and_keeps_its_own_bits():
    from slowfast.utils.meters import DeviceValMeter
    K, batches = 3, [_scores(8, 3, 90 + i, levels=5) for i in range(3)]

    def run(per_class):
        m = DeviceValMeter(3, _Cfg(2), per_class=per_class)
        logged = []
        for i, (p, lab) in enumerate(batches):
            m.update_stats(p.cuda(), lab.cuda())
            m.update_predictions(p.cuda(), lab.cuda())
            logged.append(m.log_iter_stats(0, i))
        logged.append(m.log_epoch_stats(0))
        return m, logged

    plain, logged_plain = run(None)
    pc = _meter(K, 2)
    fed, logged_fed = run(pc)
    assert torch.equal(fed.ring.rows.view(torch.int32), plain.ring.rows.view(torch.int32))  # the same ring rows
    assert torch.equal(fed.ring.counter, plain.ring.counter)
    drop = ("time_diff", "eta", "gpu_mem", "RAM")
    for a, b in zip(logged_fed, logged_plain):
        assert (a is None) == (b is None)
        if a is not None:
            assert {k: v for k, v in a.items() if k not in drop} == {k: v for k, v in b.items() if k not in drop}
    preds, labels = torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches])
    want = _want(preds, labels, K, 2)
    report = pc.finalize()
    _check_report(report, want, K)
    # the epoch's top-1 error is the report's accuracy, seen from the other side
    assert report["summary"]["samples"] == fed.num_samples == 24
    # (batches of 8: every percentage is a multiple of 12.5, exact in float32; what is left is fp64 rounding)
    assert abs((1.0 - report["summary"]["accuracy"]) * 100.0 - logged_fed[-1]["top1_err"]) < 1e-9
    fed.reset()
    assert int(pc._buf.count_nonzero()) == 0


@pytest.mark.parametrize("method", ["sum", "max"])
def test_test_meter_reports_the_ensemble_and_keeps_its_own_bits(method):
    """5 videos x 3 clips, K = 3: the per-class meter is fed once, at finalize_metrics, with the videos' rows."""
    from slowfast.utils.meters import DeviceTestMeter
    nv, nc, K = 5, 3, 3
    # untied scores: the meter's own top-k goes through torch.topk, whose order among equal scores is not the kernels'
    clips = torch.rand(nv * nc, K, generator=torch.Generator().manual_seed(95))
    video_labels = torch.tensor([0, 2, 1, 2, 0])
    clip_ids = torch.randperm(nv * nc, generator=torch.Generator().manual_seed(4))

    def run(per_class):
        m = DeviceTestMeter(nv, nc, K, 3, ensemble_method=method, per_class=per_class)
        for s in range(0, nv * nc, 5):
            ids = clip_ids[s:s + 5]
            m.update_stats(clips[ids].cuda(), video_labels[ids // nc].cuda(), ids.cuda())
        return m, m.finalize_metrics(ks=(1, 2))

    plain, stats_plain = run(None)
    pc = _meter(K, 2)
    fed, stats_fed = run(pc)
    assert stats_fed == stats_plain and stats_fed["complete"] is True
    for name in ("video_preds", "video_labels", "clip_count", "bad_count"):
        a, b = getattr(fed, name), getattr(plain, name)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    want = _want(fed.video_preds.cpu(), fed.video_labels.cpu(), K, 2)
    report = pc.finalize()
    _check_report(report, want, K)
    assert report["summary"]["samples"] == nv
    assert "%.2f" % (report["summary"]["accuracy"] * 100.0) == stats_fed["top1_acc"]
    # finalize_metrics again: the report is the videos', not twice the videos'
    fed.finalize_metrics(ks=(1, 2))
    assert pc.finalize()["confusion"].tolist() == want["conf"]


# ------------------------------------------------------------------------------------------------ the report alone
@pytest.mark.parametrize("K", [1, 67, 1024])
def test_class_report_of_written_counters(K):
    """sf_class_report on counters written by hand, up to its limit of 1024 classes: rows without support, columns
    never predicted, and counts far above any epoch's (exact in fp64 below 2^53)."""
    import sfhip
    g = torch.Generator().manual_seed(K)
    conf = torch.randint(0, 1 << 30, (K, K), generator=g) * (torch.rand(K, K, generator=g) < 0.3)
    if K > 2:
        conf[K // 2] = 0       # a class without support
        conf[:, K // 3] = 0    # a class never predicted
        conf[K - 1, K - 1] = 1 << 40
    sup = conf.sum(1)
    hits = torch.stack([conf.diagonal(), conf.diagonal() + (sup - conf.diagonal()) // 2], dim=1).contiguous()
    out, table = sfhip.class_report(conf.cuda(), hits.cuda())
    summary, want = ref.class_report({"conf": conf.tolist(), "hits": hits.tolist(), "refused": [0, 0]})
    assert table.cpu().tolist() == want
    for name, got in zip(ref.SUMMARY_FIELDS, out.cpu().tolist()):
        if name in MEANS:
            assert _close(got, summary[name]), (name, got, summary[name])
        else:
            assert got == summary[name], (name, got, summary[name])
