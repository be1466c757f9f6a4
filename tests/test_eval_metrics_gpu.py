"""sf_map, sf_topk_errors, sf_rows_append (csrc/eval_metrics.hip) and sf_ensemble_update_ml (csrc/ensemble.hip) on the
GPU, and the meters on top of them (utils/meters.py: device_map, DeviceMultiLabelTestMeter, DeviceValMeter).

mAP and the per-class AP are compared with the reference's recorded fp64 results (tests/golden/map_vectors.npz) at
|d| <= 1e-12 = N * 4 * 2^-53 at the largest N (2048): one rounding per division, the rounding of scikit-learn's recall
difference and product, one per addition.  Everything else is integer counting or a copy and is compared exactly."""
import json
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from _host_reads import count_host_reads as _count_host_reads
from _map_cases import case_names, make_case
from _util import GOLDEN

pytestmark = pytest.mark.gpu
MAP_TOL = 1e-12


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(GOLDEN, "map_vectors.npz"))


def _strided(a, pad):
    """`a` [N, C] on the GPU as a view of rows of C + pad floats (the padding holds NaN: never to be read)."""
    n, c = a.shape
    whole = torch.full((n, c + pad), float("nan"), device="cuda")
    whole[:, :c] = torch.from_numpy(a).cuda()
    return whole[:, :c]


# ------------------------------------------------------------------------------------------------ sf_map
@pytest.mark.parametrize("name", case_names())
def test_map_matches_reference(vectors, name):
    import sfhip
    preds, labels = make_case(name)
    want_map, want_ap = float(vectors[name + "/map"]), vectors[name + "/ap"]
    runs = []
    for pad_p, pad_l in ((0, 0), (3, 5), (0, 0)):
        out, ap = sfhip.mean_ap(_strided(preds, pad_p), _strided(labels, pad_l), per_class=True)
        runs.append((out.cpu(), ap.cpu()))
    out, ap = runs[0][0].numpy(), runs[0][1].numpy()
    print("%s: mAP %.17g (reference %.17g, d %.3g), per-class max d %.3g" % (
        name, out[0], want_map, abs(out[0] - want_map), np.abs(ap - want_ap).max()))
    assert np.array_equal(ap < 0, want_ap < 0) and out[1] == (want_ap >= 0).sum() and out[2] == 0
    assert np.abs(ap - want_ap).max() <= MAP_TOL
    assert abs(out[0] - want_map) <= MAP_TOL
    for o, a in runs[1:]:  # strided rows, and a second run: the same bits
        assert torch.equal(o.view(torch.int64), runs[0][0].view(torch.int64))
        assert torch.equal(a.view(torch.int64), runs[0][1].view(torch.int64))


def test_map_counts_what_it_refuses():
    import sfhip
    from slowfast.utils.meters import device_map
    preds, labels = make_case("untied_n257_c17")
    want = device_map(torch.from_numpy(preds).cuda(), torch.from_numpy(labels).cuda())
    assert isinstance(want, float) and 0.0 < want < 1.0
    p, lab = preds.copy(), labels.copy()
    p[256, 16], p[3, 0] = np.nan, np.inf
    lab[100, 7] = 0.5
    out = sfhip.mean_ap(torch.from_numpy(p).cuda(), torch.from_numpy(lab).cuda()).cpu()
    assert out[2] == 3
    with pytest.raises(ValueError, match="3 element"):
        device_map(torch.from_numpy(p).cuda(), torch.from_numpy(lab).cuda())
    # labels of another dtype are converted, as bce does
    assert device_map(torch.from_numpy(preds).cuda(), torch.from_numpy(labels).cuda().long()) == want


# ------------------------------------------------------------------------------------------------ sf_topk_errors
def _reference_errors(preds, labels, ks):
    from slowfast.utils.meters import topks_correct
    return [float((1.0 - x / preds.size(0)) * 100.0) for x in topks_correct(preds, labels, ks)]


@pytest.mark.parametrize("N", [1, 3, 64, 65])
@pytest.mark.parametrize("K", [2, 5, 400])
def test_topk_errors_match_topks_correct(N, K):
    from slowfast.models import step_tail as st
    g = torch.Generator().manual_seed(N * 1000 + K)
    # a permutation per row: untied; the label's score is boosted so that both hits and misses occur
    preds = torch.stack([torch.randperm(K, generator=g).float() for _ in range(N)]) / K
    labels = torch.randint(0, K, (N,), generator=g)
    preds[torch.arange(N), labels] += 0.5 * torch.rand(N, generator=g)
    whole = torch.full((N, K + 3), float("nan"), device="cuda")
    whole[:, :K] = preds.cuda()
    for k_hi in sorted({1, min(5, K), K}):  # torch.topk itself refuses k > K, as the entry point does
        ring = st.StatsRing(3)
        st.topk_errors(whole[:, :K], labels.cuda(), k_hi, ring)
        row = ring.rows.cpu()[0].tolist()
        top1, topk = _reference_errors(preds.cuda(), labels.cuda(), (1, k_hi))
        assert row == [0.0, top1, topk, 0.0, float(N), 0.0, 2.0, 0.0], (k_hi, row, top1, topk)
        assert int(ring.counter.cpu()[0]) == 1
    if K == 400:
        assert 0.0 < top1 <= 100.0


def test_topk_errors_tie_bad_label_nonfinite_and_wrap():
    from slowfast.models import step_tail as st
    ring = st.StatsRing(2)
    # row 0: classes 1 and 3 tie at the label's value -> label 3 is behind class 1 (rank 1), label 1 would be first;
    # row 1: the same scores with label 1
    preds = torch.tensor([[0.1, 0.7, 0.2, 0.7, 0.0], [0.1, 0.7, 0.2, 0.7, 0.0]], device="cuda")
    st.topk_errors(preds, torch.tensor([3, 1], device="cuda"), 2, ring)
    # a label out of range is wrong for every k and counted; a NaN row is wrong and raises the flag
    bad = torch.tensor([[0.9, 0.1, 0.0], [0.2, float("nan"), 0.8], [0.1, 0.2, 0.7]], device="cuda")
    st.topk_errors(bad, torch.tensor([7, 2, 2], device="cuda"), 3, ring)
    rows = ring.rows.cpu().tolist()
    assert rows[0] == [0.0, 50.0, 0.0, 0.0, 2.0, 0.0, 2.0, 0.0]
    third = float((1.0 - torch.tensor(1.0) / 3) * 100.0)
    assert rows[1] == [0.0, third, third, 1.0, 3.0, 1.0, 2.0, 0.0]
    # cap = 2: the third batch goes to slot 0 again
    st.topk_errors(preds[:1], torch.tensor([1], device="cuda"), 1, ring)
    rows = ring.rows.cpu().tolist()
    assert rows[0] == [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0] and rows[1][4] == 3.0
    assert int(ring.counter.cpu()[0]) == 3


# ------------------------------------------------------------------------------------------------ sf_rows_append
def test_rows_append_fills_the_store_and_counts_overflow():
    import sfhip
    K, cap = 157, 11
    g = torch.Generator().manual_seed(5)
    whole = torch.full((1 + cap + 1, K), -777.0, device="cuda")  # guard rows around both stores
    whole_l = whole.clone()
    store_p, store_l = whole[1:1 + cap], whole_l[1:1 + cap]
    cursor = torch.zeros(2, dtype=torch.int32, device="cuda")
    batches = []
    for n, pad in ((5, 0), (2, 3), (4, 0)):  # unequal batches, one of them a view of wider rows: cap exactly full
        p = torch.randn(n, K + pad, generator=g).cuda()[:, :K]
        lab = (torch.rand(n, K + pad, generator=g) < 0.3).float().cuda()[:, :K]
        sfhip.rows_append(p, lab, store_p, store_l, cursor)
        batches.append((p, lab))
    want_p, want_l = torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches])
    assert cursor.cpu().tolist() == [cap, 0]
    assert torch.equal(store_p.view(torch.int32), want_p.contiguous().view(torch.int32))
    assert torch.equal(store_l.view(torch.int32), want_l.contiguous().view(torch.int32))
    # one row too many: counted, nothing written
    sfhip.rows_append(torch.ones(1, K, device="cuda"), torch.ones(1, K, device="cuda"), store_p, store_l, cursor)
    assert cursor.cpu().tolist() == [cap, 1]
    assert torch.equal(store_p, want_p) and torch.equal(store_l, want_l)
    for w in (whole, whole_l):
        assert bool((w[0] == -777.0).all()) and bool((w[-1] == -777.0).all())
    # a batch that fits in part: the rows that fit are stored, the rest counted
    cursor.copy_(torch.tensor([cap - 2, 0], dtype=torch.int32))
    sfhip.rows_append(torch.full((3, K), 2.0, device="cuda"), torch.zeros(3, K, device="cuda"), store_p, store_l, cursor)
    assert cursor.cpu().tolist() == [cap, 1]
    assert bool((store_p[cap - 2:] == 2.0).all()) and torch.equal(store_p[:cap - 2], want_p[:cap - 2])
    assert bool((whole[-1] == -777.0).all())


# ------------------------------------------------------------------------------------------------ the test meter
def _feed(meter, vectors, bs, labels=None):
    n = vectors["meter/preds"].shape[0]
    labels = vectors["meter/labels"] if labels is None else labels
    for s in range(0, n, bs):
        meter.update_stats(torch.from_numpy(vectors["meter/preds"][s:s + bs]).cuda(),
                           torch.from_numpy(labels[s:s + bs]).cuda(),
                           torch.from_numpy(vectors["meter/clip_ids"][s:s + bs]).cuda())


@pytest.mark.parametrize("method", ["max", "sum"])
def test_device_multilabel_test_meter_matches_reference(vectors, method):
    from slowfast.utils.meters import DeviceMultiLabelTestMeter
    meta = json.loads(str(vectors["meta"]))
    nv, nc, ncls, bs = meta["num_videos"], meta["num_clips"], meta["num_cls"], meta["batch"]
    m = DeviceMultiLabelTestMeter(nv, nc, ncls, 4, ensemble_method=method)
    for _ in range(2):  # the second pass after reset(): the rows start from -1e10 again
        _feed(m, vectors, bs)
        assert np.array_equal(m.video_preds.cpu().numpy().view(np.int32),
                              vectors["meter/%s/video_preds" % method].view(np.int32))
        assert np.array_equal(m.video_labels.cpu().numpy(), vectors["meter/%s/video_labels" % method])
        assert np.array_equal(m.clip_count.cpu().numpy(), vectors["meter/%s/clip_count" % method])
        assert m.bad_count.cpu().tolist() == [0, 0]
        stats = m.finalize_metrics()
        assert stats["split"] == "test_final" and stats["complete"] is True
        assert abs(stats["map"] - float(vectors["meter/%s/map" % method])) <= MAP_TOL
        m.reset()


def test_device_multilabel_test_meter_raises_on_mismatch_and_bad_video(vectors):
    from slowfast.utils.meters import DeviceMultiLabelTestMeter
    meta = json.loads(str(vectors["meta"]))
    nv, nc, ncls, bs = meta["num_videos"], meta["num_clips"], meta["num_cls"], meta["batch"]
    # one clip of a video carries another label row: within a batch or across two, the video's row differs once it
    # holds a positive (every video of the fixture has one)
    labels = vectors["meter/labels"].copy()
    labels[6] = 1.0 - labels[6]
    m = DeviceMultiLabelTestMeter(nv, nc, ncls, 4, ensemble_method="max")
    _feed(m, vectors, bs, labels)
    assert m.bad_count.cpu().tolist()[0] == 0 and m.bad_count.cpu().tolist()[1] >= 1
    with pytest.raises(ValueError, match="label row"):
        m.finalize_metrics()
    m = DeviceMultiLabelTestMeter(nv, nc, ncls, 4, ensemble_method="max")
    m.update_stats(torch.rand(2, ncls).cuda(), torch.ones(2, ncls).cuda(), torch.tensor([0, nv * nc]).cuda())
    with pytest.raises(IndexError, match="1 clip"):
        m.finalize_metrics()


# ------------------------------------------------------------------------------------------------ the validation meter
class _Cfg(object):
    def __init__(self, log_period, max_epoch, multi_label, topk=5):
        self.LOG_PERIOD, self.NUM_GPUS = log_period, 1
        self.SOLVER = type("S", (), {"MAX_EPOCH": max_epoch})()
        self.DATA = type("D", (), {"MULTI_LABEL": multi_label})()
        self.TRAIN = type("T", (), {"TOPK": topk})()


def test_device_val_meter_single_label_against_a_host_fold():
    from slowfast.utils.meters import DeviceValMeter, topks_correct
    max_iter, period = 7, 3
    g = torch.Generator().manual_seed(9)
    batches = [(torch.rand(8, 10, generator=g).cuda(), torch.randint(0, 10, (8,), generator=g).cuda())
               for _ in range(max_iter)]
    # the reference loop's values: topks_correct and two .item() per batch (train_net.py:227-243)
    errs = [[float((1.0 - x / 8) * 100.0) for x in topks_correct(p, lab, (1, 5))] for p, lab in batches]
    m = DeviceValMeter(max_iter, _Cfg(period, 2, False))
    torch.cuda.synchronize()
    logged, reads = [], []
    with _count_host_reads() as seen:
        for i, (p, lab) in enumerate(batches):
            m.update_stats(p, lab)
            m.update_predictions(p, lab)
            before = len(seen)
            s = m.log_iter_stats(0, i)
            if s is not None:
                logged.append(s)
                reads.append(len(seen) - before)
            else:
                assert len(seen) == before
        before = len(seen)
        epoch = m.log_epoch_stats(0)
        reads.append(len(seen) - before)
    assert reads == [1, 1, 1], seen  # one copy per drain, one for the epoch; none in between
    assert [s["iter"] for s in logged] == ["3/7", "6/7"]
    for s, hi in zip(logged, (3, 6)):
        assert s["top1_err"] == np.median([e[0] for e in errs[hi - 3:hi]])
        assert s["top5_err"] == np.median([e[1] for e in errs[hi - 3:hi]])
    assert epoch["top1_err"] == sum(e[0] * 8 for e in errs) / (8 * max_iter)
    assert epoch["top5_err"] == sum(e[1] * 8 for e in errs) / (8 * max_iter)
    assert epoch["min_top1_err"] == min(100.0, epoch["top1_err"]) and m.num_samples == 8 * max_iter


def test_device_val_meter_multilabel_epoch_matches_reference():
    from slowfast.utils.meters import DeviceValMeter, get_map
    with open(os.path.join(GOLDEN, "val_meter_stats.json")) as f:
        case = json.load(f)["multilabel"]
    max_iter, mb, ncls = case["max_iter"], case["mb_per_gpu"], case["num_cls"]
    rs = np.random.RandomState(case["seed"])
    preds = rs.uniform(0.0, 1.0, (max_iter * mb, ncls)).astype(np.float32)
    labels = (rs.uniform(0.0, 1.0, (max_iter * mb, ncls)) < 0.35).astype(np.float32)
    want = case["logged"][-1]
    m = DeviceValMeter(max_iter, _Cfg(case["log_period"], case["max_epoch"], True))
    for epoch in range(2):  # the second epoch after reset() fills the store from row 0 again
        with _count_host_reads() as seen:
            for i in range(max_iter):
                m.update_stats(None, None)
                m.update_predictions(torch.from_numpy(preds[i * mb:(i + 1) * mb]).cuda(),
                                     torch.from_numpy(labels[i * mb:(i + 1) * mb]).cuda().double())
                m.log_iter_stats(0, i)
            assert seen == []
            stats = m.log_epoch_stats(0)
            assert len(seen) == 1, seen
        assert m.cap == max_iter * mb and set(stats) - {"time_diff", "gpu_mem", "RAM"} == set(want)
        assert abs(stats["map"] - want["map"]) <= MAP_TOL and abs(get_map(preds, labels) - want["map"]) <= MAP_TOL
        m.reset()
    # one batch more than max_iter: the store is full, the epoch refuses
    for i in range(max_iter + 1):
        m.update_predictions(torch.from_numpy(preds[:mb]).cuda(), torch.from_numpy(labels[:mb]).cuda())
    with pytest.raises(RuntimeError, match="cap = %d" % (max_iter * mb)):
        m.log_epoch_stats(0)


# ------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_device_val_meter_multilabel_epoch_over_two_ranks():
    """A process per rank on a GPU of its own (RCCL): each appends its own batches, the epoch's end gathers the filled
    rows of both once, and every rank reports the mAP of all rows with one copy to the host."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import _val_map_worker as w
    from slowfast.utils.meters import get_map
    world, out, port = 2, tempfile.mkdtemp(), str(_free_port())
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                    "_val_map_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o.decode(errors="replace")[-3000:])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    preds, labels = w.epoch_rows(world)
    # the gathered matrix: rank 0's rows, then rank 1's (mAP does not depend on the order beyond the last bits)
    order = np.concatenate([np.arange(lo, hi) for r in range(world) for lo, hi in w.rank_batches(world, r)])
    assert sorted(order.tolist()) == list(range(len(preds)))
    want = get_map(preds[order], labels[order])
    for r in range(world):
        with open(os.path.join(out, "valmap_rank%d.json" % r)) as f:
            rep = json.load(f)
        assert rep["rows"] == rep["cap"] == w.MAX_ITER * w.MB and rep["host_reads"] == 1, rep
        assert abs(rep["map"] - want) <= MAP_TOL, (rep, want)
