"""Per-class evaluation, the part that needs no GPU: the brute-force restatement (tests/_class_report_ref.py) against
cases written out by hand, the invariants that tie it to the top-k counts, every refusal of sf_confusion_update /
sf_class_report (decided before any launch, so callable without a GPU), the binding's rows, the meters' argument
handling, and DevicePerClassMeter.all_reduce over two gloo ranks on host counters."""
import ctypes
import inspect
import os
import random
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _class_report_ref as ref

FAKE = 0x7f0000001000  # a non-null, 16-byte aligned "device address": a refused call never dereferences it

# 3 classes, 7 rows; the comments give (predicted class, position of the label in the row's order)
ROWS7 = [([0.8, 0.1, 0.1], 0),   # 0, 0
         ([0.2, 0.5, 0.3], 0),   # 1, 2
         ([0.1, 0.7, 0.2], 1),   # 1, 0
         ([0.3, 0.3, 0.4], 1),   # 2, 2: class 0 ties the label's 0.3 and has the lower index
         ([0.1, 0.2, 0.7], 2),   # 2, 0
         ([0.6, 0.3, 0.1], 2),   # 0, 2
         ([0.4, 0.5, 0.1], 0)]   # 1, 1


def _counts(rows, K, k_hi):
    return ref.confusion_update(ref.empty_counts(K), [r for r, _ in rows], [l for _, l in rows], k_hi)


# ------------------------------------------------------------------------------------------------ the restatement
def test_seven_rows_three_classes_by_hand():
    c = _counts(ROWS7, 3, 2)
    assert c["conf"] == [[1, 2, 0], [0, 1, 1], [1, 0, 1]]
    assert c["hits"] == [[1, 2], [1, 1], [1, 1]] and c["refused"] == [0, 0]
    summary, table = ref.class_report(c)
    assert [row[0] for row in table] == [3.0, 2.0, 2.0]
    assert [row[1] for row in table] == [1 / 2, 1 / 3, 1 / 2]          # TP / column sum
    assert [row[2] for row in table] == [1 / 3, 1 / 2, 1 / 2]          # TP / support
    assert [row[3] for row in table] == [2 / 5, 2 / 5, 2 / 4]          # 2 TP / (column sum + support)
    assert [row[4] for row in table] == [1 / 3, 1 / 2, 1 / 2] and [row[5] for row in table] == [2 / 3, 1 / 2, 1 / 2]
    assert summary["samples"] == 7 and summary["accuracy"] == 3 / 7
    assert summary["macro_recall"] == (1 / 3 + 1 / 2 + 1 / 2) / 3 == summary["mean_class_accuracy"]
    assert summary["macro_precision"] == (1 / 2 + 1 / 3 + 1 / 2) / 3
    assert summary["macro_f1"] == (2 / 5 + 2 / 5 + 2 / 4) / 3
    assert summary["classes_with_support"] == 3 and summary["classes_never_predicted"] == 0


def test_a_tie_in_the_top_1_goes_to_the_lower_index():
    c = _counts([([0.5, 0.5, 0.0], 1), ([0.5, 0.5, 0.0], 0)], 3, 2)
    assert c["conf"] == [[1, 0, 0], [1, 0, 0], [0, 0, 0]]       # both rows predict class 0
    assert c["hits"] == [[1, 1], [0, 1], [0, 0]]                # label 1 is second: a top-2 hit only
    # -0.0 ties +0.0: the lower index is predicted whatever the sign
    c = _counts([([-0.0, 0.0, -1.0], 1), ([0.0, -0.0, -1.0], 1)], 3, 1)
    assert c["conf"] == [[0, 0, 0], [2, 0, 0], [0, 0, 0]] and c["hits"][1] == [0, 0]
    assert ref.row_order([1.0, 2.0, 2.0, 1.0]) == [1, 2, 0, 3]


def test_class_never_predicted_and_class_without_support():
    # 4 classes: class 2 is never predicted (but has support), class 3 has no support (but is predicted once)
    rows = [([0.9, 0.0, 0.1, 0.0], 0), ([0.1, 0.8, 0.1, 0.0], 1), ([0.6, 0.1, 0.3, 0.0], 2), ([0.1, 0.1, 0.2, 0.6], 1)]
    c = _counts(rows, 4, 2)
    assert c["conf"] == [[1, 0, 0, 0], [0, 1, 0, 1], [1, 0, 0, 0], [0, 0, 0, 0]]
    summary, table = ref.class_report(c)
    assert table[2] == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0]  # precision 0 / 0 -> 0; the label was second: a top-2 hit
    assert table[3] == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]  # no support: every ratio 0, left out of the means
    assert summary["classes_with_support"] == 3 and summary["classes_never_predicted"] == 1
    assert summary["macro_precision"] == (1 / 2 + 1.0 + 0.0) / 3 and summary["macro_recall"] == (1.0 + 1 / 2 + 0.0) / 3
    assert summary["accuracy"] == 2 / 4
    # nothing at all: every mean is 0, no division
    summary, table = ref.class_report(ref.empty_counts(2))
    assert summary == dict(zip(ref.SUMMARY_FIELDS, (0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 2))) and table == [[0.0] * 6] * 2


def test_refused_rows_add_to_nothing_else():
    nan, inf = float("nan"), float("inf")
    rows = [([0.1, 0.9], -1), ([0.1, 0.9], 2), ([nan, 0.9], 1), ([0.1, -inf], 0), ([nan, 0.2], 5), ([0.1, 0.9], 1)]
    c = _counts(rows, 2, 1)
    assert c["refused"] == [3, 2]  # a bad label is decided first: the row with both counts as a bad label
    assert c["conf"] == [[0, 0], [0, 1]] and c["hits"] == [[0, 0], [1, 1]]


@pytest.mark.parametrize("K,N,k_hi,levels", [(3, 50, 2, 4), (5, 64, 3, 3), (12, 40, 5, 0)])
def test_invariants_on_seeded_rows(K, N, k_hi, levels):
    """trace = the top-1 hits, sum(hits[:, 1]) = the top-k hits, row sums = support, column sums = predicted counts —
    with ties (scores drawn from `levels` values), bad labels and non-finite rows mixed in."""
    rng = random.Random(K * 1000 + N)
    preds = [[(rng.randrange(levels) / levels if levels else rng.random()) for _ in range(K)] for _ in range(N)]
    labels = [rng.randrange(K) for _ in range(N)]
    labels[3], labels[7] = -1, K
    preds[5][rng.randrange(K)] = float("nan")
    preds[9][rng.randrange(K)] = float("inf")
    c = ref.confusion_update(ref.empty_counts(K), preds, labels, k_hi)
    assert c["refused"] == [2, 2]
    accepted = [i for i in range(N) if i not in (3, 7, 5, 9)]
    assert sum(map(sum, c["conf"])) == N - 4
    assert sum(c["conf"][k][k] for k in range(K)) == ref.topk_hits(preds, labels, 1) == sum(h[0] for h in c["hits"])
    assert sum(h[1] for h in c["hits"]) == ref.topk_hits(preds, labels, k_hi)
    for k in range(K):
        assert sum(c["conf"][k]) == sum(1 for i in accepted if labels[i] == k)                        # support
        assert sum(c["conf"][j][k] for j in range(K)) == sum(1 for i in accepted if ref.row_order(preds[i])[0] == k)
        assert c["hits"][k][0] == c["conf"][k][k] and c["hits"][k][0] <= c["hits"][k][1] <= sum(c["conf"][k])
    # the predicted class is torch.topk's first index for untied rows, and the hits are topks_correct's
    if levels == 0:
        from slowfast.utils.meters import topks_correct
        keep = torch.tensor(accepted)
        p, lab = torch.tensor(preds)[keep], torch.tensor(labels)[keep]
        got = [int(x) for x in topks_correct(p, lab, (1, k_hi))]
        assert got == [ref.topk_hits(preds, labels, 1), ref.topk_hits(preds, labels, k_hi)]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_signature_table_has_the_new_entry_points():
    import sfhip
    vp, ci = ctypes.c_void_p, ctypes.c_int
    want = {"sf_confusion_small_kmax": (ci, []),
            "sf_confusion_update": (ci, [vp, ci, vp, ci, ci, ci, vp, vp, vp, vp]),
            "sf_class_report": (ci, [vp, vp, ci, vp, vp, vp])}
    for name, sig in want.items():
        assert sfhip._SIGNATURES[name] == sig, name
        assert hasattr(sfhip.lib(), name)


def test_small_route_boundary_is_the_lds_budget():
    """The largest K whose K*K + 2K + 2 four-byte counters fit 160 KiB - 512 B of LDS."""
    import sfhip
    kmax = sfhip.lib().sf_confusion_small_kmax()
    budget = 160 * 1024 - 512
    assert (kmax * kmax + 2 * kmax + 2) * 4 <= budget < ((kmax + 1) ** 2 + 2 * (kmax + 1) + 2) * 4
    assert kmax == 201 and 27 <= kmax < 400  # Jester and the fork's 3 classes on the LDS route, Kinetics on the other


def _rc(symbol, args, **change):
    import sfhip
    args = list(args)
    for k, v in change.items():
        args[int(k[1:])] = v
    return getattr(sfhip.lib(), symbol)(*args)


def test_confusion_update_refusals():
    import sfhip
    p = ctypes.c_void_p(FAKE)
    good = [p, 10, p, 4, 10, 5, p, p, p, None]  # preds ld labels N K k_hi conf hits refused stream
    for i in (0, 2, 6, 7, 8):
        assert _rc("sf_confusion_update", good, **{"a%d" % i: None}) == sfhip.SF_EINVAL, i
    for i, bad in [(1, (9, 0, -1)), (3, (0, -1)), (4, (0, -3)), (5, (0, -1, 11))]:
        for v in bad:
            assert _rc("sf_confusion_update", good, **{"a%d" % i: v}) == sfhip.SF_EINVAL, (i, v)
    for K in (3, 201, 202, 400):  # both routes check the same things
        g = [p, K, p, 4, K, 1, p, p, p, None]
        assert _rc("sf_confusion_update", g, a5=K + 1) == sfhip.SF_EINVAL, K
        assert _rc("sf_confusion_update", g, a1=K - 1) == sfhip.SF_EINVAL, K
    for i in (2, 6, 7, 8):  # int64 buffers on 8 bytes
        assert _rc("sf_confusion_update", good, **{"a%d" % i: ctypes.c_void_p(FAKE + 4)}) == sfhip.SF_EALIGN, i
    for off in (1, 2, 3):   # fp32 rows on 4 bytes (4, 8 and 12 are views: the 4-byte form serves them)
        assert _rc("sf_confusion_update", good, a0=ctypes.c_void_p(FAKE + off)) == sfhip.SF_EALIGN, off
    # a refusal for a size comes before one for alignment
    assert _rc("sf_confusion_update", good, a3=0, a6=ctypes.c_void_p(FAKE + 4)) == sfhip.SF_EINVAL


def test_class_report_refusals():
    import sfhip
    p = ctypes.c_void_p(FAKE)
    good = [p, p, 3, p, p, None]  # conf hits K out per_class stream
    for i in (0, 1, 3, 4):
        assert _rc("sf_class_report", good, **{"a%d" % i: None}) == sfhip.SF_EINVAL, i
        assert _rc("sf_class_report", good, **{"a%d" % i: ctypes.c_void_p(FAKE + 4)}) == sfhip.SF_EALIGN, i
    for K in (0, -1, 1025, 4096):  # one workgroup serves K <= 1024
        assert _rc("sf_class_report", good, a2=K) == sfhip.SF_EINVAL, K


def test_python_entries_refuse_cpu_tensors():
    import sfhip
    from slowfast.utils.meters import DevicePerClassMeter
    m = DevicePerClassMeter(3, 2, device="cpu")
    with pytest.raises(sfhip.SfhipError):
        m.update(torch.zeros(2, 3), torch.zeros(2, dtype=torch.long))
    with pytest.raises(sfhip.SfhipError):
        m.finalize()
    with pytest.raises(ValueError, match=r"preds \[N, 3\]"):
        m.update(torch.zeros(2, 4), torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError):
        sfhip.confusion_update(torch.zeros(2, 3), torch.zeros(3, dtype=torch.long), 1, m.conf, m.hits, m.refused)


# ------------------------------------------------------------------------------------------------ the meters' arguments
class _Cfg(object):
    def __init__(self, multi_label):
        self.LOG_PERIOD, self.NUM_GPUS = 2, 1
        self.SOLVER = type("S", (), {"MAX_EPOCH": 1})()
        self.DATA = type("D", (), {"MULTI_LABEL": multi_label})()
        self.TRAIN = type("T", (), {"TOPK": 2})()


def test_per_class_meter_arguments_and_layout():
    from slowfast.utils.meters import PER_CLASS_COLUMNS, SUMMARY_FIELDS, DevicePerClassMeter
    assert PER_CLASS_COLUMNS == ref.PER_CLASS_COLUMNS and SUMMARY_FIELDS == ref.SUMMARY_FIELDS
    for K, k_hi in ((0, 1), (-2, 1), (1025, 5), (3, 0), (3, 4)):
        with pytest.raises(ValueError):
            DevicePerClassMeter(K, k_hi, device="cpu")
    m = DevicePerClassMeter(4, 2, device="cpu")
    # one flat buffer: conf, hits, refused (what all_reduce sums), then the fp64 report
    assert m.state.numel() == 16 + 8 + 2 and m._buf.numel() == m.state.numel() + 8 + 24
    assert m.state.data_ptr() == m.conf.data_ptr() == m._buf.data_ptr()
    assert m.hits.data_ptr() == m._buf.data_ptr() + 8 * 16 and m.refused.data_ptr() == m._buf.data_ptr() + 8 * 24
    assert m.summary.data_ptr() == m._buf.data_ptr() + 8 * 26 and m.summary.dtype == torch.float64
    assert tuple(m.per_class.shape) == (4, 6) and m.per_class.data_ptr() == m.summary.data_ptr() + 64
    m.conf[1, 2] = 5
    m.per_class[3, 5] = 0.25
    m.reset()
    assert int(m._buf.abs().sum()) == 0


def test_meters_take_per_class_and_multilabel_meters_refuse_it():
    from slowfast.utils.meters import (DeviceMultiLabelTestMeter, DevicePerClassMeter, DeviceTestMeter,
                                       DeviceValMeter)
    for cls in (DeviceValMeter, DeviceTestMeter, DeviceMultiLabelTestMeter):
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[-1] == "per_class" and params["per_class"].default is None, cls
    # the parameters in front of it are the ones the meters had, with their defaults
    val = inspect.signature(DeviceValMeter.__init__).parameters
    assert [(n, p.default) for n, p in val.items()][1:-1] == [
        ("max_iter", inspect.Parameter.empty), ("cfg", inspect.Parameter.empty), ("ring", None), ("device", "cuda")]
    test = inspect.signature(DeviceTestMeter.__init__).parameters
    assert [(n, p.default) for n, p in test.items()][1:-1] == [
        ("num_videos", inspect.Parameter.empty), ("num_clips", inspect.Parameter.empty),
        ("num_cls", inspect.Parameter.empty), ("overall_iters", inspect.Parameter.empty), ("multi_label", False),
        ("ensemble_method", "sum"), ("device", "cuda")]
    pc = DevicePerClassMeter(3, 2, device="cpu")
    assert DeviceValMeter(4, _Cfg(False), device="cpu").per_class is None
    assert DeviceValMeter(4, _Cfg(False), device="cpu", per_class=pc).per_class is pc
    assert DeviceTestMeter(5, 3, 3, 4, device="cpu").per_class is None
    assert DeviceTestMeter(5, 3, 3, 4, device="cpu", per_class=pc).per_class is pc
    with pytest.raises(ValueError, match="single-label"):
        DeviceValMeter(4, _Cfg(True), device="cpu", per_class=pc)
    with pytest.raises(ValueError, match="single-label"):
        DeviceTestMeter(5, 3, 3, 4, multi_label=True, device="cpu", per_class=pc)
    with pytest.raises(ValueError, match="single-label"):
        DeviceMultiLabelTestMeter(5, 3, 3, 4, device="cpu", per_class=pc)
    with pytest.raises(ValueError, match="counts 3 classes"):
        DeviceTestMeter(5, 3, 7, 4, device="cpu", per_class=pc)
    with pytest.raises(TypeError):
        DeviceValMeter(4, _Cfg(False), device="cpu", per_class=object())
    # a validation meter's reset() starts the per-class epoch too
    m = DeviceValMeter(4, _Cfg(False), device="cpu", per_class=pc)
    pc.conf[0, 0] = 3
    m.reset()
    assert int(pc.conf.sum()) == 0


def test_log_report_formats_a_finalized_report(caplog):
    """log_report on a finalize() result written by hand: one json_stats line for the summary, one per class."""
    from slowfast.utils.meters import DevicePerClassMeter
    c = _counts(ROWS7, 3, 2)
    summary, table = ref.class_report(c)
    report = {"confusion": torch.tensor(c["conf"]), "hits": torch.tensor(c["hits"]),
              "per_class": torch.tensor(table, dtype=torch.float64), "summary": summary,
              "refused": {"bad_label": 0, "non_finite": 0}, "k_hi": 2}
    m = DevicePerClassMeter(3, 2, device="cpu")
    with caplog.at_level("INFO", logger="slowfast.utils.meters"):
        records = m.log_report(class_names=["awake", "drowsy", "tired"], report=report)
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("json_stats: ")]
    assert len(records) == len(lines) == 4
    assert records[0]["_type"] == "class_report" and records[0]["samples"] == 7 and records[0]["accuracy"] == 3 / 7
    assert '"accuracy": 0.428571' in lines[0] and '"samples": 7' in lines[0]
    assert records[3] == {"_type": "class_report_class", "class": "tired", "confused_as": [1, 0, 1], "support": 2,
                          "precision": 0.5, "recall": 0.5, "f1": 0.5, "top1_acc": 0.5, "topk_acc": 0.5}
    assert '"class": "tired"' in lines[3] and '"recall": 0.500000' in lines[3]
    assert m.log_report(report=report)[1]["class"] == 0
    with pytest.raises(ValueError, match="2 class names"):
        m.log_report(class_names=["a", "b"], report=report)


# ------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _halves():
    return ROWS7[:4], ROWS7[4:]


def _reduce_worker(rank, world, port, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(here), "efficient-slowfast_amd"), here):
        sys.path.insert(0, p)
    from slowfast.utils.meters import DevicePerClassMeter
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        c = _counts(_halves()[rank], 3, 2)
        m = DevicePerClassMeter(3, 2, device="cpu")
        m.conf.copy_(torch.tensor(c["conf"]))
        m.hits.copy_(torch.tensor(c["hits"]))
        m.refused.copy_(torch.tensor([rank + 1, 10 * (rank + 1)]))
        m.summary.fill_(0.5)  # the report behind the counters is not part of the collective
        m.all_reduce()
        torch.save((m.state.clone(), m.summary.clone()), out % rank)
    finally:
        dist.destroy_process_group()


def test_all_reduce_sums_the_counters_over_two_ranks(tmp_path):
    """Two gloo ranks with host counters: every rank ends with the counts of all rows; at world size 1 nothing moves."""
    from slowfast.utils.meters import DevicePerClassMeter
    out = str(tmp_path / "state%d.pt")
    mp.spawn(_reduce_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    whole = _counts(ROWS7, 3, 2)
    want = [v for row in whole["conf"] for v in row] + [v for row in whole["hits"] for v in row] + [3, 30]
    for rank in range(2):
        state, summary = torch.load(out % rank, weights_only=False)
        assert state.tolist() == want and summary.tolist() == [0.5] * 8, rank
    m = DevicePerClassMeter(3, 2, device="cpu")
    m.conf[2, 1] = 4
    m.all_reduce()
    assert m.conf.tolist() == [[0, 0, 0], [0, 0, 0], [0, 4, 0]]
