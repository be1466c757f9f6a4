"""Host side of validation and multi-label evaluation: `get_map` (numpy) against the reference's recorded results
(tests/golden/make_golden_map.py -> map_vectors.npz) and, where scikit-learn is installed, against scikit-learn on
fresh seeds; its refusals; the multi-label TestMeter end to end; DeviceValMeter's drain over a CPU ring filled by hand
against the reference ValMeter's records (val_meter_stats.json); the new rows of the signature table; every refusal of
the four entry points and the workspace query (checked before any launch, so callable without a GPU)."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _map_cases import case_names, make_case
from _util import GOLDEN

FAKE = 0x7f0000001000  # a non-null, 16-byte aligned "device address": a refused call never dereferences it
MAP_TOL = 1e-12        # N * 4 * 2^-53 at the largest N (2048): a rounding per division, sklearn's recall difference and
                       # product, a rounding per addition


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(GOLDEN, "map_vectors.npz"))


def _val_golden():
    with open(os.path.join(GOLDEN, "val_meter_stats.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ get_map
@pytest.mark.parametrize("name", case_names())
def test_get_map_matches_reference(vectors, name):
    from slowfast.utils.meters import average_precisions, get_map
    preds, labels = make_case(name)
    want_map, want_ap = float(vectors[name + "/map"]), vectors[name + "/ap"]
    got_ap = average_precisions(preds, labels)
    assert np.array_equal(got_ap < 0, want_ap < 0)  # the same classes are left out
    assert np.abs(got_ap - want_ap).max() <= MAP_TOL
    assert abs(get_map(preds, labels) - want_map) <= MAP_TOL
    if name == "all_empty":
        assert get_map(preds, labels) == 0.0 and want_map == 0.0


def test_get_map_matches_sklearn_on_fresh_seeds():
    metrics = pytest.importorskip("sklearn.metrics")
    from slowfast.utils.meters import get_map
    for seed, (n, c, q) in enumerate([(1, 3, 0), (5, 4, 4), (300, 12, 0), (513, 7, 16), (2048, 5, 8)]):
        rs = np.random.RandomState(500 + seed)
        preds = rs.standard_normal((n, c)).astype(np.float32)
        if q:
            preds = (np.round(preds * q) / q).astype(np.float32)
        labels = (rs.uniform(0, 1, (n, c)) < 0.4).astype(np.float32)
        keep = labels.any(axis=0)
        if not keep.any():
            continue
        want = np.mean([metrics.average_precision_score(labels[:, k], preds[:, k]) for k in np.nonzero(keep)[0]])
        assert abs(get_map(preds, labels) - want) <= MAP_TOL


def test_get_map_refuses_what_the_reference_turns_into_zero():
    from slowfast.utils.meters import get_map
    preds, labels = make_case("untied_n7_c17")
    for bad in (np.nan, np.inf, -np.inf):
        p = preds.copy()
        p[3, 2] = bad
        with pytest.raises(ValueError, match="1 element"):
            get_map(p, labels)
    lab = labels.copy()
    lab[0, 0], lab[1, 4] = 0.5, 2.0
    with pytest.raises(ValueError, match="2 element"):
        get_map(preds, lab)
    with pytest.raises(ValueError):
        get_map(preds, labels[:, :5])


def test_zero_signs_are_one_threshold():
    from slowfast.utils.meters import average_precisions
    preds = np.array([[-0.0], [0.0], [1.0]], dtype=np.float32)
    labels = np.array([[1.0], [0.0], [0.0]], dtype=np.float32)
    # the positive's threshold holds all three scores >= -0.0, one of them positive
    assert average_precisions(preds, labels)[0] == 1.0 / 3.0


# ------------------------------------------------------------------------------------------------ TestMeter
@pytest.mark.parametrize("method", ["max", "sum"])
def test_multilabel_test_meter_matches_reference(vectors, method):
    """Raised NotImplementedError before the multi-label route existed."""
    from slowfast.utils.meters import TestMeter
    meta = json.loads(str(vectors["meta"]))
    nv, nc, ncls, bs = meta["num_videos"], meta["num_clips"], meta["num_cls"], meta["batch"]
    n = nv * nc
    m = TestMeter(nv, nc, ncls, (n + bs - 1) // bs, multi_label=True, ensemble_method=method)
    for s in range(0, n, bs):
        m.update_stats(torch.from_numpy(vectors["meter/preds"][s:s + bs]),
                       torch.from_numpy(vectors["meter/labels"][s:s + bs]),
                       torch.from_numpy(vectors["meter/clip_ids"][s:s + bs]))
    assert np.array_equal(m.video_preds.numpy(), vectors["meter/%s/video_preds" % method])
    assert np.array_equal(m.video_labels.numpy(), vectors["meter/%s/video_labels" % method])
    assert np.array_equal(m.clip_count.numpy(), vectors["meter/%s/clip_count" % method])
    stats = m.finalize_metrics()
    assert stats["split"] == "test_final" and stats["complete"] is True
    assert abs(stats["map"] - float(vectors["meter/%s/map" % method])) <= MAP_TOL
    if method == "sum":  # -1e10 absorbs every float32 prediction: all scores tie, AP = the share of positives
        assert (m.video_preds == -1e10).all()


def test_device_meters_refuse_the_other_kind():
    from slowfast.utils.meters import DeviceMultiLabelTestMeter, DeviceTestMeter
    m = DeviceTestMeter(4, 2, 5, 1, multi_label=True, device="cpu")
    with pytest.raises(NotImplementedError, match="multi-label.*DeviceMultiLabelTestMeter"):
        m.finalize_metrics()
    with pytest.raises(ValueError):
        DeviceMultiLabelTestMeter(4, 2, 5, 1, multi_label=False)
    with pytest.raises(NotImplementedError):
        DeviceMultiLabelTestMeter(4, 2, 5, 1, ensemble_method="mean")


# ------------------------------------------------------------------------------------------------ DeviceValMeter
class _Cfg(object):
    def __init__(self, case):
        self.LOG_PERIOD, self.NUM_GPUS = case["log_period"], case["num_gpus"]
        self.SOLVER = type("S", (), {"MAX_EPOCH": case["max_epoch"]})()
        self.DATA = type("D", (), {"MULTI_LABEL": case["multi_label"]})()
        self.TRAIN = type("T", (), {"TOPK": 5})()


def _write_batch(ring, top1, top5, mb, flag=0.0, bad=0.0, kind=2.0):
    """What sf_topk_errors leaves for one batch, by hand on a CPU ring."""
    row = int(ring.counter[0]) % ring.cap
    ring.rows[row] = torch.tensor([0.0, top1, top5, flag, mb, bad, kind, 0.0])
    ring.counter += 1


def _same_stats(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) - {"time_diff", "eta", "gpu_mem", "RAM"} == set(w)  # the reference's keys and the machine's
        assert {"time_diff", "gpu_mem"} <= set(g) and ("eta" in g) == (g["_type"] == "val_iter")
        for k, v in w.items():
            if isinstance(v, float):
                assert float(g[k]) == v, (k, g[k], v)  # the reference's arithmetic on the same values: equal floats
            else:
                assert g[k] == v, (k, g[k], v)


def _run_val_case(case, scale=1.0, world_cfg=None):
    """The case's epochs through one DeviceValMeter over a CPU ring; the rows hold `scale` times the recorded errors."""
    from slowfast.utils.meters import DeviceValMeter
    cfg = _Cfg(case)
    if world_cfg is not None:
        cfg.NUM_GPUS = world_cfg
    m = DeviceValMeter(case["max_iter"], cfg, device="cpu")
    assert m.ring.cap == case["log_period"] and m.min_top1_err == 100.0 and m.min_top5_err == 100.0
    logged = []
    for ep in case["epochs"]:
        m.iter_tic()
        for i in range(case["max_iter"]):
            _write_batch(m.ring, scale * ep["top1"][i], scale * ep["top5"][i], case["mb_per_gpu"])
            m.iter_toc()
            m.update_predictions(torch.zeros(2, 3), torch.zeros(2, 3))  # single-label: a no-op, nothing is kept
            s = m.log_iter_stats(ep["cur_epoch"], i)
            if s is not None:
                logged.append(s)
            m.iter_tic()
        logged.append(m.log_epoch_stats(ep["cur_epoch"]))
        m.reset()
    assert m.all_preds is None
    return logged


def test_val_meter_drain_matches_reference_val_meter():
    case = _val_golden()["period3"]
    logged = _run_val_case(case)
    kinds = [s["_type"] for s in case["logged"]]
    assert kinds == ["val_iter", "val_iter", "val_epoch"] * 2
    _same_stats(logged, case["logged"])
    # the second epoch was worse: its minimum is the first one's
    assert logged[-1]["min_top1_err"] == logged[2]["top1_err"] < logged[-1]["top1_err"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _drain_worker(rank, world, port, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(here), "efficient-slowfast_amd"), here):
        sys.path.insert(0, p)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        # rank 0 holds zeros and rank 1 twice the recorded errors: only the all-reduced mean is the recorded sequence
        # (doubling and halving are exact in float32)
        got = _run_val_case(_val_golden()["period2_world2"], scale=2.0 * rank, world_cfg=world)
        if rank == 0:
            torch.save(got, out)
    finally:
        dist.destroy_process_group()


def test_val_meter_drain_reduces_over_two_ranks(tmp_path):
    """Two gloo ranks: the drain all-reduces the ring block and counts mb_per_gpu x world samples per batch."""
    out = str(tmp_path / "stats.pt")
    mp.spawn(_drain_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    case = _val_golden()["period2_world2"]
    assert case["num_gpus"] == 2
    _same_stats(torch.load(out, weights_only=False), case["logged"])


def test_val_meter_drain_errors():
    from slowfast.utils.meters import DeviceValMeter
    case = _val_golden()["period3"]
    m = DeviceValMeter(case["max_iter"], _Cfg(case), device="cpu")
    _write_batch(m.ring, 50.0, 25.0, 8, bad=1.0)
    with pytest.raises(ValueError, match=r"label\(s\) outside \[0, classes\)"):
        m.drain()
    m = DeviceValMeter(case["max_iter"], _Cfg(case), device="cpu")
    _write_batch(m.ring, 50.0, 25.0, 8, kind=0.0)
    with pytest.raises(RuntimeError, match="ring of its own"):
        m.drain()
    m = DeviceValMeter(case["max_iter"], _Cfg(case), device="cpu")
    for _ in range(case["log_period"] + 1):
        _write_batch(m.ring, 50.0, 25.0, 8)
    with pytest.raises(RuntimeError, match="drain at least every LOG_PERIOD"):
        m.drain()
    multi = _val_golden()["multilabel"]
    m = DeviceValMeter(multi["max_iter"], _Cfg(multi), device="cpu")
    m.update_stats(torch.zeros(2, 3), torch.zeros(2, dtype=torch.long))  # multi-label: a no-op
    assert int(m.ring.counter[0]) == 0
    with pytest.raises(RuntimeError, match="no predictions"):
        m.log_epoch_stats(0)


def test_val_meter_multilabel_iteration_records():
    """The multi-label val_iter records need no device: no errors, no drain."""
    from slowfast.utils.meters import DeviceValMeter
    case = _val_golden()["multilabel"]
    m = DeviceValMeter(case["max_iter"], _Cfg(case), device="cpu")
    logged = [s for s in (m.log_iter_stats(case["cur_epoch"], i) for i in range(case["max_iter"])) if s is not None]
    _same_stats(logged, case["logged"][:-1])
    assert case["logged"][-1]["_type"] == "val_epoch" and "map" in case["logged"][-1]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_signature_table_has_the_new_entry_points():
    import sfhip
    vp, ci, cl, pi = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, sfhip._pi
    want = {
        "sf_topk_errors": (ci, [vp, ci, vp, ci, ci, ci, vp, pi, ci, vp]),
        "sf_rows_append": (ci, [vp, ci, vp, ci, ci, ci, vp, vp, pi, ci, vp]),
        "sf_ensemble_update_ml": (ci, [vp, vp, vp, ci, vp, vp, pi, pi, ci, ci, ci, ci, vp]),
        "sf_map_ws_bytes": (cl, [ci, ci]),
        "sf_map": (ci, [vp, ci, vp, ci, ci, ci, vp, vp, vp, vp]),
    }
    for name, sig in want.items():
        assert sfhip._SIGNATURES[name] == sig, name
        assert hasattr(sfhip.lib(), name)
    from slowfast.models import step_tail as st
    assert (st.KIND_CE, st.KIND_BCE, st.KIND_EVAL) == (0, 1, 2)


def _rc(symbol, args, **change):
    import sfhip
    args = list(args)
    for k, v in change.items():
        args[int(k[1:])] = v
    return getattr(sfhip.lib(), symbol)(*args)


def _refusals(symbol, good, pointers, sizes, optional=()):
    import sfhip
    E = sfhip.SF_EINVAL
    for i in pointers:
        assert _rc(symbol, good, **{"a%d" % i: None}) == E, (symbol, i)
    for i, bad in sizes:
        for v in bad:
            assert _rc(symbol, good, **{"a%d" % i: v}) == E, (symbol, i, v)


def test_topk_errors_refusals():
    import sfhip
    p, cnt = ctypes.c_void_p(FAKE), ctypes.cast(ctypes.c_void_p(FAKE), sfhip._pi)
    good = [p, 10, p, 4, 10, 5, p, cnt, 3, None]  # preds ld labels N K k_hi ring counter cap stream
    _refusals("sf_topk_errors", good, (0, 2, 6, 7),
              [(1, (9, 0)), (3, (0, -1)), (4, (0, -3)), (5, (0, -1, 11)), (8, (0, -1))])


def test_rows_append_refusals():
    import sfhip
    p, cur = ctypes.c_void_p(FAKE), ctypes.cast(ctypes.c_void_p(FAKE), sfhip._pi)
    good = [p, 10, p, 12, 4, 10, p, p, cur, 8, None]  # preds ldp labels ldl N K store_preds store_labels cursor cap
    _refusals("sf_rows_append", good, (0, 2, 6, 7, 8),
              [(1, (9,)), (3, (9,)), (4, (0, -1)), (5, (0, -2)), (9, (0, -1))])


def test_ensemble_update_ml_refusals():
    import sfhip
    p, ip = ctypes.c_void_p(FAKE), ctypes.cast(ctypes.c_void_p(FAKE), sfhip._pi)
    # preds video_idx labels ldl video_preds video_labels clip_count bad_count B K Nv mode
    good = [p, p, p, 7, p, p, ip, ip, 4, 7, 5, 1, None]
    _refusals("sf_ensemble_update_ml", good, (0, 1, 2, 4, 5, 6, 7),
              [(3, (6, 0)), (8, (0, -1)), (9, (0, -1)), (10, (0, -1)), (11, (2, -1))])


def test_map_refusals_and_workspace():
    import sfhip
    L = sfhip.lib()
    p = ctypes.c_void_p(FAKE)
    good = [p, 17, p, 20, 300, 17, p, p, None, None]  # scores lds labels ldl N C ws out ap stream
    _refusals("sf_map", good, (0, 2, 6, 7), [(1, (16,)), (3, (16,)), (4, (0, -1, 65535 * 256 + 1)), (5, (0, -1))])
    for i in (6, 7, 8):  # fp64 buffers on 8 bytes
        assert _rc("sf_map", good, **{"a%d" % i: ctypes.c_void_p(FAKE + 4)}) == sfhip.SF_EALIGN, i
    # a (class, block of 256 candidates) partial is three doubles
    for n, c in ((1, 1), (256, 1), (257, 1), (1863, 157), (2048, 33)):
        assert L.sf_map_ws_bytes(n, c) == -(-n // 256) * c * 3 * 8, (n, c)
    assert L.sf_map_ws_bytes(65535 * 256, 2) == 65535 * 2 * 24
    for n, c in ((0, 5), (-1, 5), (5, 0), (5, -1), (65535 * 256 + 1, 1)):
        assert L.sf_map_ws_bytes(n, c) == 0, (n, c)


def test_python_entries_refuse_cpu_tensors():
    import sfhip
    from slowfast.models import step_tail as st
    from slowfast.utils.meters import device_map
    ring = st.StatsRing(2, device="cpu")
    with pytest.raises(sfhip.SfhipError):
        st.topk_errors(torch.rand(3, 5), torch.zeros(3, dtype=torch.long), 1, ring)
    with pytest.raises(sfhip.SfhipError):
        device_map(torch.rand(3, 5), torch.zeros(3, 5))
    with pytest.raises(sfhip.SfhipError):
        sfhip.rows_append(torch.rand(3, 5), torch.zeros(3, 5), torch.zeros(8, 5), torch.zeros(8, 5),
                          torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        sfhip.mean_ap(torch.rand(3, 5), torch.zeros(3, 4))
