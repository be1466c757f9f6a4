"""AVA frame-mAP without a GPU: the numpy restatement (tests/_ava_ref.py) against recorded results of the reference's own
PascalDetectionEvaluator (tests/golden/ava_eval/*.json, written by tests/golden/make_golden_ava.py), the host logic of
slowfast/utils/ava_eval_helper.py (parsing, table layout), DeviceAVAMeter's ground-truth selection and refusals, and the
refusals of sf_ava_ws_bytes / sf_ava_match / sf_ava_ap that are decided before any launch.

tp / fp labels and counts are compared exactly.  AP and mAP at |d| <= 1e-12: the restatement follows the reference's
arithmetic, so the only freedom is numpy's summation order — n <= 600 terms of a few ulp each plus n 2^-53 for the sum,
about 1e-13."""
import ctypes
import glob
import json
import os
from collections import defaultdict

import numpy as np
import pytest
import torch

import _ava_cases as cases
import _ava_ref as ref
from _util import GOLDEN

AP_TOL = 1e-12
RECORDS = sorted(glob.glob(os.path.join(GOLDEN, "ava_eval", "*.json")))


def _evaluate(case):
    return ref.evaluate(case["preds"], case["boxes"], case["metadata"], case["groundtruth"], case["excluded"],
                        case["whitelist"], case["names"])


def _record_case(record):
    i = record["inputs"]
    gt = tuple(defaultdict(list, d) for d in i["groundtruth"])
    return {"preds": np.asarray(i["preds"], np.float32), "boxes": np.asarray(i["boxes"], np.float32),
            "metadata": np.asarray(i["metadata"], np.float32), "groundtruth": gt, "excluded": set(i["excluded"]),
            "whitelist": set(i["whitelist"]), "categories": i["categories"], "names": i["names"]}


def test_every_recorded_case_is_present():
    names = {os.path.splitext(os.path.basename(p))[0] for p in RECORDS}
    assert names == (set(cases.hand_cases()) - {"tied_scores"}) | {"random257"}


@pytest.mark.parametrize("path", RECORDS, ids=lambda p: os.path.splitext(os.path.basename(p))[0])
def test_restatement_matches_the_reference_evaluator(path):
    name = os.path.splitext(os.path.basename(path))[0]
    with open(path) as f:
        record = json.load(f)
    case = _record_case(record)
    # the recorded inputs are the inputs the GPU tests regenerate
    live = cases.random_case(257) if name == "random257" else cases.hand_cases()[name]
    for k in ("preds", "boxes", "metadata"):
        assert np.array_equal(case[k], live[k]), k
    assert [dict(d) for d in live["groundtruth"]] == [dict(d) for d in case["groundtruth"]]
    assert live["excluded"] == case["excluded"] and live["whitelist"] == case["whitelist"]
    want, got = record["expected"], _evaluate(case)
    have = {"%s|%d" % k: [bool(v) for v in labels] for k, (_, labels) in got["per_image"].items()}
    assert have == want["tp_fp"]
    n = len(want["num_gt"])  # the evaluator's classes: 1 .. the largest category id
    assert got["num_gt"][:n].tolist() == want["num_gt"] and not got["num_gt"][n:].any()
    for cid, ap in want["ap"].items():
        if ap is None:
            assert np.isnan(got["ap"][int(cid) - 1]), cid
        else:
            assert abs(got["ap"][int(cid) - 1] - ap) <= AP_TOL, (cid, got["ap"][int(cid) - 1], ap)
    assert abs(got["map"] - want["map"]) <= AP_TOL


def test_hand_cases_by_hand():
    """What each hand-built case must give, worked out on paper."""
    want = {"earlier_row_wins": ([1, 0], 0.5), "iou_exactly_half": ([1], 1.0), "iou_ulp_below_half": ([0], 0.0),
            "identical_gt_boxes": ([1, 0], 0.5), "invalid_box_dropped": ([0, 1], 1.0), "excluded_image": ([1, 0], 1.0),
            "image_without_gt": ([1, 0], 1.0), "gt_image_without_detections": ([1], 1.0 / 3.0),
            "class_without_gt": ([1], 1.0), "class_outside_whitelist": ([1], 0.5), "envelope": ([0, 1, 0, 1, 1], 0.6),
            "tied_scores": ([0, 0, 1, 1, 0, 1], 0.75)}
    hand = cases.hand_cases()
    assert set(want) == set(hand)
    for name, (tp, mean_ap) in want.items():
        got = _evaluate(hand[name])
        assert got["tp"][:, 0].tolist() == tp, name
        assert not got["tp"][:, 1:].any(), name
        assert abs(got["map"] - mean_ap) <= 1e-15, (name, got["map"])
        if name == "class_outside_whitelist":  # class 4's box is kept and nothing may detect it: AP 0, counted
            assert got["num_gt"].tolist() == [1, 0, 0, 1, 0, 0, 0] and got["ap"][3] == 0.0
            assert np.isnan(np.delete(got["ap"], [0, 3])).all()
        else:
            assert np.isnan(got["ap"][1:]).all(), name  # only class 1 has ground truth
    assert _evaluate(hand["invalid_box_dropped"])["valid"].tolist() == [0, 1]
    assert _evaluate(hand["excluded_image"])["valid"].tolist() == [1, 0]
    assert _evaluate(hand["gt_image_without_detections"])["num_gt"][0] == 3
    assert _evaluate(hand["envelope"])["envelope"] == [0]


@pytest.mark.parametrize("K", sorted(cases.RANDOM_SEEDS))
def test_random_seeds_exercise_the_rules(K):
    got = _evaluate(cases.random_case(K))
    assert int(got["tp"].sum()) >= 20 and got["taken"] >= 20 and len(got["envelope"]) >= 1
    for c in range(7):  # scores are distinct within a class
        assert len(set(cases.random_case(K)["preds"][:, c].tolist())) == K


# ------------------------------------------------------------------------------------------------ host logic
def _write_annotations(tmp_path):
    (tmp_path / "gt.csv").write_text(
        "vidA,0904,0.1,0.2,0.5,0.6,3,7\n"
        "vidA,0904,0.1,0.2,0.5,0.6,1,7\n"
        "vidA,0904,0.3,0.3,0.9,0.9,3,8\n"
        "vidA,0904,0.0,0.0,0.2,0.2,9,8\n"      # class 9: not in the label map
        "vidB,0905,0.2,0.2,0.4,0.4,1,1\n"
        "vidB,0908,0.2,0.2,0.4,0.4,2,1\n"
        "vidZ,0912,0.2,0.2,0.4,0.4,2,1\n"      # a video the frame lists do not name
        "vidB,0916,0.5,0.5,0.7,0.7,1,2\n")     # excluded
    (tmp_path / "excl.csv").write_text("vidB,0916\nvidA,1000\n")
    (tmp_path / "labels.pbtxt").write_text(
        'item {\n  name: "bend"\n  id: 1\n}\nitem {\n  name: "crawl"\n  label_id: 2\n}\nitem {\n  name: "run"\n  id: 3\n}\n')
    (tmp_path / "val.csv").write_text(
        "original_vido_id video_id frame_id path labels\n"
        'vidA 0 0 vidA/000001.jpg ""\nvidA 0 1 vidA/000002.jpg ""\nvidB 1 0 vidB/000001.jpg ""\n')


class _Cfg(object):
    def __init__(self, tmp_path, full=False, num_gpus=1):
        d = str(tmp_path)
        self.LOG_PERIOD, self.NUM_GPUS = 2, num_gpus
        self.AVA = type("A", (), {"ANNOTATION_DIR": d, "FRAME_LIST_DIR": d, "EXCLUSION_FILE": "excl.csv",
                                  "LABEL_MAP_FILE": "labels.pbtxt", "GROUNDTRUTH_FILE": "gt.csv",
                                  "TEST_LISTS": ["val.csv"], "TRAIN_LISTS": [], "FULL_TEST_ON_VAL": full})()


def test_annotation_parsing(tmp_path):
    from slowfast.utils import ava_eval_helper as H
    _write_annotations(tmp_path)
    assert H.make_image_key("vidA", "904") == "vidA,0904"
    categories, ids = H.read_labelmap(str(tmp_path / "labels.pbtxt"))
    assert categories == [{"id": 1, "name": "bend"}, {"id": 2, "name": "crawl"}, {"id": 3, "name": "run"}]
    assert ids == {1, 2, 3}
    assert H.read_exclusions(str(tmp_path / "excl.csv")) == {"vidB,0916", "vidA,1000"}
    assert H.read_exclusions(None) == set()
    boxes, labels, scores = H.read_csv(str(tmp_path / "gt.csv"), ids)
    assert labels["vidA,0904"] == [3, 1, 3] and scores["vidA,0904"] == [1.0, 1.0, 1.0]
    assert boxes["vidA,0904"][0] == [0.2, 0.1, 0.6, 0.5]  # y1, x1, y2, x2
    assert H.read_csv(str(tmp_path / "gt.csv"), None, load_score=True)[2]["vidA,0904"] == [7.0, 7.0, 8.0, 8.0]
    assert H.load_video_names(_Cfg(tmp_path), False) == ["vidA", "vidB"]
    # get_ava_eval_data / write_results: the official CSV of host arrays
    dets = H.get_ava_eval_data(np.array([[0.5, 0.25, 0.125]], np.float32), np.array([[0, 1, 2, 3, 4]], np.float32),
                               [[1.2, 904.6]], {1, 3}, video_idx_to_name=["vidA", "vidB"])
    assert dict(dets[0]) == {"vidB,0905": [[2.0, 1.0, 4.0, 3.0]] * 2} and dict(dets[1]) == {"vidB,0905": [1, 3]}
    H.write_results(dets, str(tmp_path / "out.csv"))
    assert (tmp_path / "out.csv").read_text() == ("vidB,0905,1.000,2.000,3.000,4.000,1,0.5000\n"
                                                  "vidB,0905,1.000,2.000,3.000,4.000,3,0.1250\n")


def test_ground_truth_tables_layout(tmp_path):
    from slowfast.utils import ava_eval_helper as H
    _write_annotations(tmp_path)
    _, ids = H.read_labelmap(str(tmp_path / "labels.pbtxt"))
    gt = H.read_csv(str(tmp_path / "gt.csv"), ids)
    t = H.GroundTruthTables(gt, H.read_exclusions(str(tmp_path / "excl.csv")), ids, ["vidA", "vidB"], 4)
    h = t.host
    assert t.image_keys == ["vidA,0904", "vidB,0905", "vidB,0908"] and t.device is None
    assert h["gt_off"].tolist() == [0, 3, 4, 5] and h["gt_off"].dtype == np.int32
    # image 0: grouped by class, CSV order kept inside class 3 (column 2); boxes as x1, y1, x2, y2
    assert h["gt_cls"].tolist() == [0, 2, 2, 0, 1]
    assert h["gt_box"].dtype == np.float64 and h["gt_box"][:3].tolist() == [
        [0.1, 0.2, 0.5, 0.6], [0.1, 0.2, 0.5, 0.6], [0.3, 0.3, 0.9, 0.9]]
    assert h["num_gt"].tolist() == [2, 2, 2, 0]  # vidZ counts (it is ground truth), vidB,0916 does not (excluded)
    assert h["whitelist"].tolist() == [1, 1, 1, 0]
    lut = h["lut"]
    assert lut.shape == (2, 1001) and lut.dtype == np.int32
    assert lut[0, 904] == 0 and lut[1, 905] == 1 and lut[1, 908] == 2 and lut[1, 916] == -2 and lut[0, 1000] == -2
    assert (lut == -1).sum() == lut.size - 5
    with pytest.raises(ValueError, match="class 3"):
        H.GroundTruthTables(gt, set(), ids, ["vidA", "vidB"], 2)


def test_device_ava_meter_ground_truth_choice_and_refusals(tmp_path):
    from slowfast.utils.meters import DeviceAVAMeter, get_ava_mini_groundtruth
    _write_annotations(tmp_path)
    val = DeviceAVAMeter(4, _Cfg(tmp_path), "val")
    assert val.video_idx_to_name == ["vidA", "vidB"] and not val.uses_full_groundtruth
    assert sorted(val.mini_groundtruth[0]) == ["vidA,0904", "vidB,0908", "vidB,0916", "vidZ,0912"]
    assert sorted(get_ava_mini_groundtruth(val.full_groundtruth)[1]) == sorted(val.mini_groundtruth[1])
    assert val.groundtruth_tables(3, None).image_keys == ["vidA,0904", "vidB,0908"]
    assert DeviceAVAMeter(4, _Cfg(tmp_path, full=True), "val").uses_full_groundtruth
    test = DeviceAVAMeter(4, _Cfg(tmp_path), "test", video_idx_to_name=["vidB"])
    assert test.uses_full_groundtruth and test.groundtruth_tables(3, None).image_keys == ["vidB,0905", "vidB,0908"]
    with pytest.raises(ValueError, match="DeviceTrainMeter"):
        DeviceAVAMeter(4, _Cfg(tmp_path), "train")
    with pytest.raises(ValueError, match="unknown mode"):
        DeviceAVAMeter(4, _Cfg(tmp_path), "eval")
    with pytest.raises(ValueError, match="GPU tensors"):
        val.update_stats(torch.zeros(2, 3), torch.zeros(2, 5), torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="no predictions"):
        val.finalize_metrics()
    assert val.log_iter_stats(0, 0) is None
    stats = val.log_iter_stats(0, 1)
    assert stats["_type"] == "val_iter" and stats["cur_epoch"] == "1" and stats["cur_iter"] == "2"
    assert "cur_epoch" not in test.log_iter_stats(0, 1)


def test_evaluate_ava_refuses_host_tensors():
    from slowfast.utils import ava_eval_helper as H
    with pytest.raises(ValueError, match="GPU tensors"):
        H.evaluate_ava(torch.zeros(1, 3), torch.zeros(1, 5), torch.zeros(1, 2), set(), {1}, [],
                       groundtruth=({}, {}, {}), video_idx_to_name=["v"])


# ------------------------------------------------------------------------------------------------ C ABI
def test_ava_entries_refuse_before_any_launch():
    import sfhip
    L = sfhip.lib()
    assert sfhip._SIGNATURES["sf_ava_ws_bytes"] == (ctypes.c_long, [ctypes.c_int] * 3)
    K, C, G = 513, 7, 40
    nblk = 3
    up8 = lambda n: -(-n // 8) * 8  # noqa: E731
    assert L.sf_ava_ws_bytes(K, C, G) == C * nblk * 8 + 2 * up8(K * C * 4) + up8(G * 4) + up8(C * nblk * 4)
    assert L.sf_ava_ws_bytes(K, C, 0) > 0
    for k, c, g in ((0, 7, 1), (5, 0, 1), (5, 7, -1), (2 ** 24, 2, 1), (65535 * 256 + 1, 1, 1), (2 ** 23, 2 ** 8, 1)):
        assert L.sf_ava_ws_bytes(k, c, g) == 0, (k, c, g)
    assert L.sf_ava_ws_bytes(65535 * 256, 1, 1) > 0
    FAKE = 1 << 20  # never dereferenced: every call below is refused before a launch
    vp = ctypes.c_void_p
    match = [vp(FAKE), 5, vp(FAKE), 2, K, C, vp(FAKE), vp(FAKE), vp(FAKE), G, 3, vp(FAKE), 2, 100, vp(FAKE), vp(FAKE),
             vp(FAKE), vp(FAKE), None]

    def rc(name, args, **over):
        a = list(args)
        for i, v in over.items():
            a[int(i[1:])] = v
        return getattr(L, name)(*a)
    for i in (0, 2, 6, 7, 8, 11, 14, 15, 16, 17):
        assert rc("sf_ava_match", match, **{"a%d" % i: None}) == sfhip.SF_EINVAL, i
    for i, v in ((1, 4), (3, 1), (4, 0), (5, 0), (9, -1), (10, -1), (12, 0), (13, 0), (12, 2 ** 30)):
        assert rc("sf_ava_match", match, **{"a%d" % i: v}) == sfhip.SF_EINVAL, (i, v)
    for i, off in ((0, 2), (2, 2), (6, 4), (7, 2), (8, 2), (11, 2), (15, 4)):
        assert rc("sf_ava_match", match, **{"a%d" % i: vp(FAKE + off)}) == sfhip.SF_EALIGN, (i, off)
    ap = [vp(FAKE), C, vp(FAKE), vp(FAKE), K, C, vp(FAKE), vp(FAKE), G, vp(FAKE), vp(FAKE), vp(FAKE), None]
    for i in (0, 2, 3, 6, 7, 9, 10):
        assert rc("sf_ava_ap", ap, **{"a%d" % i: None}) == sfhip.SF_EINVAL, i
    for i, v in ((1, C - 1), (4, 0), (5, 0), (8, -1)):
        assert rc("sf_ava_ap", ap, **{"a%d" % i: v}) == sfhip.SF_EINVAL, (i, v)
    for i, off in ((0, 2), (7, 2), (9, 4), (10, 4), (11, 4)):
        assert rc("sf_ava_ap", ap, **{"a%d" % i: vp(FAKE + off)}) == sfhip.SF_EALIGN, (i, off)
