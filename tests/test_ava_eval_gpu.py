"""sf_ava_match / sf_ava_ap (csrc/ava_eval.hip) on the GPU, and evaluate_ava / DeviceAVAMeter on top of them, against the
numpy restatement of the reference's evaluator (tests/_ava_ref.py, itself pinned to the reference's recorded results by
tests/test_ava_eval_cpu.py).

tp / valid flags and counts are compared exactly.  AP and mAP at |d| <= 1e-12: both sides divide the same integers
(one rounding per precision), the restatement multiplies by a recall step k/n - (k-1)/n where the kernel divides the
sum by n — at most n <= 600 terms of a few 2^-53 each, about 1e-13."""
import json
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _ava_cases as cases
import _ava_ref as ref
from _host_reads import count_host_reads as _count_host_reads

pytestmark = pytest.mark.gpu
AP_TOL = 1e-12
_REF = {}


def _expected(name, case):
    """The restatement's result of a case, computed once per module."""
    if name not in _REF:
        _REF[name] = ref.evaluate(case["preds"], case["boxes"], case["metadata"], case["groundtruth"],
                                  case["excluded"], case["whitelist"], case["names"])
    return _REF[name]


def _tables(case):
    from slowfast.utils.ava_eval_helper import GroundTruthTables
    return GroundTruthTables(case["groundtruth"], case["excluded"], case["whitelist"], case["names"],
                             case["preds"].shape[1], device="cuda")


def _run(case):
    """(out fp64 [4 + C], tp, valid) as numpy, from one ava_frame_map call."""
    import sfhip
    out, tp, valid = sfhip.ava_frame_map(*(torch.from_numpy(case[k]).cuda() for k in ("preds", "boxes", "metadata")),
                                         _tables(case), flags=True)
    return out.cpu().numpy(), tp.cpu().numpy(), valid.cpu().numpy()


def _compare(name, case):
    want = _expected(name, case)
    out, tp, valid = _run(case)
    assert np.array_equal(valid, want["valid"])
    assert np.array_equal(tp, want["tp"])
    assert out[2] == 0 and out[3] == 0
    counted = ~np.isnan(want["ap"])
    assert out[1] == counted.sum()
    ap = out[4:]
    assert (ap[~counted] == -1).all()
    print(name, "max |dAP| %.3g" % (np.abs(ap[counted] - want["ap"][counted]).max() if counted.any() else 0.0),
          "|dmAP| %.3g" % abs(out[0] - want["map"]))
    assert np.abs(ap[counted] - want["ap"][counted]).max() <= AP_TOL
    assert abs(out[0] - want["map"]) <= AP_TOL
    return want, out, tp, valid


HAND = cases.hand_cases()


def test_two_detections_of_one_box_the_earlier_row_is_the_true_positive():
    _, _, tp, _ = _compare("earlier_row_wins", HAND["earlier_row_wins"])
    assert tp[:, 0].tolist() == [1, 0]  # the later row scores higher and is still the false positive


def test_iou_exactly_half_is_a_true_positive():
    _, _, tp, _ = _compare("iou_exactly_half", HAND["iou_exactly_half"])
    assert tp[0, 0] == 1


def test_iou_one_float32_ulp_below_half_is_a_false_positive():
    _, _, tp, _ = _compare("iou_ulp_below_half", HAND["iou_ulp_below_half"])
    assert tp[0, 0] == 0


def test_identical_ground_truth_boxes_both_detections_pick_the_first():
    _, out, tp, _ = _compare("identical_gt_boxes", HAND["identical_gt_boxes"])
    assert tp[:, 0].tolist() == [1, 0] and out[0] == 0.5  # the second box stays undetected: recall stops at 1/2


def test_invalid_box_is_dropped():
    _, _, _, valid = _compare("invalid_box_dropped", HAND["invalid_box_dropped"])
    assert valid.tolist() == [0, 1]


def test_excluded_image_is_dropped_from_both_sides():
    _, out, _, valid = _compare("excluded_image", HAND["excluded_image"])
    assert valid.tolist() == [1, 0] and out[0] == 1.0  # its ground-truth box does not count either


def test_image_absent_from_the_ground_truth_gives_false_positives():
    _, _, tp, valid = _compare("image_without_gt", HAND["image_without_gt"])
    assert valid.tolist() == [1, 1] and tp[1].sum() == 0


def test_ground_truth_image_without_detections_counts_in_num_gt():
    _, out, _, _ = _compare("gt_image_without_detections", HAND["gt_image_without_detections"])
    assert abs(out[0] - 1.0 / 3.0) <= 1e-15


def test_class_without_ground_truth_is_left_out_of_the_mean():
    _, out, _, _ = _compare("class_without_gt", HAND["class_without_gt"])
    assert out[1] == 1 and out[0] == 1.0 and out[4 + 1] == -1


def test_class_outside_the_whitelist_is_ignored():
    """Class 4 has a ground-truth box the detection's box matches, and column 3 is not whitelisted: no detection of
    it exists, so it is no true positive, and the class counts in the mean with AP 0 (as the evaluator counts it)."""
    case = HAND["class_outside_whitelist"]
    assert _tables(case).host["num_gt"].tolist()[:4] == [1, 0, 0, 1] and case["groundtruth"][1]["vidA,0902"] == [1, 4]
    _, out, tp, _ = _compare("class_outside_whitelist", case)
    assert tp[0].tolist() == [1, 0, 0, 0, 0, 0, 0] and out[4 + 3] == 0.0 and out[4] == 1.0 and out[1] == 2
    assert out[0] == 0.5


def test_envelope_differs_from_raw_precision():
    want, out, _, _ = _compare("envelope", HAND["envelope"])
    assert want["envelope"] == [0] and abs(out[0] - 0.6) <= 1e-15  # 1/2 + 3/5 + 3/5 over 3 would be the raw sum


def test_equal_scores_the_higher_row_stands_first():
    _, out, _, _ = _compare("tied_scores", HAND["tied_scores"])
    assert out[0] == 0.75


@pytest.mark.parametrize("K", sorted(cases.RANDOM_SEEDS))
def test_random_epoch_matches_the_restatement(K):
    case = cases.random_case(K)
    want = _expected("random%d" % K, case)
    assert int(want["tp"].sum()) >= 20 and want["taken"] >= 20 and len(want["envelope"]) >= 1
    _compare("random%d" % K, case)


def test_strided_views_and_run_to_run_bits():
    """Row views of wider buffers (NaN padding that must never be read), and the same bits twice."""
    import sfhip
    case = cases.random_case(257)
    views = []
    for k in ("preds", "boxes", "metadata"):
        a = case[k]
        whole = torch.full((a.shape[0], a.shape[1] + 3), float("nan"), device="cuda")
        whole[:, :a.shape[1]] = torch.from_numpy(a).cuda()
        views.append(whole[:, :a.shape[1]])
    t = _tables(case)
    first = sfhip.ava_frame_map(*views, t).cpu().numpy()
    again = sfhip.ava_frame_map(*views, t).cpu().numpy()
    dense = _run(case)[0]
    assert first.tobytes() == again.tobytes() == dense.tobytes()


def test_bad_video_index_and_nan_score_are_counted():
    import sfhip
    case = cases.random_case(255)
    t = _tables(case)
    dev = [torch.from_numpy(case[k]).cuda() for k in ("preds", "boxes", "metadata")]
    valid_rows = [r for r in np.flatnonzero(_expected("random255", case)["valid"]) if r not in (5, 9)]
    dev[0][int(valid_rows[0]), 0] = float("nan")
    dev[0][int(valid_rows[1]), 2] = float("inf")
    dev[0][int(valid_rows[2]), 3] = float("nan")  # column 3 is not evaluated: not counted
    dev[2][5, 0] = 17.0
    dev[2][9, 0] = float("nan")
    out, _, valid = sfhip.ava_frame_map(*dev, t, flags=True)
    out, valid = out.cpu().numpy(), valid.cpu().numpy()
    assert out[2] == 2 and out[3] == 2 and valid[5] == 2 and valid[9] == 2


# ------------------------------------------------------------------------------------------------ the meter
BATCHES = (0, 40, 41, 130, 131, 257)  # uneven, one of a single row


def test_meter_epoch_one_host_copy_reset_and_mini_ground_truth(tmp_path):
    from slowfast.utils.meters import DeviceAVAMeter, get_ava_mini_groundtruth
    case = cases.random_case(257)
    cases.write_case_files(case, str(tmp_path))
    want = _expected("random257", case)
    m = DeviceAVAMeter(3, cases.MeterCfg(str(tmp_path), True), "val", video_idx_to_name=case["names"])
    dev = [torch.from_numpy(case[k]).cuda() for k in ("preds", "boxes", "metadata")]
    dev[2] = dev[2].round().long()  # the loader's metadata is integer
    m.groundtruth_tables(7, "cuda")  # built at the first epoch's end otherwise: not part of the count
    with _count_host_reads() as seen:
        for lo, hi in zip(BATCHES[:-1], BATCHES[1:]):
            m.iter_tic()
            m.update_stats(dev[0][lo:hi], dev[1][lo:hi], dev[2][lo:hi])
            m.iter_toc()
        assert seen == []
        value = m.finalize_metrics()
    assert len(seen) == 1, seen
    assert m.rows == 257 and m.cap >= 257
    assert abs(value - want["map"]) <= AP_TOL and m.full_map == value
    names = {c["id"]: c["name"] for c in case["categories"]}
    assert set(m.per_class_ap) == {names[c + 1] for c in np.flatnonzero(~np.isnan(want["ap"]))}
    for c in np.flatnonzero(~np.isnan(want["ap"])):
        assert abs(m.per_class_ap[names[c + 1]] - want["ap"][c]) <= AP_TOL
    # reset empties the store: the next epoch sees only its own rows
    m.reset()
    assert m.rows == 0
    m.update_stats(dev[0][:100], dev[1][:100], dev[2][:100])
    sub = {k: case[k][:100] for k in ("preds", "boxes", "metadata")}
    want100 = ref.evaluate(sub["preds"], sub["boxes"], sub["metadata"], case["groundtruth"], case["excluded"],
                           case["whitelist"], case["names"])
    assert abs(m.log_epoch_stats(0)["map"] - want100["map"]) <= AP_TOL
    # val mode without FULL_TEST_ON_VAL: the mini ground truth (second % 4 == 0)
    mini = DeviceAVAMeter(3, cases.MeterCfg(str(tmp_path), False), "val", video_idx_to_name=case["names"])
    mini.update_stats(*dev)
    want_mini = ref.evaluate(case["preds"], case["boxes"], case["metadata"],
                             get_ava_mini_groundtruth(case["groundtruth"]), case["excluded"], case["whitelist"],
                             case["names"])
    assert want_mini["map"] != want["map"]
    assert abs(mini.finalize_metrics(log=False) - want_mini["map"]) <= AP_TOL


def test_rows_of_one_image_split_across_two_updates(tmp_path):
    """Image A's rows arrive in two update_stats calls with image B's row between them: the meter's stores keep the
    order of arrival, so A's earlier row still wins over its later, higher-scoring one."""
    import sfhip
    from slowfast.utils.ava_eval_helper import evaluate_ava
    from slowfast.utils.meters import DeviceAVAMeter
    unit = (0, 0, 1, 1)
    gt = [("vidA", 902) + unit + (1,), ("vidB", 903) + unit + (1,)]
    case = cases._case(np.array([[0.2] + [0.1] * 6, [0.5] + [0.1] * 6, [0.9] + [0.1] * 6], np.float32),
                       [unit, unit, unit], [(0, 902), (1, 903), (0, 902)], gt)
    want = _expected("split_rows", case)
    # class 1 by descending score: A1 fp, B tp, A0 tp -> envelope 2/3 at both true positives, two ground-truth boxes
    assert want["tp"][:, 0].tolist() == [1, 1, 0] and abs(want["map"] - 2.0 / 3.0) <= 1e-15
    cases.write_case_files(case, str(tmp_path))
    m = DeviceAVAMeter(2, cases.MeterCfg(str(tmp_path), True), "test", video_idx_to_name=case["names"])
    dev = [torch.from_numpy(case[k]).cuda() for k in ("preds", "boxes", "metadata")]
    m.update_stats(*(t[:2] for t in dev))  # A0, B
    m.update_stats(*(t[2:] for t in dev))  # A1
    assert m.rows == 3
    stored = [t[:m.rows] for t in (m.all_preds, m.all_ori_boxes, m.all_metadata)]
    for have, sent in zip(stored, dev):
        assert torch.equal(have, sent)
    out, tp, valid = sfhip.ava_frame_map(*stored, m.groundtruth_tables(7, "cuda"), flags=True)
    assert tp.cpu().numpy()[:, 0].tolist() == [1, 1, 0] and valid.cpu().tolist() == [1, 1, 1]
    assert np.array_equal(tp.cpu().numpy(), want["tp"])
    value = m.finalize_metrics(log=False)
    assert abs(value - want["map"]) <= AP_TOL and value == float(out[0])
    # the same rows through the reference's entry point
    assert evaluate_ava(*dev, case["excluded"], case["whitelist"], case["categories"], groundtruth=case["groundtruth"],
                        video_idx_to_name=case["names"]) == value


def test_nan_score_raises(tmp_path):
    from slowfast.utils.meters import DeviceAVAMeter
    case = cases.random_case(255)
    cases.write_case_files(case, str(tmp_path))
    m = DeviceAVAMeter(1, cases.MeterCfg(str(tmp_path), True), "test", video_idx_to_name=case["names"])
    dev = [torch.from_numpy(case[k]).cuda() for k in ("preds", "boxes", "metadata")]
    dev[0][int(np.flatnonzero(_expected("random255", case)["valid"])[0]), 1] = float("nan")
    m.update_stats(*dev)
    with pytest.raises(ValueError, match="NaN or infinite"):
        m.finalize_metrics()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_meter_epoch_over_two_ranks():
    """A process per rank on a GPU of its own: uneven row counts, all_gather once per store, every rank reports the mAP
    of all rows."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import _ava_worker as w
    world, out, port = 2, tempfile.mkdtemp(), str(_free_port())
    here = os.path.dirname(os.path.abspath(__file__))
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, os.path.join(here, "_ava_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o.decode(errors="replace")[-3000:])
    assert all(p.returncode == 0 for p in procs), logs
    case = w.epoch_case(world)
    want = _expected("two_ranks", case)
    for r in range(world):
        with open(os.path.join(out, "ava_rank%d.json" % r)) as f:
            got = json.load(f)
        assert abs(got["map"] - want["map"]) <= AP_TOL and got["rows"] == w.rank_rows(world, r)[1] - w.rank_rows(
            world, r)[0]
        assert got["host_reads"] == 2  # the ranks' row counts (a shape) and the result
