#!/usr/bin/env python3
"""Golden records for the AVA frame-mAP: the REFERENCE's own PascalDetectionEvaluator (slowfast/utils/ava_evaluation/,
driven the way utils/ava_eval_helper.py:173-246 run_evaluation drives it) over the cases of tests/_ava_cases.py.

Only the ava_evaluation package is imported (ava_eval_helper.py itself needs fvcore), under the three aliases numpy
2.x no longer has (metrics.py:41 np.bool, :95 np.NAN, :101 np.float).  The detections are built as
ava_eval_helper.py:249-285 get_ava_eval_data builds them, restated here because that module cannot be imported.

tests/golden/ava_eval/<case>.json: the inputs (preds, boxes, metadata, ground truth, exclusions, whitelist, video names)
and what the evaluator computed: tp / fp labels per (image, class) in detection order, num_gt per class, AP per class
(null: no ground truth) and the mAP.  Scores are distinct within a class in every recorded case: the order np.argsort
gives equal scores is not part of the record."""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
REF_PKG = "/root/reference/SlowFast/slowfast/utils/ava_evaluation"
RECORDED = ("random257", "earlier_row_wins", "iou_exactly_half", "iou_ulp_below_half", "identical_gt_boxes",
            "invalid_box_dropped", "excluded_image", "image_without_gt", "gt_image_without_detections",
            "class_without_gt", "class_outside_whitelist", "envelope")


def load_reference_evaluator():
    np.float, np.NAN, np.bool = float, np.nan, bool
    spec = importlib.util.spec_from_file_location("ava_evaluation", os.path.join(REF_PKG, "__init__.py"),
                                                  submodule_search_locations=[REF_PKG])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["ava_evaluation"] = pkg
    spec.loader.exec_module(pkg)
    from ava_evaluation import object_detection_evaluation, standard_fields
    return object_detection_evaluation, standard_fields


def run_reference(ode, sf, case):
    from _ava_ref import detections_by_image
    evaluator = ode.PascalDetectionEvaluator(case["categories"])
    tp_fp = {}
    per_image = evaluator._evaluation.per_image_eval
    inner = per_image._compute_tp_fp_for_single_class
    state = {}

    def spy(**kw):  # the labels of one (image, class), as the evaluator itself computes them
        scores, labels = inner(**kw)
        state.setdefault("calls", []).append([bool(v) for v in labels])
        return scores, labels
    per_image._compute_tp_fp_for_single_class = spy
    boxes, labels, _ = case["groundtruth"]
    for key in boxes:
        if key in case["excluded"]:
            continue
        evaluator.add_single_ground_truth_image_info(key, {
            sf.InputDataFields.groundtruth_boxes: np.array(boxes[key], dtype=float),
            sf.InputDataFields.groundtruth_classes: np.array(labels[key], dtype=int),
            sf.InputDataFields.groundtruth_difficult: np.zeros(len(boxes[key]), dtype=bool)})
    dets = detections_by_image(case["preds"], case["boxes"], case["metadata"], case["whitelist"], case["names"])
    for key, rows in dets.items():
        if key in case["excluded"]:
            continue
        state["calls"] = []
        evaluator.add_single_detected_image_info(key, {
            sf.DetectionResultFields.detection_boxes: np.array([r[3] for r in rows], dtype=float),
            sf.DetectionResultFields.detection_classes: np.array([r[1] for r in rows], dtype=int),
            sf.DetectionResultFields.detection_scores: np.array([r[2] for r in rows], dtype=float)})
        # _compute_tp_fp calls it once per class index 0 .. num_class - 1 (class id = index + 1)
        for idx, lab in enumerate(state["calls"]):
            if lab:
                tp_fp["%s|%d" % (key, idx + 1)] = lab
    num_gt = [int(v) for v in evaluator._evaluation.num_gt_instances_per_class]
    metrics = evaluator.evaluate()
    ap = {}
    for cat in case["categories"]:
        v = metrics.get("PascalBoxes_PerformanceByCategory/AP@0.5IOU/" + cat["name"])
        ap[str(cat["id"])] = None if v is None or np.isnan(v) else float(v)
    return {"tp_fp": tp_fp, "num_gt": num_gt, "ap": ap, "map": float(metrics["PascalBoxes_Precision/mAP@0.5IOU"])}


def main():
    from _ava_cases import hand_cases, random_case
    ode, sf = load_reference_evaluator()
    cases = dict(hand_cases(), random257=random_case(257))
    out_dir = os.path.join(HERE, "ava_eval")
    os.makedirs(out_dir, exist_ok=True)
    for name in RECORDED:
        case = cases[name]
        record = {"inputs": {"preds": case["preds"].astype(float).tolist(), "boxes": case["boxes"].astype(float).tolist(),
                             "metadata": case["metadata"].astype(float).tolist(),
                             "groundtruth": [dict(d) for d in case["groundtruth"]],
                             "excluded": sorted(case["excluded"]), "whitelist": sorted(case["whitelist"]),
                             "categories": case["categories"], "names": case["names"]},
                  "expected": run_reference(ode, sf, case)}
        path = os.path.join(out_dir, name + ".json")
        with open(path, "w") as f:
            json.dump(record, f, sort_keys=True)
        print("%-28s %6.1f KB  mAP %.6f" % (name, os.path.getsize(path) / 1024, record["expected"]["map"]))


if __name__ == "__main__":
    main()
