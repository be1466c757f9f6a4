"""Plain-numpy fp64 restatement of the AVA frame-mAP the reference computes (utils/ava_eval_helper.py and the
PascalDetectionEvaluator of utils/ava_evaluation/), following its loops literally; tests/test_ava_eval_cpu.py pins it
against recorded results of the reference's own evaluator, tests/test_ava_eval_gpu.py compares the kernels with it.

The one rule the reference leaves open: np.argsort(scores)[::-1] (metrics.py:60-61) orders equal scores arbitrarily.
Here, among equal scores of a class, the detection of the higher row index stands first."""
from collections import defaultdict

import numpy as np


def detections_by_image(preds, ori_boxes, metadata, class_whitelist, video_idx_to_name):
    """ava_eval_helper.py:249-285 get_ava_eval_data, keeping the row of every detection: {key: [(row, class id, score,
    [y1, x1, y2, x2]), ...]} in row order, keys in order of first appearance."""
    out = defaultdict(list)
    for i in range(preds.shape[0]):
        video_idx = int(np.round(metadata[i][0]))
        sec = int(np.round(metadata[i][1]))
        key = video_idx_to_name[video_idx] + "," + "%04d" % (sec)
        batch_box = [float(v) for v in ori_boxes[i]]
        batch_box = [batch_box[j] for j in [0, 2, 1, 4, 3]]
        for cls_idx in range(preds.shape[1]):
            if cls_idx + 1 in class_whitelist:
                out[key].append((i, cls_idx + 1, float(preds[i][cls_idx]), batch_box[1:]))
    return out


def area(boxes):  # np_box_ops.py:31-40
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def intersection(boxes1, boxes2):  # np_box_ops.py:43-68
    [y_min1, x_min1, y_max1, x_max1] = np.split(boxes1, 4, axis=1)
    [y_min2, x_min2, y_max2, x_max2] = np.split(boxes2, 4, axis=1)
    all_pairs_min_ymax = np.minimum(y_max1, np.transpose(y_max2))
    all_pairs_max_ymin = np.maximum(y_min1, np.transpose(y_min2))
    intersect_heights = np.maximum(np.zeros(all_pairs_max_ymin.shape), all_pairs_min_ymax - all_pairs_max_ymin)
    all_pairs_min_xmax = np.minimum(x_max1, np.transpose(x_max2))
    all_pairs_max_xmin = np.maximum(x_min1, np.transpose(x_min2))
    intersect_widths = np.maximum(np.zeros(all_pairs_max_xmin.shape), all_pairs_min_xmax - all_pairs_max_xmin)
    return intersect_heights * intersect_widths


def iou(boxes1, boxes2):  # np_box_ops.py:71-89
    intersect = intersection(boxes1, boxes2)
    union = np.expand_dims(area(boxes1), axis=1) + np.expand_dims(area(boxes2), axis=0) - intersect
    return intersect / union


def match_single_class(det_boxes, gt_boxes):
    """per_image_evaluation.py:302-345 without difficult / group-of boxes: (tp labels, "taken" flags — detections whose
    best box had IoU >= 0.5 but was claimed by an earlier one)."""
    n = det_boxes.shape[0]
    tp = np.zeros(n, dtype=bool)
    taken = np.zeros(n, dtype=bool)
    if n == 0 or gt_boxes.size == 0:
        return tp, taken
    with np.errstate(invalid="ignore", divide="ignore"):
        overlaps = iou(det_boxes, gt_boxes)
    max_overlap_gt_ids = np.argmax(overlaps, axis=1)
    is_gt_box_detected = np.zeros(overlaps.shape[1], dtype=bool)
    for i in range(n):
        gt_id = max_overlap_gt_ids[i]
        if overlaps[i, gt_id] >= 0.5:
            if not is_gt_box_detected[gt_id]:
                tp[i] = True
                is_gt_box_detected[gt_id] = True
            else:
                taken[i] = True
    return tp, taken


def average_precision(scores, rows, labels, num_gt):
    """metrics.py:60-125 for one class (num_gt > 0): (AP, envelope differs from the raw precision at a true positive).
    Descending score, equal scores by descending row."""
    if scores.size == 0:
        return 0.0, False
    order = np.lexsort((-rows, -scores))
    true_positive_labels = labels.astype(int)[order]
    false_positive_labels = 1 - true_positive_labels
    cum_true_positives = np.cumsum(true_positive_labels)
    cum_false_positives = np.cumsum(false_positive_labels)
    precision = cum_true_positives.astype(float) / (cum_true_positives + cum_false_positives)
    recall = cum_true_positives.astype(float) / num_gt
    raw = precision.copy()
    recall = np.concatenate([[0], recall, [1]])
    precision = np.concatenate([[0], precision, [0]])
    for i in range(len(precision) - 2, -1, -1):
        precision[i] = np.maximum(precision[i], precision[i + 1])
    indices = np.where(recall[1:] != recall[:-1])[0] + 1
    ap = np.sum((recall[indices] - recall[indices - 1]) * precision[indices])
    at_tp = np.nonzero(true_positive_labels)[0]
    return float(ap), bool(np.any(precision[1:-1][at_tp] != raw[at_tp]))


def evaluate(preds, ori_boxes, metadata, groundtruth, excluded_keys, class_whitelist, video_idx_to_name):
    """The whole evaluation.  preds [K, C], ori_boxes [K, 5], metadata [K, 2] numpy arrays; groundtruth: the read_csv
    triple.  Returns a dict: tp uint8 [K, C], valid uint8 [K], num_gt int [C], ap float64 [C] (NaN: class left out),
    map, taken (number of false positives whose best box was claimed), envelope (classes whose envelope differs from the
    raw precision), per_image {(key, class id): (scores, tp labels)} as _compute_tp_fp returns them."""
    preds = np.asarray(preds)
    K, C = preds.shape
    gt_boxes, gt_labels = groundtruth[0], groundtruth[1]
    num_gt = np.zeros(C, dtype=np.int64)
    kept_gt = {}
    for key in gt_boxes:  # run_evaluation:187-212, _update_ground_truth_statistics
        if key in excluded_keys:
            continue
        kept_gt[key] = (np.array(gt_boxes[key], dtype=float).reshape(-1, 4), np.array(gt_labels[key], dtype=int))
        for c in range(C):
            num_gt[c] += int(np.sum(kept_gt[key][1] == c + 1))
    tp = np.zeros((K, C), dtype=np.uint8)
    valid = np.zeros(K, dtype=np.uint8)
    taken_total = 0
    per_image = {}
    per_class = [([], [], []) for _ in range(C)]  # scores, rows, labels
    for key, dets in detections_by_image(preds, ori_boxes, metadata, class_whitelist, video_idx_to_name).items():
        if key in excluded_keys:  # run_evaluation:216-225
            continue
        rows = np.array([d[0] for d in dets], dtype=np.int64)
        classes = np.array([d[1] for d in dets], dtype=int)
        scores = np.array([d[2] for d in dets], dtype=float)
        boxes = np.array([d[3] for d in dets], dtype=float).reshape(-1, 4)
        keep = np.logical_and(boxes[:, 0] < boxes[:, 2], boxes[:, 1] < boxes[:, 3])  # _remove_invalid_boxes
        rows, classes, scores, boxes = rows[keep], classes[keep], scores[keep], boxes[keep]
        valid[rows] = 1
        g_boxes, g_classes = kept_gt.get(key, (np.empty((0, 4), dtype=float), np.array([], dtype=int)))
        for c in range(C):
            sel = classes == c + 1
            if not sel.any():
                continue
            labels, taken = match_single_class(boxes[sel], g_boxes[g_classes == c + 1])
            tp[rows[sel], c] = labels
            taken_total += int(taken.sum())
            per_image[(key, c + 1)] = (scores[sel], labels)
            per_class[c][0].append(scores[sel])
            per_class[c][1].append(rows[sel])
            per_class[c][2].append(labels)
    ap = np.full(C, np.nan, dtype=np.float64)
    envelope = []
    for c in range(C):  # object_detection_evaluation.py:777-801
        if num_gt[c] == 0:
            continue
        if per_class[c][0]:
            s, r, l = (np.concatenate(v) for v in per_class[c])
        else:
            s, r, l = np.array([], dtype=float), np.array([], dtype=np.int64), np.array([], dtype=bool)
        ap[c], differs = average_precision(s, r, l, num_gt[c])
        if differs:
            envelope.append(c)
    counted = ap[~np.isnan(ap)]
    return {"tp": tp, "valid": valid, "num_gt": num_gt, "ap": ap, "taken": taken_total, "envelope": envelope,
            "map": float(np.mean(counted)) if counted.size else float("nan"), "per_image": per_image}
