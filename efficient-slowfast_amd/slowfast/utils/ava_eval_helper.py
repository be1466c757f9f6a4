"""AVA evaluation (reference utils/ava_eval_helper.py) on the `sf_ava_match` / `sf_ava_ap` kernels.

The reference copies every prediction to the host, builds per-image Python lists and runs the 3 300-line port of the TF
object-detection API over every (image, class) pair.  Here the host parses the annotation files once
(`read_csv`, `read_exclusions`, `read_labelmap` — plain `open`, no fvcore), `GroundTruthTables` lays the ground truth
out as six small device tables, and `evaluate_ava` computes the frame-mAP at IoU 0.5 from device tensors with ONE
device-to-host copy.  The rules (restated in include/sfhip.h, by numpy loops in tests/_ava_ref.py):

* detections: ava_eval_helper.py:249-285 (`get_ava_eval_data`, kept here for host tensors and `write_results`);
* dropped images and boxes: run_evaluation:187-225, per_image_evaluation.py `_remove_invalid_boxes`;
* matching: per_image_evaluation.py:331-345 — detections of an (image, class) in ROW order, not score order;
* IoU: np_box_ops.py in fp64; ground-truth counts: object_detection_evaluation.py `_update_ground_truth_statistics`;
* AP and the mean: metrics.py:60-125, object_detection_evaluation.py:777-815; equal scores: the higher row first."""
import csv
import logging
import os
import time
from collections import defaultdict

import numpy as np
import torch

logger = logging.getLogger(__name__)

MAP_KEY = "PascalBoxes_Precision/mAP@0.5IOU"
CATEGORY_KEY = "PascalBoxes_PerformanceByCategory/AP@0.5IOU/"


def make_image_key(video_id, timestamp):
    """Returns a unique identifier for a video id & timestamp (ava_eval_helper.py:48-50)."""
    return "%s,%04d" % (video_id, int(timestamp))


def read_csv(csv_file, class_whitelist=None, load_score=False):
    """Boxes and class labels of a CSV file in the AVA format (ava_eval_helper.py:53-87): three dicts keyed by image key
    — boxes [y1, x1, y2, x2], integer labels, scores (1.0 unless `load_score`).  Rows of a class outside the whitelist
    are skipped."""
    boxes = defaultdict(list)
    labels = defaultdict(list)
    scores = defaultdict(list)
    with open(csv_file, "r") as f:
        for row in csv.reader(f):
            assert len(row) in [7, 8], "Wrong number of columns: " + str(row)
            image_key = make_image_key(row[0], row[1])
            x1, y1, x2, y2 = [float(n) for n in row[2:6]]
            action_id = int(row[6])
            if class_whitelist and action_id not in class_whitelist:
                continue
            score = 1.0
            if load_score:
                score = float(row[7])
            boxes[image_key].append([y1, x1, y2, x2])
            labels[image_key].append(action_id)
            scores[image_key].append(score)
    return boxes, labels, scores


def read_exclusions(exclusions_file):
    """The set of excluded image keys of a `video-id,timestamp` CSV; empty for None (ava_eval_helper.py:90-105)."""
    excluded = set()
    if exclusions_file:
        with open(exclusions_file, "r") as f:
            for row in csv.reader(f):
                assert len(row) == 2, "Expected only 2 columns, got: " + str(row)
                excluded.add(make_image_key(row[0], row[1]))
    return excluded


def read_labelmap(labelmap_file):
    """(categories [{"id", "name"}], set of class ids) of a .pbtxt label map (ava_eval_helper.py:108-123)."""
    labelmap = []
    class_ids = set()
    name = ""
    with open(labelmap_file, "r") as f:
        for line in f:
            if line.startswith("  name:"):
                name = line.split('"')[1]
            elif line.startswith("  id:") or line.startswith("  label_id:"):
                class_id = int(line.strip().split(" ")[-1])
                labelmap.append({"id": class_id, "name": name})
                class_ids.add(class_id)
    return labelmap, class_ids


def load_video_names(cfg, is_train):
    """`video_idx_to_name` of datasets/ava_helper.py:15-65 load_image_lists: the video names of the frame lists in order
    of first appearance."""
    lists = cfg.AVA.TRAIN_LISTS if is_train else cfg.AVA.TEST_LISTS
    names, seen = [], set()
    for filename in lists:
        with open(os.path.join(cfg.AVA.FRAME_LIST_DIR, filename), "r") as f:
            f.readline()
            for line in f:
                row = line.split()
                assert len(row) == 5  # original_vido_id video_id frame_id path labels
                if row[0] not in seen:
                    seen.add(row[0])
                    names.append(row[0])
    return names


def get_ava_eval_data(scores, boxes, metadata, class_whitelist, verbose=False, video_idx_to_name=None):
    """Host tensors / arrays -> the (boxes, labels, scores) dicts of the official evaluation (ava_eval_helper.py:249-285).
    Every row is walked in Python: this is for `write_results` and small inputs, `evaluate_ava` does not use it."""
    out_scores = defaultdict(list)
    out_labels = defaultdict(list)
    out_boxes = defaultdict(list)
    for i in range(scores.shape[0]):
        video_idx = int(np.round(metadata[i][0]))
        sec = int(np.round(metadata[i][1]))
        key = video_idx_to_name[video_idx] + "," + "%04d" % (sec)
        batch_box = boxes[i].tolist()
        batch_box = [batch_box[j] for j in [0, 2, 1, 4, 3]]  # the first is the batch index
        for cls_idx, score in enumerate(scores[i].tolist()):
            if cls_idx + 1 in class_whitelist:
                out_scores[key].append(score)
                out_labels[key].append(cls_idx + 1)
                out_boxes[key].append(batch_box[1:])
    return out_boxes, out_labels, out_scores


def write_results(detections, filename):
    """The (boxes, labels, scores) dicts in the official CSV format (ava_eval_helper.py:288-302)."""
    start = time.time()
    boxes, labels, scores = detections
    with open(filename, "w") as f:
        for key in boxes.keys():
            for box, label, score in zip(boxes[key], labels[key], scores[key]):
                f.write("%s,%.03f,%.03f,%.03f,%.03f,%d,%.04f\n" % (key, box[1], box[0], box[3], box[2], label, score))
    logger.info("AVA results wrote to %s" % filename)
    logger.info("\ttook %d seconds." % (time.time() - start))


class GroundTruthTables(object):
    """The ground truth of an evaluation as `sf_ava_match` / `sf_ava_ap` read it, built on the host once.

    groundtruth: the (boxes, labels, scores) triple of `read_csv`; excluded_keys: `read_exclusions`; class_whitelist:
    the evaluated class ids (a detection of class id j + 1 is column j of preds); video_idx_to_name: the list metadata's
    video index points into; num_classes: the columns of preds.

    Host arrays (numpy) and, with `device`, their copies: gt_box fp64 [G, 4] (x1, y1, x2, y2), gt_cls int32 [G] (column),
    gt_off int32 [I + 1] — the rows of image m, grouped by ascending class, CSV order kept within a class — lut int32
    [V, S] ((video index, second) -> image id, -1: no ground truth, -2: excluded), whitelist uint8 [C], num_gt int32 [C]
    (rows per class over ALL non-excluded images, object_detection_evaluation.py `_update_ground_truth_statistics`).
    `image_keys[m]` names image m.  An image of a video that `video_idx_to_name` does not list can receive no
    detection: it has no table rows, but it counts in num_gt."""

    def __init__(self, groundtruth, excluded_keys, class_whitelist, video_idx_to_name, num_classes, device=None):
        gt_boxes, gt_labels = groundtruth[0], groundtruth[1]
        C = int(num_classes)
        names = list(video_idx_to_name)
        listed = set(names)
        num_gt = np.zeros((C,), dtype=np.int32)
        rows, cls, off, keys = [], [], [0], []
        per_video = defaultdict(dict)  # name -> {second: image id, or -2}
        max_sec = 0
        for key in excluded_keys:
            video, sec = key.rsplit(",", 1)
            per_video[video][int(sec)] = -2
            max_sec = max(max_sec, int(sec))
        for key in gt_boxes:  # run_evaluation:187-212
            if key in excluded_keys:
                continue
            labels = [int(v) for v in gt_labels[key]]
            for v in labels:
                if not 1 <= v <= C:
                    raise ValueError("GroundTruthTables: {} has a box of class {}, the predictions have {} "
                                     "classes".format(key, v, C))
                num_gt[v - 1] += 1
            video, sec = key.rsplit(",", 1)
            if video not in listed:
                continue
            if int(sec) < 0:
                raise ValueError("GroundTruthTables: negative timestamp in {}".format(key))
            per_video[video][int(sec)] = len(keys)
            max_sec = max(max_sec, int(sec))
            keys.append(key)
            for j in sorted(range(len(labels)), key=lambda j: labels[j]):  # stable: CSV order within a class
                y1, x1, y2, x2 = gt_boxes[key][j]
                rows.append((x1, y1, x2, y2))
                cls.append(labels[j] - 1)
            off.append(len(rows))
        lut = np.full((max(len(names), 1), max_sec + 1), -1, dtype=np.int32)
        for v, name in enumerate(names):
            for sec, m in per_video.get(name, {}).items():
                if sec >= 0:
                    lut[v, sec] = m
        whitelist = np.zeros((C,), dtype=np.uint8)
        for v in class_whitelist:
            if 1 <= int(v) <= C:
                whitelist[int(v) - 1] = 1
        self.image_keys = keys
        self.num_classes = C
        self.host = {"gt_box": np.asarray(rows, dtype=np.float64).reshape(-1, 4), "gt_cls": np.asarray(cls, np.int32),
                     "gt_off": np.asarray(off, np.int32), "lut": lut, "whitelist": whitelist, "num_gt": num_gt}
        self.device = None
        if device is not None:
            self.to(device)

    def to(self, device):
        """Upload the tables (six copies, once)."""
        self.device = torch.device(device)
        for k, v in self.host.items():
            setattr(self, k, torch.from_numpy(v).to(self.device))
        return self


def device_frame_map(preds, ori_boxes, metadata, tables, who="evaluate_ava"):
    """(mAP, per-class AP float64 [C] with -1 for a class left out) of device tensors against `tables`: five launches and
    ONE device-to-host copy.  ValueError for a NaN or infinite score of an evaluated detection or a video index outside
    `video_idx_to_name`."""
    import sfhip
    if tables.device is None:
        tables.to(preds.device)
    out = sfhip.ava_frame_map(preds.detach().float(), ori_boxes.detach().float(), metadata.detach().float(), tables)
    host = out.cpu().numpy()  # the one device-to-host copy
    if host[2] != 0 or host[3] != 0:
        raise ValueError("{}: {} NaN or infinite score(s), {} row(s) with a video index outside [0, {})".format(
            who, int(host[2]), int(host[3]), tables.host["lut"].shape[0]))
    return float(host[0]), host[4:].copy()


def evaluate_ava(preds, original_boxes, metadata, excluded_keys, class_whitelist, categories, groundtruth=None,
                 video_idx_to_name=None, name="latest"):
    """The reference's entry point (ava_eval_helper.py:136-170) for device tensors: preds [K, C], original_boxes [K, 5],
    metadata [K, 2] (a tensor, not its .tolist()); returns the mAP at IoU 0.5.  `groundtruth` may be a
    `GroundTruthTables` (built once, as DeviceAVAMeter does) or the `read_csv` triple.  The reference also dumps
    detections_<name>.csv / groundtruth_<name>.csv, which needs every prediction on the host: call
    `write_results(get_ava_eval_data(...))` for that.  There is no host fallback: the tensors must be on the GPU."""
    eval_start = time.time()
    if not (torch.is_tensor(preds) and preds.is_cuda):
        raise ValueError("evaluate_ava: preds, original_boxes and metadata are GPU tensors (the evaluation runs on the "
                         "sf_ava_match / sf_ava_ap kernels; there is no host route)")
    tables = groundtruth
    if not isinstance(tables, GroundTruthTables):
        tables = GroundTruthTables(groundtruth, excluded_keys, class_whitelist, video_idx_to_name, preds.shape[1],
                                   device=preds.device)
    logger.info("Evaluating with %d unique GT frames." % len(tables.image_keys))
    mean_ap, _ = device_frame_map(preds, original_boxes, metadata, tables)
    logger.info("AVA eval done in %f seconds." % (time.time() - eval_start))
    return mean_ap


def per_category_results(categories, mean_ap, ap):
    """The metrics dict PascalDetectionEvaluator.evaluate returns (object_detection_evaluation.py:250-290): the mAP and
    one entry per category with ground truth."""
    results = {MAP_KEY: mean_ap}
    for cat in categories:
        j = int(cat["id"]) - 1
        if 0 <= j < len(ap) and ap[j] >= 0:
            results[CATEGORY_KEY + cat["name"]] = float(ap[j])
    return results
