"""Inputs shared by the AVA evaluation tests and tests/golden/make_golden_ava.py: the seeded random epochs and the
hand-built cases, one rule each.  A case is a dict: preds float32 [K, C], boxes float32 [K, 5] (batch index, x1, y1, x2,
y2), metadata float32 [K, 2] (video index, second), groundtruth (the read_csv triple: boxes [y1, x1, y2, x2] per image
key), excluded (set of keys), whitelist (set of class ids), categories, names (video_idx_to_name)."""
import os
from collections import defaultdict

import numpy as np

NAMES = ["vidA", "vidB", "vidC", "vidD", "vidE"]
WHITELIST = (1, 2, 3, 5, 6)  # of C = 7 columns; class 6 never has ground truth, class 4 / 7 are not evaluated
RANDOM_SEEDS = {255: 11, 257: 12, 513: 13}  # K -> seed (checked on the host: see random_case)


def key_of(video, sec):
    return "%s,%04d" % (video, int(sec))


def _case(preds, boxes, meta, gt_rows, excluded=(), whitelist=WHITELIST, names=NAMES, filter_gt=True):
    """gt_rows: [(video name, second, x1, y1, x2, y2, class id)] in CSV order.  filter_gt: drop the rows of classes
    outside the whitelist, as read_csv does; False keeps them (a triple that was read without the whitelist)."""
    gb, gl, gs = defaultdict(list), defaultdict(list), defaultdict(list)
    for video, sec, x1, y1, x2, y2, cls in gt_rows:
        if filter_gt and cls not in whitelist:
            continue
        k = key_of(video, sec)
        gb[k].append([y1, x1, y2, x2])
        gl[k].append(int(cls))
        gs[k].append(1.0)
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    return {"preds": np.asarray(preds, dtype=np.float32),
            "boxes": np.concatenate([np.zeros((boxes.shape[0], 1), np.float32), boxes], axis=1),
            "metadata": np.asarray(meta, dtype=np.float32).reshape(-1, 2), "groundtruth": (gb, gl, gs),
            "excluded": set(excluded), "whitelist": set(whitelist), "names": list(names),
            "categories": [{"id": c, "name": "action%d" % c} for c in sorted(whitelist)]}


def random_case(K, seed=None, C=7, images=37):
    """K rows over `images` images of 5 videos.  Boxes lie on a grid of 1/8 (exact in float32) and most detections are a
    ground-truth box moved by a few grid steps, so many IoUs reach 0.5 and several rows claim one box; 3 images are
    excluded, 5 have no ground truth, 3 ground-truth images get no detection, a few boxes are invalid; scores are
    distinct within a class; the rows are shuffled, so the rows of an image are not contiguous."""
    rs = np.random.RandomState(RANDOM_SEEDS[K] if seed is None else seed)
    keys = [(NAMES[i % len(NAMES)], 902 + 2 * (i // len(NAMES)) + (i % 3)) for i in range(images + 3)]
    det_images, gt_only = keys[:images], keys[images:]
    excluded = {key_of(*k) for k in det_images[3:6]}
    no_gt = set(det_images[6:11])
    gt_rows, persons = [], {}
    for k in det_images + gt_only:
        if k in no_gt:
            continue
        persons[k] = []
        for _ in range(rs.randint(1, 4)):
            x1, y1 = rs.randint(0, 24, 2) / 8.0
            w, h = rs.randint(4, 17, 2) / 8.0
            persons[k].append((x1, y1, x1 + w, y1 + h))
            for cls in rs.choice([1, 2, 3, 5], size=rs.randint(1, 4), replace=False):
                gt_rows.append((k[0], k[1], x1, y1, x1 + w, y1 + h, int(cls)))
    k = det_images[12]  # two identical ground-truth boxes of one class in one image
    x1, y1, x2, y2 = persons[k][0]
    gt_rows += [(k[0], k[1], x1, y1, x2, y2, 1)] * 2
    boxes, meta = [], []
    for i in range(K):
        k = det_images[rs.randint(len(det_images))]
        if k in persons and rs.uniform() < 0.8:
            x1, y1, x2, y2 = persons[k][rs.randint(len(persons[k]))]
            dx1, dy1, dx2, dy2 = rs.randint(-2, 3, 4) / 8.0
            box = (x1 + dx1, y1 + dy1, x2 + dx2, y2 + dy2)
        else:
            x1, y1 = rs.randint(0, 24, 2) / 8.0
            box = (x1, y1, x1 + rs.randint(4, 17) / 8.0, y1 + rs.randint(4, 17) / 8.0)
        if rs.uniform() < 0.03:
            box = (box[0], box[1], box[0], box[3])  # x1 == x2: dropped
        boxes.append(box)
        meta.append((NAMES.index(k[0]) + rs.uniform(-0.3, 0.3), k[1] + rs.uniform(-0.3, 0.3)))  # rounds to the key
    preds = np.stack([(rs.permutation(K) + 0.5) / K for _ in range(C)], axis=1)
    return _case(preds, boxes, meta, gt_rows, excluded)


def hand_cases():
    """name -> case; every case isolates one rule of the evaluator (the test names say which)."""
    unit, wide = (0, 0, 1, 1), (0, 0, 2, 1)
    below = (0, 0, float(np.nextafter(np.float32(2), np.float32(3))), 1)  # IoU one float32 ulp below 0.5
    A = ("vidA", 902)
    gtA = [A + unit + (1,)]

    def rows(n, video=0, sec=902):
        return [(video, sec)] * n

    def preds(col0, C=7):
        p = np.full((len(col0), C), 0.25, dtype=np.float32)
        p[:, 0] = col0
        return p
    cases = {
        # two detections whose best box is the same one: the EARLIER row is the true positive
        "earlier_row_wins": _case(preds([0.2, 0.9]), [unit, unit], rows(2), gtA),
        "iou_exactly_half": _case(preds([0.9]), [wide], rows(1), gtA),
        "iou_ulp_below_half": _case(preds([0.9]), [below], rows(1), gtA),
        # both detections pick the FIRST of two identical boxes: the second one is a false positive
        "identical_gt_boxes": _case(preds([0.9, 0.8]), [unit, unit], rows(2), gtA * 2),
        "invalid_box_dropped": _case(preds([0.9, 0.8]), [(0, 0, 0, 1), unit], rows(2), gtA),
        "excluded_image": _case(preds([0.9, 0.8]), [unit, unit], [(0, 902), (1, 903)],
                                gtA + [("vidB", 903) + unit + (1,)], excluded={key_of("vidB", 903)}),
        "image_without_gt": _case(preds([0.9, 0.8]), [unit, unit], [(0, 902), (2, 950)], gtA),
        "gt_image_without_detections": _case(preds([0.9]), [unit], rows(1), gtA + [("vidC", 910) + unit + (1,)] * 2),
        # class 2 has detections and no ground truth: left out of the mean; class 1's AP is 1
        "class_without_gt": _case(preds([0.9]), [unit], rows(1), gtA),
        # class 4 is outside the whitelist and its ground-truth box is KEPT (an unfiltered triple): column 3 yields no
        # detection although its box would match — the evaluator counts the class with AP 0, so the mAP is 1/2
        "class_outside_whitelist": _case(preds([0.9]), [unit], rows(1), gtA + [A + unit + (4,)], filter_gt=False),
        # fp, tp, fp, tp, tp by descending score: the envelope at rank 2 is 3/5 where the precision is 1/2
        "envelope": _case(preds([0.9, 0.8, 0.7, 0.6, 0.5]),
                          [(5, 5, 6, 6), unit, (3, 3, 4, 4), (3, 0, 4, 1), (8, 8, 9, 9)], rows(5),
                          gtA + [A + (3, 0, 4, 1) + (1,), A + (8, 8, 9, 9) + (1,)]),
        # equal scores, rows fp fp tp tp (0.7: fp) tp: the higher row stands first, AP = 3/4 (1/2 in ascending row order)
        "tied_scores": _case(preds([0.5, 0.5, 0.5, 0.5, 0.7, 0.5]),
                             [(5, 5, 6, 6), (6, 6, 7, 7), unit, (3, 0, 4, 1), (7, 7, 8, 8), (8, 8, 9, 9)], rows(6),
                             gtA + [A + (3, 0, 4, 1) + (1,), A + (8, 8, 9, 9) + (1,)]),
    }
    return cases


def write_case_files(case, d):
    """The case's annotations as the files DeviceAVAMeter reads: gt.csv, excl.csv, labels.pbtxt in directory d."""
    with open(os.path.join(d, "gt.csv"), "w") as f:
        for key, boxes in case["groundtruth"][0].items():
            for (y1, x1, y2, x2), cls in zip(boxes, case["groundtruth"][1][key]):
                f.write("%s,%r,%r,%r,%r,%d,1\n" % (key, float(x1), float(y1), float(x2), float(y2), cls))
    with open(os.path.join(d, "excl.csv"), "w") as f:
        f.write("".join(k + "\n" for k in sorted(case["excluded"])))
    with open(os.path.join(d, "labels.pbtxt"), "w") as f:
        for c in case["categories"]:
            f.write('item {\n  name: "%s"\n  id: %d\n}\n' % (c["name"], c["id"]))


class MeterCfg(object):
    """The fields of the config DeviceAVAMeter reads, pointing at write_case_files' directory."""

    def __init__(self, d, full, num_gpus=1):
        self.LOG_PERIOD, self.NUM_GPUS = 2, num_gpus
        self.AVA = type("A", (), {"ANNOTATION_DIR": d, "FRAME_LIST_DIR": d, "EXCLUSION_FILE": "excl.csv",
                                  "LABEL_MAP_FILE": "labels.pbtxt", "GROUNDTRUTH_FILE": "gt.csv",
                                  "TEST_LISTS": [], "TRAIN_LISTS": [], "FULL_TEST_ON_VAL": full})()
