#!/usr/bin/env python3
"""The epoch's end of a detection evaluation at a synthetic size of the order of the AVA validation set, against the
numpy restatement of the reference's evaluator (tests/_ava_ref.py) on the same host.

Size: 64 videos x seconds 902 .. 1798 = 57 408 key frames (AVA v2.2 val), 1 .. 4 annotated persons per frame with
1 .. 3 labels each (G about 290 000 rows; the real file has about a quarter of a million), C = 80 classes of which the
60 evaluated ones are whitelisted, K = 150 000 predicted boxes (about 2.6 per frame — the order of the person detector's
boxes above AVA.DETECTION_SCORE_THRESH), four in five of them an annotated person's box moved by a few percent.

  device   `device_frame_map` on tensors already in the meter's stores: sf_ava_match + sf_ava_ap (five launches) and
           the one copy; the median of ROUNDS calls, each between two device synchronisations, host clock
  tables   GroundTruthTables: the host pass over the ground truth and the six uploads, once per meter
  host     tests/_ava_ref.evaluate on the same arrays already on the host, one call (the reference's own evaluator
           does not run on numpy 2: its cost is this loop's plus a per-batch pickled gather)
Clocks not pinned.   usage: tools/microbench/ava_eval_bench.py [out.txt] [--no-host]"""
import os
import statistics
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd"), os.path.join(ROOT, "tests")]
ROUNDS = 5
VIDEOS, SEC0, SEC1, C, K = 64, 902, 1798, 80, 150000


def synthetic_epoch(seed=0):
    rs = np.random.RandomState(seed)
    names = ["video%02d" % v for v in range(VIDEOS)]
    whitelist = set(range(1, 61))
    gb, gl, gs = defaultdict(list), defaultdict(list), defaultdict(list)
    persons = {}
    for v in range(VIDEOS):
        for sec in range(SEC0, SEC1 + 1):
            key = "%s,%04d" % (names[v], sec)
            persons[(v, sec)] = []
            for _ in range(rs.randint(1, 5)):
                x1, y1 = rs.uniform(0.0, 0.6, 2)
                w, h = rs.uniform(0.1, 0.4, 2)
                box = [round(float(t), 3) for t in (x1, y1, x1 + w, y1 + h)]
                persons[(v, sec)].append(box)
                for cls in rs.choice(60, size=rs.randint(1, 4), replace=False) + 1:
                    gb[key].append([box[1], box[0], box[3], box[2]])
                    gl[key].append(int(cls))
                    gs[key].append(1.0)
    excluded = {"%s,%04d" % (names[v], SEC0 + 7 * v) for v in range(VIDEOS)}
    boxes = np.zeros((K, 5), np.float32)
    meta = np.zeros((K, 2), np.float32)
    for i in range(K):
        v, sec = rs.randint(VIDEOS), rs.randint(SEC0, SEC1 + 1)
        if rs.uniform() < 0.8:
            p = persons[(v, sec)]
            box = np.asarray(p[rs.randint(len(p))]) + rs.uniform(-0.03, 0.03, 4)
        else:
            x1, y1 = rs.uniform(0.0, 0.6, 2)
            box = np.asarray([x1, y1, x1 + rs.uniform(0.1, 0.4), y1 + rs.uniform(0.1, 0.4)])
        boxes[i, 1:] = box
        meta[i] = (v, sec)
    preds = rs.uniform(0.0, 1.0, (K, C)).astype(np.float32)
    return preds, boxes, meta, (gb, gl, gs), excluded, whitelist, names


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    import torch
    from slowfast.utils.ava_eval_helper import GroundTruthTables, device_frame_map
    assert torch.cuda.is_available(), "ava_eval_bench needs an MI355X"
    preds, boxes, meta, gt, excluded, whitelist, names = synthetic_epoch()
    t0 = time.perf_counter()
    tables = GroundTruthTables(gt, excluded, whitelist, names, C, device="cuda")
    torch.cuda.synchronize()
    t_tables = time.perf_counter() - t0
    G = int(tables.host["gt_cls"].shape[0])
    lines = ["ava_eval_bench on %s: K = %d rows, C = %d (%d evaluated), G = %d ground-truth rows in %d images" % (
        torch.cuda.get_device_name(0), K, C, len(whitelist), G, len(tables.image_keys))]
    dev = [torch.from_numpy(a).cuda() for a in (preds, boxes, meta)]
    value, ap = device_frame_map(*dev, tables)
    times = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device_frame_map(*dev, tables)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    lines.append("  device_frame_map (5 launches + one copy)   %10.2f ms  (%.2f .. %.2f), mAP %.17g" % (
        statistics.median(times) * 1e3, min(times) * 1e3, max(times) * 1e3, value))
    lines.append("  GroundTruthTables (host pass + uploads)    %10.2f ms, once per meter" % (t_tables * 1e3))
    if "--no-host" not in sys.argv:
        import _ava_ref
        t0 = time.perf_counter()
        want = _ava_ref.evaluate(preds, boxes, meta, gt, excluded, whitelist, names)
        lines.append("  tests/_ava_ref.evaluate on the host        %10.2f ms, mAP %.17g (|d| %.3g, %d true positives)" % (
            (time.perf_counter() - t0) * 1e3, want["map"], abs(want["map"] - value), int(want["tp"].sum())))
    text = "\n".join(lines)
    print(text)
    if args:
        with open(args[0], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
