#!/usr/bin/env python3
"""Golden records for validation and multi-label evaluation: the REFERENCE's own slowfast/utils/meters.py — get_map
(:690-714, scikit-learn's average_precision_score), the multi-label TestMeter (:216-373) and ValMeter (:557-687) —
imported as make_golden_meter.py does.

tests/golden/map_vectors.npz: for every case of tests/_map_cases.py (inputs are regenerated from the seed, only results
are stored) get_map's value and the per-class average_precision_score (-1 for a class without a positive); one
multi-label TestMeter run, 5 videos x 3 clips in shuffled batches of 4 (a batch splits a video), ensemble "max" and
"sum", with its inputs, final rows, label rows, clip counts and `map`.

tests/golden/val_meter_stats.json: what ValMeter hands to logging.log_json_stats (time, memory and ETA fields dropped:
they depend on the machine) — single-label over two epochs (min_top1_err carries over), multi-label over one."""
import contextlib
import io
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

MACHINE_FIELDS = ("time_diff", "eta", "gpu_mem", "RAM")


def _per_class(preds, labels):
    from sklearn.metrics import average_precision_score
    aps = np.full((preds.shape[1],), -1.0)
    for c in range(preds.shape[1]):
        if labels[:, c].any():
            aps[c] = average_precision_score(labels[:, c], preds[:, c])
    return aps


def _quiet_get_map(meters, preds, labels):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(meters.get_map(preds, labels))


def map_vectors(meters):
    from _map_cases import case_names, make_case
    out = {}
    for name in case_names():
        preds, labels = make_case(name)
        out[name + "/map"] = np.float64(_quiet_get_map(meters, preds, labels))
        out[name + "/ap"] = _per_class(preds, labels)
    # the multi-label TestMeter
    nv, nc, ncls, bs = 5, 3, 7, 4
    rs = np.random.RandomState(77)
    n = nv * nc
    labels_v = (rs.uniform(0.0, 1.0, (nv, ncls)) < 0.4).astype(np.float32)
    labels_v[:, 0] = (1, 0, 1, 0, 1)  # every video has a positive, one class has both kinds for sure
    preds = rs.uniform(0.0, 1.0, (n, ncls)).astype(np.float32)
    ids = rs.permutation(n)
    out["meter/preds"], out["meter/clip_ids"] = preds[ids], ids.astype(np.int64)
    out["meter/labels"] = labels_v[ids // nc]
    meta = dict(num_videos=nv, num_clips=nc, num_cls=ncls, batch=bs)
    import slowfast.utils.logging as logging
    for method in ("max", "sum"):
        m = meters.TestMeter(nv, nc, ncls, (n + bs - 1) // bs, multi_label=True, ensemble_method=method)
        for s in range(0, n, bs):
            m.update_stats(torch.from_numpy(out["meter/preds"][s:s + bs]),
                           torch.from_numpy(out["meter/labels"][s:s + bs]),
                           torch.from_numpy(out["meter/clip_ids"][s:s + bs]))
        logged = []
        orig = logging.log_json_stats
        logging.log_json_stats = lambda stats: logged.append(dict(stats))
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                m.finalize_metrics()
        finally:
            logging.log_json_stats = orig
        out["meter/%s/video_preds" % method] = m.video_preds.numpy()
        out["meter/%s/video_labels" % method] = m.video_labels.numpy()
        out["meter/%s/clip_count" % method] = m.clip_count.numpy()
        out["meter/%s/map" % method] = np.float64(logged[-1]["map"])
    out["meta"] = json.dumps(meta)
    path = os.path.join(HERE, "map_vectors.npz")
    np.savez_compressed(path, **out)
    print("map_vectors %.1f KB, %d cases" % (os.path.getsize(path) / 1024, len(case_names())))


def val_meter_stats(meters):
    import _refimport
    import slowfast.utils.logging as logging
    cases = {}
    logged = []
    orig = logging.log_json_stats
    logging.log_json_stats = lambda stats: logged.append(
        {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in stats.items()
         if k not in MACHINE_FIELDS})
    try:
        # single-label: two epochs through ONE meter, reset in between as train.py does; the second epoch is worse, so
        # its min_top1_err is the first one's
        for case, (log_period, max_iter, max_epoch, num_gpus, mb, seed) in {
                "period3": (3, 7, 4, 1, 8, 21), "period2_world2": (2, 5, 3, 2, 4, 22)}.items():
            rs = np.random.RandomState(seed)
            cfg = _refimport._CfgNode({"LOG_PERIOD": log_period, "NUM_GPUS": num_gpus,
                                       "SOLVER": {"MAX_EPOCH": max_epoch}, "DATA": {"MULTI_LABEL": False}})
            del logged[:]
            m = meters.ValMeter(max_iter, cfg)
            epochs = []
            for cur_epoch, lo in ((1, 0), (2, mb // 2)):
                # what one batch hands the meter: float32 percentages read back with .item() (train_net.py:230-237)
                c1 = rs.randint(lo, mb + 1, max_iter)
                c5 = np.minimum(c1, rs.randint(lo, mb + 1, max_iter))
                top1 = [float(np.float32((1.0 - (mb - c) / mb) * 100.0)) for c in c1]
                top5 = [float(np.float32((1.0 - (mb - c) / mb) * 100.0)) for c in c5]
                m.iter_tic()
                for i in range(max_iter):
                    m.iter_toc()
                    m.update_stats(top1[i], top5[i], mb * num_gpus)
                    m.log_iter_stats(cur_epoch, i)
                    m.iter_tic()
                m.log_epoch_stats(cur_epoch)
                m.reset()
                epochs.append(dict(cur_epoch=cur_epoch, top1=top1, top5=top5))
            cases[case] = dict(log_period=log_period, max_iter=max_iter, max_epoch=max_epoch, num_gpus=num_gpus,
                               mb_per_gpu=mb, multi_label=False, epochs=epochs, logged=list(logged))
        # multi-label: one epoch; the batches are regenerated from the seed by the test
        log_period, max_iter, max_epoch, mb, ncls, seed = 2, 5, 3, 6, 9, 23
        cfg = _refimport._CfgNode({"LOG_PERIOD": log_period, "NUM_GPUS": 1, "SOLVER": {"MAX_EPOCH": max_epoch},
                                   "DATA": {"MULTI_LABEL": True}})
        rs = np.random.RandomState(seed)
        preds = rs.uniform(0.0, 1.0, (max_iter * mb, ncls)).astype(np.float32)
        labels = (rs.uniform(0.0, 1.0, (max_iter * mb, ncls)) < 0.35).astype(np.float32)
        del logged[:]
        m = meters.ValMeter(max_iter, cfg)
        m.iter_tic()
        for i in range(max_iter):
            m.iter_toc()
            m.update_predictions(torch.from_numpy(preds[i * mb:(i + 1) * mb]),
                                 torch.from_numpy(labels[i * mb:(i + 1) * mb]))
            m.log_iter_stats(0, i)
            m.iter_tic()
        with contextlib.redirect_stdout(io.StringIO()):
            m.log_epoch_stats(0)
        cases["multilabel"] = dict(log_period=log_period, max_iter=max_iter, max_epoch=max_epoch, num_gpus=1,
                                   mb_per_gpu=mb, num_cls=ncls, seed=seed, multi_label=True, cur_epoch=0,
                                   logged=list(logged))
    finally:
        logging.log_json_stats = orig
    path = os.path.join(HERE, "val_meter_stats.json")
    with open(path, "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
    print("val_meter_stats %.1f KB" % (os.path.getsize(path) / 1024), [len(c["logged"]) for c in cases.values()])


def main():
    from make_golden_meter import load_reference_meters
    meters = load_reference_meters()
    map_vectors(meters)
    val_meter_stats(meters)


if __name__ == "__main__":
    main()
