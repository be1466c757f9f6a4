#!/usr/bin/env python3
"""Golden record for the training meter under DATA.MULTI_LABEL: the REFERENCE's own slowfast/utils/meters.py::TrainMeter
(:426-554), imported as make_golden_train_meter.py does, fed a fixed sequence of per-step losses as the multi-label
route of train_net.py hands them over (top1_err = top5_err = None there: the meter must not touch them).  What it
hands to logging.log_json_stats is captured.  Writes tests/golden/train_meter_multilabel_stats.json: the config
fields, the value sequence and the captured train_iter / train_epoch records (time, memory and ETA fields are
dropped: they depend on the machine) — no top1_err / top5_err anywhere and no loss in the epoch record."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

MACHINE_FIELDS = ("time_diff", "eta", "gpu_mem", "RAM")


def main():
    from make_golden_meter import load_reference_meters
    meters = load_reference_meters()
    import _refimport
    import slowfast.utils.logging as logging
    cases = {}
    for case, (log_period, epoch_iters, max_epoch, steps, num_gpus, mb, seed) in {
            "period4": (4, 10, 3, 10, 1, 8, 11), "period3_world2": (3, 7, 2, 7, 2, 4, 12)}.items():
        rs = np.random.RandomState(seed)
        # a mean BCE over boxes x classes, read back with .item() as float32
        loss = [float(np.float32(v)) for v in rs.uniform(0.02, 0.9, steps)]
        lrs = [0.1 * (0.9 ** i) for i in range(steps)]
        cfg = _refimport._CfgNode({"LOG_PERIOD": log_period, "NUM_GPUS": num_gpus, "SOLVER": {"MAX_EPOCH": max_epoch},
                                   "DATA": {"MULTI_LABEL": True}})
        logged = []
        orig = logging.log_json_stats
        logging.log_json_stats = lambda stats: logged.append(
            {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in stats.items()
             if k not in MACHINE_FIELDS})
        try:
            m = meters.TrainMeter(epoch_iters, cfg)
            m.iter_tic()
            for i in range(steps):
                m.iter_toc()
                m.update_stats(None, None, loss[i], lrs[i], mb * num_gpus)
                m.log_iter_stats(1, i)
                m.iter_tic()
            m.log_epoch_stats(1)
        finally:
            logging.log_json_stats = orig
        cases[case] = dict(log_period=log_period, epoch_iters=epoch_iters, max_epoch=max_epoch, num_gpus=num_gpus,
                           mb_per_gpu=mb, cur_epoch=1, loss=loss, lr=lrs, logged=logged)
    path = os.path.join(HERE, "train_meter_multilabel_stats.json")
    with open(path, "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
    print("train_meter_multilabel_stats %.1f KB" % (os.path.getsize(path) / 1024),
          [len(c["logged"]) for c in cases.values()])


if __name__ == "__main__":
    main()
