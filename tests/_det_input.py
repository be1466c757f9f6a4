"""Shared by the detection input-step tests: the recording tests/golden/detection_input.npz (the reference's own
`Ava._images_and_boxes_preprocessing`, written by tests/golden/make_golden_detection_input.py), the config each
recorded case stands for, and the host decisions replayed from the recorded seed."""
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def recording():
    """(npz, {name: case})  — loaded once, never written to."""
    z = np.load(os.path.join(HERE, "golden", "detection_input.npz"))
    return z, {c["name"]: c for c in json.loads(str(z["cases"]))}


def case_cfg(c, backend="pytorch"):
    from slowfast.config.defaults import get_cfg
    z, _ = recording()
    cfg = get_cfg()
    cfg.AVA.IMG_PROC_BACKEND = backend
    cfg.AVA.BGR = c["bgr"]
    cfg.DATA.MEAN, cfg.DATA.STD = [float(v) for v in z["mean"]], [float(v) for v in z["std"]]
    cfg.DATA.TRAIN_CROP_SIZE = cfg.DATA.TEST_CROP_SIZE = c["crop"]
    if c["split"] == "train":
        cfg.DATA.TRAIN_JITTER_SCALES = list(c["jitter"])
    cfg.AVA.TRAIN_USE_COLOR_AUGMENTATION = bool(c.get("color"))
    cfg.AVA.TRAIN_PCA_JITTER_ONLY = True
    cfg.AVA.TRAIN_PCA_EIGVAL = z["eigval"].tolist()
    cfg.AVA.TRAIN_PCA_EIGVEC = z["eigvec"].tolist()
    cfg.AVA.TEST_FORCE_FLIP = bool(c.get("force_flip"))
    return cfg


def clip_of(c):
    z, _ = recording()
    return z["clip_%dx%d" % tuple(c["hw"])]


@functools.lru_cache(maxsize=None)
def replay(name):
    """(DetParams, boxes float64 [k, 4], the next draw of numpy's RNG) of case `name` from its recorded seed."""
    from slowfast.datasets import utils as ds
    z, cases = recording()
    c = cases[name]
    np.random.seed(c["seed"])
    p = ds.det_clip_params(case_cfg(c), c["split"], c["hw"][0], c["hw"][1])
    nxt = float(np.random.uniform())
    return p, ds.det_boxes(z["boxes01"], c["hw"][0], c["hw"][1], p), nxt


def imgs64(name):
    """The reference's float64 run of case `name`, [C, T, win_h, win_w]."""
    import make_golden_detection_input as gen
    return gen.load_imgs64(recording()[0], name)


def collated():
    """(case names of the recorded batch, the reference's `detection_collate` output for it: boxes float32 [K, 5],
    ori_boxes float32 [K, 5], metadata int64 [K, 2]).  Sample i's metadata rows are [i + 3, 900 + i]."""
    z, _ = recording()
    return json.loads(str(z["collate/cases"])), z["collate/boxes"], z["collate/ori_boxes"], z["collate/metadata"]
