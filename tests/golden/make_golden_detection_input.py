#!/usr/bin/env python3
"""Golden vectors for the detection (AVA) input step, produced by the REFERENCE itself:
`Ava._images_and_boxes_preprocessing` (slowfast/datasets/ava_dataset.py:233-338, the AVA.IMG_PROC_BACKEND "pytorch"
route) on an `Ava` object made with object.__new__ and its attributes set, so that no frame list or annotation file is
read.

Build container only.  transform.py, utils.py and ava_dataset.py are loaded by path under a synthetic package with
inert stand-ins for `cv2` / `torchvision`, as make_golden_input.py does.  Writes tests/golden/detection_input.npz: the
uint8 BGR clips (one per frame size) and, per case, the seed, the reference's float32 output [C, T, H, W], the same
run in float64 (the error bar of the GPU test: the clip is handed over as a tensor whose .float() yields float64,
everything else is the reference's own code), the boxes in float64, the decisions the run took (observed at the
reference's own calls: the size handed to interpolate, the offsets handed to crop_boxes, the flip, the lighting
offsets), and the next draw of numpy's RNG."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
DS = "/root/reference/SlowFast/slowfast/datasets"

MEAN, STD = [0.45, 0.40, 0.50], [0.225, 0.25, 0.2]  # distinct per channel: the BGR-order indexing shows
EIGVAL = [0.225, 0.224, 0.229]
EIGVEC = [[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]]
T = 4
# x1, y1, x2, y2 in [0, 1]: one box across the whole frame (crosses the window on every side), one against each edge,
# one in the middle, and the four corners (at least one of which lies wholly outside any 8 x 8 window)
BOXES01 = [[0.02, 0.04, 0.97, 0.95], [0.0, 0.3, 0.4, 0.6], [0.6, 0.3, 1.0, 0.7], [0.3, 0.0, 0.7, 0.3],
           [0.3, 0.7, 0.6, 1.0], [0.45, 0.45, 0.55, 0.55], [0.0, 0.0, 0.06, 0.07], [0.93, 0.0, 1.0, 0.06],
           [0.0, 0.92, 0.05, 1.0], [0.92, 0.9, 1.0, 1.0]]

CASES = [
    dict(name="train_landscape", split="train", hw=(20, 28), jitter=[10, 14], crop=8, bgr=False, seed=3),
    dict(name="train_portrait_bgr", split="train", hw=(30, 22), jitter=[10, 14], crop=8, bgr=True, seed=4),
    dict(name="train_pca", split="train", hw=(20, 28), jitter=[10, 14], crop=8, bgr=False, seed=7, color=True),
    dict(name="train_noresize", split="train", hw=(20, 28), jitter=[20, 20], crop=8, bgr=False, seed=11),
    dict(name="val_center", split="val", hw=(20, 28), crop=8, bgr=False, seed=5),
    dict(name="val_center_flip", split="val", hw=(20, 28), crop=8, bgr=False, seed=5, force_flip=True),
    dict(name="val_portrait_bgr", split="val", hw=(30, 22), crop=8, bgr=True, seed=6),
    dict(name="test_landscape", split="test", hw=(20, 28), crop=8, bgr=False, seed=8),
    dict(name="test_portrait_flip_bgr", split="test", hw=(30, 22), crop=8, bgr=True, seed=9, force_flip=True),
]


def load_reference():
    """(ava_dataset, transform, utils) of the reference, loaded by path."""
    from make_golden_input import load_reference_input_functions
    utils, transform = load_reference_input_functions()  # registers the package "sfds" and the stand-ins
    mods = {"utils": utils, "transform": transform}
    for name in ("ava_helper", "cv2_transform", "build", "ava_dataset"):
        spec = importlib.util.spec_from_file_location("sfds." + name, os.path.join(DS, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules["sfds." + name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return mods["ava_dataset"], transform, utils


COLLATE = ["train_landscape", "train_pca", "train_noresize", "val_center", "val_center_flip"]  # one window, AVA.BGR False


def load_reference_loader():
    """The reference's datasets/loader.py by path; its multigrid sampler (not used by detection_collate) is a stand-in."""
    import types
    stub = types.ModuleType("slowfast.datasets.multigrid_helper")
    stub.ShortCycleBatchSampler = object
    sys.modules.setdefault("slowfast.datasets.multigrid_helper", stub)
    spec = importlib.util.spec_from_file_location("sfds.loader", os.path.join(DS, "loader.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["sfds.loader"] = m
    spec.loader.exec_module(m)
    return m


def make_dataset(ava_dataset, c):
    """An Ava object with the attributes __init__ sets from the config (ava_dataset.py:23-45), nothing loaded."""
    ds = object.__new__(ava_dataset.Ava)
    ds._split = c["split"]
    ds._data_mean, ds._data_std = MEAN, STD
    ds._use_bgr = c["bgr"]
    ds.random_horizontal_flip = True
    ds._crop_size = c["crop"]
    if c["split"] == "train":
        ds._jitter_min_scale, ds._jitter_max_scale = c["jitter"]
        ds._use_color_augmentation = bool(c.get("color"))
        ds._pca_jitter_only = True
        ds._pca_eigval, ds._pca_eigvec = EIGVAL, EIGVEC
    else:
        ds._test_force_flip = bool(c.get("force_flip"))
    return ds


class _AsFloat64(torch.Tensor):
    """A uint8 clip whose .float() gives float64: the reference's own code then runs in double precision."""

    def float(self):
        return self.as_subclass(torch.Tensor).double()


def clip_of(c):
    """One clip per frame size, shared by the cases of that size (stored once, as clip_<H>x<W>)."""
    h, w = c["hw"]
    return np.random.RandomState(200 + h).randint(0, 256, (T, h, w, 3)).astype(np.uint8)


def reference_record(ava_dataset, transform, c, clip, f64=False):
    """Run the reference on `clip` (uint8 [T, H, W, 3], BGR) -> (imgs [C, T, H, W], boxes float64, decisions)."""
    ds = make_dataset(ava_dataset, c)
    seen = dict(new_hw=list(c["hw"]), y=0, x=0, flip=False, offsets=[0.0, 0.0, 0.0])
    real = dict(interpolate=torch.nn.functional.interpolate, crop_boxes=transform.crop_boxes,
                horizontal_flip=transform.horizontal_flip, lighting_jitter=transform.lighting_jitter)

    def interpolate(images, size=None, **kw):
        seen["new_hw"] = [int(size[0]), int(size[1])]
        return real["interpolate"](images, size=size, **kw)

    def crop_boxes(boxes, x_offset, y_offset):
        seen["y"], seen["x"] = int(y_offset), int(x_offset)
        return real["crop_boxes"](boxes, x_offset, y_offset)

    def horizontal_flip(prob, images, boxes=None):
        out, fb = real["horizontal_flip"](prob, images, boxes=boxes)
        seen["flip"] = not torch.equal(out, images)  # random pixels: a flipped clip differs from itself
        return out, fb

    def lighting_jitter(images, alphastd, eigval, eigvec):
        state = np.random.get_state()  # the offsets as the reference adds them: on a zero float32 image, then rewind
        z = real["lighting_jitter"](torch.zeros(1, 3, 1, 1), alphastd, eigval, eigvec)
        seen["offsets"] = [float(v) for v in z.flatten().tolist()]
        np.random.set_state(state)
        return real["lighting_jitter"](images, alphastd, eigval, eigvec)

    torch.nn.functional.interpolate = interpolate
    transform.crop_boxes, transform.horizontal_flip = crop_boxes, horizontal_flip
    transform.lighting_jitter = lighting_jitter
    try:
        np.random.seed(c["seed"])
        imgs = torch.as_tensor(clip).permute(0, 3, 1, 2)  # T H W C -> T C H W (ava_dataset.py:383-384)
        if f64:
            imgs = imgs.as_subclass(_AsFloat64)
        out, boxes = ds._images_and_boxes_preprocessing(imgs, boxes=np.array(BOXES01, dtype=np.float64))
        seen["next_numpy"] = float(np.random.uniform())
    finally:
        torch.nn.functional.interpolate = real["interpolate"]
        transform.crop_boxes, transform.horizontal_flip = real["crop_boxes"], real["horizontal_flip"]
        transform.lighting_jitter = real["lighting_jitter"]
    out = out.permute(1, 0, 2, 3).contiguous()  # T C H W -> C T H W (:389-390)
    assert out.dtype == (torch.float64 if f64 else torch.float32) and boxes.dtype == np.float64
    return out.numpy(), boxes, seen


def load_imgs64(z, name):
    """The float64 run of case `name` from the loaded file `z`."""
    return z[name + "/imgs"].astype(np.float64) + z[name + "/d64"].astype(np.float64)


if __name__ == "__main__":
    ava_dataset, transform, utils = load_reference()
    out = {"cases": None, "mean": np.array(MEAN, np.float32), "std": np.array(STD, np.float32),
           "eigval": np.array(EIGVAL, np.float64), "eigvec": np.array(EIGVEC, np.float64),
           "boxes01": np.array(BOXES01, np.float64)}
    cases = []
    for c in CASES:
        clip = clip_of(c)
        imgs, boxes, seen = reference_record(ava_dataset, transform, c, clip)
        imgs64, boxes64, seen64 = reference_record(ava_dataset, transform, c, clip, f64=True)
        assert seen == seen64 and np.array_equal(boxes, boxes64) and imgs.shape == imgs64.shape
        out["clip_%dx%d" % tuple(c["hw"])] = clip
        out[c["name"] + "/imgs"] = imgs
        # the float64 run, stored as its difference from the float32 run (a few 1e-6; in float32 that keeps it to
        # 1e-13, half the bytes): imgs64 = imgs + d64, see load_imgs64
        out[c["name"] + "/d64"] = (imgs64 - imgs.astype(np.float64)).astype(np.float32)
        out[c["name"] + "/boxes"] = boxes
        cases.append(dict(c, want=seen))
        err = float(np.abs(imgs.astype(np.float64) - imgs64).max())
        degenerate = int(((boxes[:, 0] == boxes[:, 2]) | (boxes[:, 1] == boxes[:, 3])).sum())
        print("%-24s imgs %s fp32-vs-fp64 %.2e  %s  boxes collapsed onto an edge: %d" % (
            c["name"], imgs.shape, err, {k: v for k, v in seen.items() if k != "next_numpy"}, degenerate))
    # the loader's collation (datasets/loader.py:18-52) of one batch: the cases of COLLATE in that order
    loader = load_reference_loader()
    k = len(BOXES01)
    batch = [([torch.zeros(1)], np.zeros((k, 2), np.int32), i,
              {"boxes": out[n + "/boxes"], "ori_boxes": np.array(BOXES01, np.float64),
               "metadata": [[i + 3, 900 + i]] * k}) for i, n in enumerate(COLLATE)]
    _, _, _, extra = loader.detection_collate(batch)
    for key in ("boxes", "ori_boxes", "metadata"):
        out["collate/" + key] = extra[key].numpy()
    out["collate/cases"] = json.dumps(COLLATE)
    out["cases"] = json.dumps(cases)
    out["seq"] = json.dumps({"%d/%d/%d/%d" % a: utils.get_sequence(*a)
                             for a in ((3, 8, 2, 40), (38, 8, 2, 40), (20, 8, 2, 40), (0, 4, 1, 3), (5, 32, 2, 7))})
    path = os.path.join(HERE, "detection_input.npz")
    np.savez_compressed(path, **out)
    print("detection_input %.1f KB" % (os.path.getsize(path) / 1024))
