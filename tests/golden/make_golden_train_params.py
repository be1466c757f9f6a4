#!/usr/bin/env python3
"""Recorded decisions of one TRAINING sample, produced by the REFERENCE's own functions in the order its Kinetics loader
calls them (datasets/kinetics.py:186-189, decoder.py:447-454, kinetics.py:237-245): utils.get_random_sampling_rate
(datasets/utils.py:318-327), decoder.get_start_end_idx with clip_idx -1 (decoder.py:55-83), decoder.temporal_sampling
(:35-52) on a tensor whose frames hold their own number, and utils.spatial_sampling (datasets/utils.py:151-203) on a
float64 frame whose two channels hold each pixel's row and column: bilinear resampling of a ramp is the source
coordinate itself, so the scaled size, the crop offset and the flip are read back from the cropped values.

Build container only; the reference's modules are loaded as make_golden_input.py / make_golden_views.py load them.
The crop / min_scale arithmetic of kinetics.py:146-165 is inline code of `__getitem__`, not a function that could be
called: each case states the (min_scale, crop_size) the loader would pass, worked out by hand, and the CPU test holds
`train_clip_params` to them.  Writes tests/golden/train_clip_params.json: per case the sampling rate, the frame
indices, (new_h, new_w, y, x, flip) and the next draw of either generator (what was consumed)."""
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

# cfg terms (what train_clip_params reads) and, worked out by hand, what kinetics.py:146-165 makes of them
CASES = [
    # full-size step of the default schedule: no short cycle, DEFAULT_S 224 -> min_scale 256 * 224 / 224
    dict(seed=1, total=300, h=256, w=340, num_frames=32, sampling_rate=2, long_rate=0, fps=30, target_fps=30,
         short_cycle_idx=None, default_s=224, factors=[0.5, 0.5 ** 0.5], jitter=[256, 320], train_crop=224, flip=True,
         inv=False, min_scale=256, crop_size=224),
    # short cycle 0: crop round(0.5 * 224) = 112, min_scale round(256 * 112 / 224) = 128
    dict(seed=2, total=300, h=256, w=340, num_frames=8, sampling_rate=2, long_rate=8, fps=30, target_fps=30,
         short_cycle_idx=0, default_s=224, factors=[0.5, 0.5 ** 0.5], jitter=[256, 320], train_crop=224, flip=True,
         inv=False, min_scale=128, crop_size=112),
    # short cycle 1, portrait, 25 fps: crop round(0.7071 * 224) = 158, min_scale round(256 * 158 / 224) = round(180.57)
    dict(seed=3, total=250, h=340, w=256, num_frames=16, sampling_rate=2, long_rate=4, fps=25, target_fps=30,
         short_cycle_idx=1, default_s=224, factors=[0.5, 0.5 ** 0.5], jitter=[256, 320], train_crop=224, flip=True,
         inv=True, min_scale=181, crop_size=158),
    # short cycle index 2 (the full-size iteration of a short cycle) in a long-cycle shape: TRAIN_CROP_SIZE 158 stays,
    # min_scale round(256 * 158 / 224) = 181
    dict(seed=4, total=120, h=240, w=320, num_frames=8, sampling_rate=2, long_rate=8, fps=30, target_fps=30,
         short_cycle_idx=2, default_s=224, factors=[0.5, 0.5 ** 0.5], jitter=[256, 320], train_crop=158, flip=True,
         inv=False, min_scale=181, crop_size=158),
    # DEFAULT_S 0 (no multigrid): min_scale untouched; a video shorter than the span (delta 0); no flip draw
    dict(seed=5, total=20, h=48, w=36, num_frames=8, sampling_rate=8, long_rate=0, fps=30, target_fps=30,
         short_cycle_idx=None, default_s=0, factors=[0.5, 0.5 ** 0.5], jitter=[20, 28], train_crop=16, flip=False,
         inv=False, min_scale=20, crop_size=16),
    # small frames, upscaling, square
    dict(seed=6, total=64, h=24, w=24, num_frames=4, sampling_rate=4, long_rate=6, fps=30, target_fps=30,
         short_cycle_idx=None, default_s=0, factors=[0.5, 0.5 ** 0.5], jitter=[30, 40], train_crop=16, flip=True,
         inv=False, min_scale=30, crop_size=16),
]


def load_reference():
    """(utils, decoder) of the reference, or raises ImportError."""
    import make_golden_input
    import make_golden_views
    utils, _ = make_golden_input.load_reference_input_functions()  # first: it leaves what it imported in sys.modules,
    decoder = make_golden_views.load_reference_decoder()           # the decoder's loader puts sys.modules back
    return utils, decoder


def _read_back(vals, n_src, crop):
    """(scaled extent, offset, reversed) from the ramp values along one axis of the crop: value(i) = s * (o + i + 0.5)
    - 0.5 with s = n_src / n_scaled (two middle samples: the ends may be clamped at the frame's edge)."""
    i = crop // 2
    a, b = float(vals[i]), float(vals[i + 1])
    rev = b < a
    if rev:
        a, b = float(vals[crop - 1 - i]), float(vals[crop - 2 - i])
    s = b - a
    n = n_src / s
    o = (a + 0.5) / s - 0.5 - i
    assert abs(n - round(n)) < 1e-6 and abs(o - round(o)) < 1e-6, (n, o)
    return int(round(n)), int(round(o)), rev


def reference_record(utils, decoder, c):
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    rate = utils.get_random_sampling_rate(c["long_rate"], c["sampling_rate"])
    frames = torch.arange(c["total"], dtype=torch.float32).view(-1, 1, 1, 1)
    start, end = decoder.get_start_end_idx(c["total"], c["num_frames"] * rate * c["fps"] / c["target_fps"], -1, 1)
    idx = decoder.temporal_sampling(frames, start, end, c["num_frames"]).flatten().long().tolist()
    ys = torch.arange(c["h"], dtype=torch.float64).view(1, 1, -1, 1).expand(1, 1, c["h"], c["w"])
    xs = torch.arange(c["w"], dtype=torch.float64).view(1, 1, 1, -1).expand(1, 1, c["h"], c["w"])
    out = utils.spatial_sampling(torch.cat([ys, xs]).contiguous(), spatial_idx=-1, min_scale=c["min_scale"],
                                 max_scale=c["jitter"][1], crop_size=c["crop_size"],
                                 random_horizontal_flip=c["flip"], inverse_uniform_sampling=c["inv"])
    assert tuple(out.shape) == (2, 1, c["crop_size"], c["crop_size"])
    new_h, y, rev_y = _read_back(out[0, 0, :, 0], c["h"], c["crop_size"])
    new_w, x, flip = _read_back(out[1, 0, 0, :], c["w"], c["crop_size"])
    assert not rev_y
    return dict(rate=rate, start=start, indices=idx, new_h=new_h, new_w=new_w, y=y, x=x, flip=flip,
                next_random=random.random(), next_numpy=float(np.random.uniform()))


if __name__ == "__main__":
    utils, decoder = load_reference()
    rec = [dict(c, want=reference_record(utils, decoder, c)) for c in CASES]
    path = os.path.join(HERE, "train_clip_params.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rec) + "\n]\n")  # one case per line
    for r in rec:
        w = r["want"]
        print(r["seed"], w["rate"], w["indices"][:3], "...", (w["new_h"], w["new_w"], w["y"], w["x"], w["flip"]))
    print("train_clip_params %.1f KB" % (os.path.getsize(path) / 1024))
