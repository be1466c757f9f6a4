#!/usr/bin/env python3
"""Golden vectors for Jester's colour jitter, produced by the REFERENCE's own code: transform.RandomColorJitter
(datasets/transform.py:692-717, PIL's ImageEnhance.Brightness / Contrast / Color) on small uint8 clips, that output
carried through the rest of the Jester sample (datasets/jester.py:232-250: utils.tensor_normalize, utils.spatial_sampling
with seeded numpy, utils.pack_pathway_output), and the draws of decoder.decode(..., jester=True) on Python's `random`.

Build container only (it needs the reference tree and Pillow; the recorded run used Pillow 12.2.0).  transform.py,
datasets/utils.py and decoder.py are loaded as make_golden_train_params.py loads them.  torchvision is not installed:
`torchvision.transforms` gets two inert stand-ins that do what RandomColorJitter uses the originals for on uint8 RGB
frames — ToPILImage: Image.fromarray of the HWC bytes of a CHW uint8 tensor; ToTensor: the float32 CHW tensor / 255.

decode() cannot be called without a video container, and its jitter draws are inline code, not a function.  The draws
are therefore taken by the reference's functions where there are functions and by these lines of decoder.py:447-460
restated here where there are none, in decode()'s order:
    start_idx, end_idx = get_start_end_idx(frames.shape[0], num_frames * sampling_rate * fps / target_fps, -1, 1)
    frames = temporal_sampling(frames, start_idx, end_idx, num_frames)
    bright = random.uniform(0.4, 1.4)
    contrast = random.uniform(0.4, 1.4)
    color = random.uniform(0.4, 1.4)
preceded by utils.get_random_sampling_rate (datasets/jester.py:186-189) and followed by the numpy draws of
spatial_sampling, which these records leave to train_clip_params' own golden.

Writes tests/golden/jester_jitter.npz: per frame case the uint8 clip, the factors and the jittered uint8 clip; per
pipeline case the uint8 clip, the factors, the numpy seed and the reference's [slow, fast]; per draw case the sampling rate, the window
start, the three factors and the next random.random()."""
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

MEAN, STD = [0.45, 0.40, 0.50], [0.225, 0.25, 0.2]

# frames only: name, (T, H, W), (bright, contrast, color), how the clip is filled
FRAME_CASES = [
    dict(name="below_one", thw=(2, 9, 13), factors=(0.4, 0.55, 0.7), fill="random"),
    dict(name="above_one", thw=(2, 9, 13), factors=(1.4, 1.3, 1.25), fill="random"),
    dict(name="one_exactly", thw=(2, 7, 5), factors=(1.0, 0.8, 1.2), fill="random"),
    dict(name="drawn", thw=(3, 12, 10), factors=None, fill="random"),         # random.uniform(0.4, 1.4), seed 7
    dict(name="no_bright", thw=(2, 6, 8), factors=(0.0, 1.3, 0.6), fill="random"),
    dict(name="no_contrast", thw=(2, 6, 8), factors=(1.3, 0.0, 0.6), fill="random"),
    dict(name="no_color", thw=(2, 6, 8), factors=(0.6, 1.3, 0.0), fill="random"),
    dict(name="none", thw=(1, 4, 4), factors=(0.0, -1.0, 0.0), fill="random"),
    dict(name="one_pixel", thw=(3, 1, 1), factors=(1.2, 0.7, 1.4), fill="random"),
    dict(name="saturated", thw=(1, 5, 6), factors=(1.4, 1.4, 1.4), fill="white"),
    dict(name="mean_half_up", thw=(1, 4, 6), factors=(1.0, 0.5, 1.0), fill="half"),    # grey mean k + 1/2 exactly
    dict(name="mean_below_half", thw=(1, 5, 5), factors=(1.0, 0.5, 1.0), fill="under"),  # one pixel short of it
]
# the whole sample: thw, factors, spatial_sampling's arguments, alpha, reverse, numpy seed
PIPE_CASES = [
    dict(name="pipe_down", thw=(8, 20, 26), factors=(0.62, 1.31, 0.87), min_scale=10, max_scale=14, crop=8,
         flip=True, inv=False, alpha=4, reverse=False, seed=3),
    dict(name="pipe_up_reverse", thw=(4, 10, 14), factors=(1.37, 0.48, 1.12), min_scale=18, max_scale=24, crop=12,
         flip=True, inv=False, alpha=2, reverse=True, seed=1),
]
# decode()'s draws: what train_clip_params' golden lists, and the jitter behind it
DRAW_CASES = [
    dict(seed=11, total=37, h=100, w=176, num_frames=8, sampling_rate=2, long_rate=0, fps=12, target_fps=12),
    dict(seed=12, total=300, h=256, w=340, num_frames=8, sampling_rate=2, long_rate=8, fps=30, target_fps=30),
    dict(seed=13, total=20, h=100, w=150, num_frames=16, sampling_rate=4, long_rate=6, fps=25, target_fps=30),
]


def load_reference():
    """(utils, transform, decoder) of the reference, with the two torchvision.transforms stand-ins in place."""
    import make_golden_input
    import make_golden_views
    from PIL import Image
    utils, transform = make_golden_input.load_reference_input_functions()
    decoder = make_golden_views.load_reference_decoder()
    transform.transforms.ToPILImage = lambda: (lambda img: Image.fromarray(img.permute(1, 2, 0).contiguous().numpy()))
    transform.transforms.ToTensor = lambda: (lambda img: torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1)
                                             .float().div(255))
    return utils, transform, decoder


def fill_clip(c):
    t, h, w = c["thw"]
    if c["fill"] == "white":
        return np.full((t, h, w, 3), 255, np.uint8)
    if c["fill"] in ("half", "under"):  # grey values k and k + 1 on equal R = G = B pixels
        flat = np.full(t * h * w, 100, np.uint8)
        flat[:(h * w) // 2] = 101
        assert (h * w) % 2 == (1 if c["fill"] == "under" else 0)  # 12 of 24 pixels: 100.5; 12 of 25: 100.48
        return np.repeat(flat.reshape(t, h, w, 1), 3, axis=3)
    return np.random.RandomState(sum(c["thw"]) + len(c["name"])).randint(0, 256, (t, h, w, 3)).astype(np.uint8)


def reference_jitter(transform, clip, factors):
    """decoder.py:461-469 on a uint8 THWC clip -> float32 THWC in [0, 1] (what tensor_normalize then receives)."""
    frames = torch.from_numpy(clip).permute(0, 3, 1, 2)
    frames = transform.RandomColorJitter(bright=factors[0], contrast=factors[1], color=factors[2])(frames)
    frames = torch.as_tensor(np.stack([f.numpy() for f in frames]))
    return frames.permute(0, 2, 3, 1)


def as_bytes(frames01):
    u = (frames01 * 255.0).round()
    assert torch.equal(u / 255.0, frames01)  # ToTensor's division loses nothing: the bytes are recovered exactly
    return u.to(torch.uint8).numpy()


if __name__ == "__main__":
    import PIL
    import make_golden_input
    utils, transform, decoder = load_reference()
    out = {"mean": np.array(MEAN, np.float32), "std": np.array(STD, np.float32), "pillow": PIL.__version__}
    for c in FRAME_CASES + PIPE_CASES:
        if c["factors"] is None:
            random.seed(7)
            c["factors"] = (random.uniform(0.4, 1.4), random.uniform(0.4, 1.4), random.uniform(0.4, 1.4))
        clip = fill_clip(dict(c, fill=c.get("fill", "random")))
        frames = reference_jitter(transform, clip, c["factors"])
        out[c["name"] + "/clip"] = clip
        if "crop" not in c:
            out[c["name"] + "/jittered"] = as_bytes(frames)
        else:
            np.random.seed(c["seed"])
            x = utils.tensor_normalize(frames, MEAN, STD).permute(3, 0, 1, 2)
            x = utils.spatial_sampling(x, spatial_idx=-1, min_scale=c["min_scale"], max_scale=c["max_scale"],
                                       crop_size=c["crop"], random_horizontal_flip=c["flip"],
                                       inverse_uniform_sampling=c["inv"])
            slow, fast = utils.pack_pathway_output(make_golden_input.cfg_like(c["alpha"], c["reverse"]), x)
            out[c["name"] + "/slow"] = slow.contiguous().numpy()
            out[c["name"] + "/fast"] = fast.contiguous().numpy()
        print("%-18s %s %s" % (c["name"], c["thw"], tuple(round(f, 3) for f in c["factors"])))
    for c in DRAW_CASES:
        random.seed(c["seed"])
        rate = utils.get_random_sampling_rate(c["long_rate"], c["sampling_rate"])
        start, _ = decoder.get_start_end_idx(c["total"], c["num_frames"] * rate * c["fps"] / c["target_fps"], -1, 1)
        bright = random.uniform(0.4, 1.4)
        contrast = random.uniform(0.4, 1.4)
        color = random.uniform(0.4, 1.4)
        c["want"] = dict(rate=rate, start=start, factors=[bright, contrast, color], next_random=random.random())
    out["frame_cases"] = json.dumps(FRAME_CASES)
    out["pipe_cases"] = json.dumps(PIPE_CASES)
    out["draw_cases"] = json.dumps(DRAW_CASES)
    path = os.path.join(HERE, "jester_jitter.npz")
    np.savez_compressed(path, **out)
    print("jester_jitter %.1f KB, Pillow %s" % (os.path.getsize(path) / 1024, PIL.__version__))
