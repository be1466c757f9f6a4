#!/usr/bin/env python3
"""Recorded frame indices of the test-time views, produced by the REFERENCE's own slowfast/datasets/decoder.py
get_start_end_idx (:55-83) and temporal_sampling (:35-52), called as decoder.decode calls them (:447-454).

Build container only.  decoder.py cannot be imported as part of its package here (the package pulls in cv2 / av, the
module itself torchvision), so it is loaded by path under a synthetic package with inert stand-ins for the modules
that are not installed (neither function touches them); `sys.modules` is put back afterwards.  Writes tests/golden/view_indices.json: the cases and,
per case, the indices of every temporal view."""
import importlib.util
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DS = "/root/reference/SlowFast/slowfast/datasets"

# (frames in the decoded video, DATA.NUM_FRAMES, DATA.SAMPLING_RATE, fps, DATA.TARGET_FPS, TEST.NUM_ENSEMBLE_VIEWS)
CASES = [
    dict(total=40, num_frames=8, sampling_rate=2, fps=30, target_fps=30, num_clips=3),
    dict(total=10, num_frames=8, sampling_rate=2, fps=30, target_fps=30, num_clips=3),
    dict(total=1, num_frames=8, sampling_rate=2, fps=30, target_fps=30, num_clips=3),
    dict(total=300, num_frames=32, sampling_rate=2, fps=30, target_fps=30, num_clips=10),
    dict(total=250, num_frames=32, sampling_rate=2, fps=25, target_fps=30, num_clips=10),
    dict(total=301, num_frames=8, sampling_rate=8, fps=29.97, target_fps=30, num_clips=10),
    dict(total=97, num_frames=4, sampling_rate=16, fps=24, target_fps=30, num_clips=7),
    dict(total=64, num_frames=64, sampling_rate=1, fps=30, target_fps=30, num_clips=1),
]


STAND_INS = ("cv2", "scipy", "scipy.ndimage", "torchvision", "torchvision.io", "torchvision.transforms", "PIL",
             "PIL.Image", "PIL.ImageOps", "PIL.ImageEnhance", "slowfast", "slowfast.datasets", "slowfast.datasets.utils")


def load_reference_decoder():
    """The reference's decoder module, or raises (no reference tree, or an import the stand-ins do not cover)."""
    if not os.path.isfile(os.path.join(DS, "decoder.py")):
        raise ImportError("no reference tree at " + DS)
    sys.dont_write_bytecode = True
    saved = dict(sys.modules)
    try:
        for name in STAND_INS:  # only for what is not installed; parents come before their children
            try:
                importlib.import_module(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
                if "." in name:
                    setattr(sys.modules[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], sys.modules[name])
        if not hasattr(sys.modules["torchvision.transforms"], "ToTensor"):
            sys.modules["torchvision.transforms"].ToTensor = object
        pkg = types.ModuleType("sfdec")
        pkg.__path__ = [DS]
        sys.modules["sfdec"] = pkg
        mods = {}
        for name in ("transform", "decoder"):
            spec = importlib.util.spec_from_file_location("sfdec." + name, os.path.join(DS, name + ".py"))
            m = importlib.util.module_from_spec(spec)
            sys.modules["sfdec." + name] = m
            spec.loader.exec_module(m)
            mods[name] = m
        return mods["decoder"]
    finally:
        for name in STAND_INS + ("sfdec", "sfdec.transform", "sfdec.decoder"):
            if name in saved:
                sys.modules[name] = saved[name]
            else:
                sys.modules.pop(name, None)


def reference_indices(decoder, c):
    """Per temporal view, the frames decoder.decode selects from a fully decoded video of c['total'] frames."""
    frames = torch.arange(c["total"], dtype=torch.float32).view(-1, 1, 1, 1)  # each frame holds its own number
    out = []
    for clip_idx in range(c["num_clips"]):
        start, end = decoder.get_start_end_idx(
            frames.shape[0], c["num_frames"] * c["sampling_rate"] * c["fps"] / c["target_fps"], clip_idx, c["num_clips"])
        out.append(decoder.temporal_sampling(frames, start, end, c["num_frames"]).flatten().long().tolist())
    return out


if __name__ == "__main__":
    dec = load_reference_decoder()
    rec = [dict(c, indices=reference_indices(dec, c)) for c in CASES]
    path = os.path.join(HERE, "view_indices.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rec) + "\n]\n")  # one case per line
    for r in rec:
        print(r["total"], r["num_frames"], r["indices"][0], "...", r["indices"][-1])
    print("view_indices %.1f KB" % (os.path.getsize(path) / 1024))
