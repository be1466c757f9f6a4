"""Jester's colour jitter, host side (no GPU): the numpy restatement of the contract (tests/_jitter_ref.py) against the
frames the reference's transform.RandomColorJitter produced with PIL (tests/golden/jester_jitter.npz, written by
make_golden_jester_jitter.py), and `datasets.utils.jester_clip_params` against the draws decoder.decode(..., jester=True)
takes from Python's `random`.  Every comparison is exact."""
import json
import os
import random

import numpy as np
import pytest
import torch

import _jitter_ref as ref
from _util import GOLDEN
from slowfast.config.defaults import get_cfg
from slowfast.datasets import utils as ds


def _golden():
    return np.load(os.path.join(GOLDEN, "jester_jitter.npz"))


def test_restatement_equals_the_reference_frames():
    z = _golden()
    cases = json.loads(str(z["frame_cases"]))
    assert len(cases) >= 12
    same = set()
    for c in cases:
        clip, want = z[c["name"] + "/clip"], z[c["name"] + "/jittered"]
        got = ref.jitter_clip(clip, *c["factors"])
        assert got.dtype == np.uint8 and np.array_equal(got, want), c["name"]
        if np.array_equal(want, clip):
            same.add(c["name"])
    # the fixture is not a set of identities: only no stage at all, white under factors above 1, and the two-level
    # frame whose mean is its upper level (blend(0.5, 101, 100) = 100.5 truncates to 100) leave a clip as it was
    assert same == {"none", "saturated", "mean_half_up"}
    # what the cases were built for: both rounding directions of the mean, saturation, both ends of the clip
    by = {c["name"]: c for c in cases}
    assert ref.grey_mean(z["mean_half_up/clip"][0], 1.0) == 101 and ref.grey_mean(z["mean_below_half/clip"][0], 1.0) == 100
    assert ref.grey_mean(z["saturated/clip"][0], by["saturated"]["factors"][0]) == 255
    assert z["above_one/jittered"].max() == 255 and z["above_one/jittered"].min() == 0
    assert np.array_equal(z["none/jittered"], z["none/clip"])


def test_blend_rules():
    """Inside [0, 1] the value is truncated, outside it is clipped first; the product and the sum round separately."""
    x = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ref.blend(1.0, x[::-1].copy(), x), x) and np.array_equal(ref.blend(0.0, x[::-1].copy(), x), x[::-1])
    assert ref.blend(1.4, 0, 200).tolist() == 255 and ref.blend(1.4, 200, 0).tolist() == 0
    assert ref.blend(0.5, 0, 255).tolist() == 127 and ref.blend(0.5, 255, 0).tolist() == 127
    f = np.float32(0.7)
    want = np.float32(np.float32(100) + np.float32(f * np.float32(-37)))
    assert ref.blend(0.7, 100, 63).tolist() == int(want)
    assert ref.grey(np.array([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)).tolist() == [
        255, 0, 76, 150, 29]


def _cfg(c):
    cfg = get_cfg()
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.DATA.TARGET_FPS = c["num_frames"], c["sampling_rate"], c["target_fps"]
    cfg.DATA.TRAIN_JITTER_SCALES, cfg.DATA.TRAIN_CROP_SIZE = [64, 80], 56
    cfg.MULTIGRID.DEFAULT_S, cfg.MULTIGRID.LONG_CYCLE_SAMPLING_RATE = 0, c["long_rate"]
    return cfg


@pytest.mark.parametrize("mode", ["train", "val"])
def test_jester_clip_params_take_the_recorded_draws(mode):
    """Seeded alike, jester_clip_params draws what decode(..., jester=True) draws from `random` — sampling rate, window
    start, bright, contrast, color — and leaves `random` where decode leaves it; numpy's generator is where
    train_clip_params leaves it (the jitter does not touch it)."""
    cases = json.loads(str(_golden()["draw_cases"]))
    assert len(cases) >= 3 and any(c["long_rate"] > 0 for c in cases)
    for c in cases:
        cfg, w = _cfg(c), c["want"]
        random.seed(c["seed"])
        np.random.seed(c["seed"])
        frames, params, jit = ds.jester_clip_params(cfg, mode, c["total"], c["h"], c["w"], fps=c["fps"])
        assert random.random() == w["next_random"], c["seed"]
        after_numpy = np.random.uniform()
        assert isinstance(jit, ds.ColorJitter) and list(jit) == w["factors"], c["seed"]
        assert all(0.4 <= v <= 1.4 for v in jit)
        span = c["num_frames"] * w["rate"] * c["fps"] / c["target_fps"]
        index = torch.linspace(w["start"], w["start"] + span - 1, c["num_frames"])
        assert frames.tolist() == torch.clamp(index, 0, c["total"] - 1).long().tolist(), c["seed"]
        # the same seeds through train_clip_params: the same frames and spatial decisions, the same numpy state
        random.seed(c["seed"])
        np.random.seed(c["seed"])
        frames2, params2 = ds.train_clip_params(cfg, c["total"], c["h"], c["w"], fps=c["fps"])
        assert frames2.tolist() == frames.tolist() and params2 == params
        assert np.random.uniform() == after_numpy
        assert random.random() != w["next_random"]  # three draws short of decode()


def test_sample_color_jitter_order_and_source():
    random.seed(5)
    want = [random.uniform(0.4, 1.4) for _ in range(3)]
    random.seed(5)
    state = np.random.get_state()[1].copy()
    j = ds.sample_color_jitter()
    assert (j.bright, j.contrast, j.color) == tuple(want)
    assert np.array_equal(np.random.get_state()[1], state)  # Python's `random`, not numpy
    random.seed(5)
    lo = ds.sample_color_jitter(0.9, 1.1)
    assert all(0.9 <= v <= 1.1 for v in lo)


def test_test_mode_raises():
    c = json.loads(str(_golden()["draw_cases"]))[0]
    state = random.getstate()
    with pytest.raises(NotImplementedError, match="test_view_params"):
        ds.jester_clip_params(_cfg(c), "test", c["total"], c["h"], c["w"])
    with pytest.raises(NotImplementedError):
        ds.jester_clip_params(_cfg(c), "trainval", c["total"], c["h"], c["w"])
    assert random.getstate() == state  # nothing was drawn
