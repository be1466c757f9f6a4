"""The training input step, host side (no GPU): `datasets.utils.train_clip_params` against hand-checked cases and
against the reference's recorded decisions and RNG consumption (tests/golden/train_clip_params.json, written by
make_golden_train_params.py; re-derived from the reference's own functions where its tree is present), the layout of
`batch_table`, and every refusal of sf_clip_batch / sf_clip_batch_gray, all decided on the host before a launch."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

from slowfast.config.defaults import get_cfg
from slowfast.datasets import utils as ds


def _cfg(num_frames=8, sampling_rate=2, default_s=224, jitter=(256, 320), train_crop=224, long_rate=0,
         target_fps=30, flip=True, inv=False, factors=(0.5, 0.5 ** 0.5)):
    cfg = get_cfg()
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.DATA.TARGET_FPS = num_frames, sampling_rate, target_fps
    cfg.DATA.TRAIN_JITTER_SCALES, cfg.DATA.TRAIN_CROP_SIZE = list(jitter), train_crop
    cfg.DATA.RANDOM_FLIP, cfg.DATA.INV_UNIFORM_SAMPLE = flip, inv
    cfg.MULTIGRID.DEFAULT_S, cfg.MULTIGRID.SHORT_CYCLE_FACTORS = default_s, list(factors)
    cfg.MULTIGRID.LONG_CYCLE_SAMPLING_RATE = long_rate
    return cfg


class _Spy:
    """Records the (min_scale, max_scale, crop_size) train_clip_params hands to sample_spatial_params."""

    def __init__(self, monkeypatch):
        self.seen = []
        real = ds.sample_spatial_params

        def spy(height, width, spatial_idx=-1, min_scale=256, max_scale=320, crop_size=224, **kw):
            self.seen.append((spatial_idx, min_scale, max_scale, crop_size))
            return real(height, width, spatial_idx, min_scale, max_scale, crop_size, **kw)

        monkeypatch.setattr(ds, "sample_spatial_params", spy)


@pytest.mark.parametrize("idx,crop,min_scale", [(0, 112, 128), (1, 158, 181), (2, 224, 256), (None, 224, 256)])
def test_short_cycle_crop_and_jitter(monkeypatch, idx, crop, min_scale):
    """DEFAULT_S 224, factors [0.5, 0.5**0.5], jitter [256, 320]: round(0.5 * 224) = 112 and round(256 * 112 / 224) =
    128; round(0.70711 * 224) = round(158.39) = 158 and round(256 * 158 / 224) = round(180.57) = 181; max_scale stays."""
    spy = _Spy(monkeypatch)
    random.seed(0)
    np.random.seed(0)
    frames, p = ds.train_clip_params(_cfg(), 300, 256, 340, short_cycle_idx=idx)
    assert spy.seen == [(-1, min_scale, 320, crop)]
    assert p.crop == crop and min_scale <= p.new_h <= 320 and p.new_w == int(np.floor(340 / 256 * p.new_h))
    assert 0 <= p.y <= p.new_h - crop and 0 <= p.x <= p.new_w - crop
    assert frames.dtype == torch.int64 and frames.numel() == 8


def test_default_s_zero_leaves_min_scale(monkeypatch):
    spy = _Spy(monkeypatch)
    ds.train_clip_params(_cfg(default_s=0), 300, 256, 340)
    ds.train_clip_params(_cfg(default_s=0, jitter=(200, 300), train_crop=128), 300, 256, 340, short_cycle_idx=None)
    assert spy.seen == [(-1, 256, 320, 224), (-1, 200, 300, 128)]


def test_window_start_lies_in_delta():
    """span = 8 * 2 = 16 frames of 40: delta = 24; linspace(start, start + 15, 8) truncated -> the first index is
    floor(start) in [0, 24], the last floor(start + 15) in [15, 39], the rest spaced 15 / 7 apart."""
    cfg = _cfg()
    starts = set()
    for seed in range(40):
        random.seed(seed)
        state = random.getstate()
        frames, _ = ds.train_clip_params(cfg, 40, 256, 340)
        random.setstate(state)
        start = random.uniform(0, 24)  # the one draw from `random` (LONG_CYCLE_SAMPLING_RATE is 0)
        assert 0 <= start <= 24
        want = torch.clamp(torch.linspace(start, start + 15, 8), 0, 39).long()
        assert frames.tolist() == want.tolist() and 0 <= frames[0] <= 24 and frames[-1] <= 39
        starts.add(int(frames[0]))
    assert len(starts) > 10  # the window moves


def test_video_shorter_than_the_span_repeats_its_last_frame():
    frames, _ = ds.train_clip_params(_cfg(), 10, 256, 340)  # delta = 0: start 0, indices run off the end
    assert frames.tolist() == [0, 2, 4, 6, 8, 9, 9, 9]
    frames, _ = ds.train_clip_params(_cfg(), 1, 256, 340)
    assert frames.tolist() == [0] * 8
    frames, _ = ds.train_clip_params(_cfg(), 40, 256, 340, fps=15)  # half the rate: the clip spans 8 decoded frames
    assert (frames[1:] - frames[:-1]).tolist() == [1] * 7


def test_sampling_rate_draws_only_in_a_long_cycle():
    random.seed(7)
    before = random.getstate()
    assert ds.get_random_sampling_rate(0, 2) == 2
    assert random.getstate() == before  # LONG_CYCLE_SAMPLING_RATE 0: nothing drawn
    rates = {ds.get_random_sampling_rate(8, 2) for _ in range(200)}
    assert rates == set(range(2, 9)) and random.getstate() != before
    with pytest.raises(AssertionError):
        ds.get_random_sampling_rate(1, 2)
    # train_clip_params: with the rate fixed the window start is the FIRST draw from `random`
    random.seed(7)
    frames, _ = ds.train_clip_params(_cfg(), 40, 256, 340)
    random.seed(7)
    assert int(frames[0]) == int(random.uniform(0, 24))


def _recorded(repo_root):
    with open(os.path.join(repo_root, "tests", "golden", "train_clip_params.json")) as f:
        return json.load(f)


def _restated(c):
    cfg = _cfg(c["num_frames"], c["sampling_rate"], c["default_s"], c["jitter"], c["train_crop"], c["long_rate"],
               c["target_fps"], c["flip"], c["inv"], c["factors"])
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    frames, p = ds.train_clip_params(cfg, c["total"], c["h"], c["w"], short_cycle_idx=c["short_cycle_idx"], fps=c["fps"])
    return dict(indices=frames.tolist(), new_h=p.new_h, new_w=p.new_w, y=p.y, x=p.x, flip=p.flip, crop=p.crop,
                next_random=random.random(), next_numpy=float(np.random.uniform()))


def test_decisions_and_rng_order_match_the_recording(repo_root):
    """Seeded alike, train_clip_params takes the reference's frames, scale, crop and flip and leaves both generators
    where the reference's four calls leave them (the next draw of each is recorded)."""
    rec = _recorded(repo_root)
    assert len(rec) >= 6
    assert {c["short_cycle_idx"] for c in rec} >= {None, 0, 1, 2} and any(c["want"]["flip"] for c in rec)
    assert any(c["long_rate"] > 0 for c in rec) and any(c["long_rate"] == 0 for c in rec)
    for c in rec:
        got, want = _restated(c), c["want"]
        assert got.pop("crop") == c["crop_size"], c
        assert got == {k: want[k] for k in got}, c


def test_recording_is_what_the_reference_says(repo_root):
    import make_golden_train_params as gen
    try:
        utils, decoder = gen.load_reference()
    except ImportError as e:
        pytest.skip("the reference's loader modules are not importable here: %s" % e)
    rec = _recorded(repo_root)
    assert [{k: v for k, v in c.items() if k != "want"} for c in rec] == json.loads(json.dumps(gen.CASES))
    for c in rec:
        assert gen.reference_record(utils, decoder, c) == c["want"], c


def _samples():
    p0 = ds.SpatialParams(10, 14, 1, 3, False, 8)
    p1 = ds.SpatialParams(24, 24, 16, 0, True, 8)
    return [(torch.tensor([0, 1, 3, 4]), p0), (torch.tensor([2, 2, 7, 7]), p1)]


def test_batch_table_layout():
    videos = [torch.zeros(5, 20, 28, 3, dtype=torch.uint8), torch.zeros(8, 24, 24, 3, dtype=torch.uint8)]
    tab = ds.batch_table(videos, _samples(), ds.slow_frame_indices(4, 2))
    assert tab.dtype == torch.int64 and tab.is_contiguous() and tab.numel() == 2 * ds.BATCH_ROW + 2 * 4 + 2
    assert tab[:9].tolist() == [videos[0].data_ptr(), 5, 20, 28, 10, 14, 1, 3, 0]
    assert tab[9:18].tolist() == [videos[1].data_ptr(), 8, 24, 24, 24, 24, 16, 0, 1]
    assert tab[18:26].tolist() == [0, 1, 3, 4, 2, 2, 7, 7] and tab[26:].tolist() == [0, 3]
    single = ds.batch_table(videos, _samples(), torch.zeros(0, dtype=torch.long))
    assert single.numel() == 26 and torch.equal(single, tab[:26])


def test_binding_declares_the_batch_entries():
    import sfhip
    for name in ("sf_clip_batch", "sf_clip_batch_gray"):
        assert name in sfhip._SIGNATURES
    assert callable(sfhip.clip_batch) and callable(ds.gpu_train_batch)
    tab = torch.zeros(2 * 13 + 2, dtype=torch.int64)
    with pytest.raises(sfhip.SfhipError):  # no CPU fallback
        sfhip.clip_batch(tab, tab, 2, 8, [0.45] * 3, [0.225] * 3, torch.zeros(2, 4, 8, 8, 4))
    videos = [torch.zeros(5, 20, 28, 3, dtype=torch.uint8), torch.zeros(8, 24, 24, 3, dtype=torch.uint8)]
    with pytest.raises(sfhip.SfhipError):
        ds.gpu_train_batch(videos, _samples(), [0.45] * 3, [0.225] * 3, 2)


def test_argument_checks_are_host_only():
    """Every refusal of sf_clip_batch / sf_clip_batch_gray is decided on the host before anything is launched, so it can
    be asked for without a GPU: the addresses below are never dereferenced on a device."""
    import sfhip
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    L = sfhip.lib()
    videos = [torch.zeros(5, 20, 28, 3, dtype=torch.uint8), torch.zeros(8, 24, 24, 3, dtype=torch.uint8)]
    tab = ds.batch_table(videos, _samples(), ds.slow_frame_indices(4, 2))
    m3 = (ctypes.c_float * 3)(0.45, 0.45, 0.45)
    mp = ctypes.cast(m3, ctypes.c_void_p)
    fake = ctypes.c_void_p(4096)  # stands for a device pointer

    def call(gray, tab=tab, table=fake, fast=fake, slow=fake, B=2, n_fast=4, n_slow=2, crop=8, pw=0, wp=8, mean=mp):
        host = ctypes.c_void_p(tab.data_ptr()) if tab is not None else None
        if gray:
            return L.sf_clip_batch_gray(host, table, B, n_fast, n_slow, crop, 0.45, 0.225, fast, slow, 0, pw, wp, None)
        return L.sf_clip_batch(host, table, B, n_fast, n_slow, crop, 0, mean, mp, fast, slow, 0, pw, wp, None)

    def edited(pos, val):
        bad = tab.clone()
        bad[pos] = val
        return bad

    refusals = [
        dict(tab=None), dict(table=None), dict(fast=None),              # null pointers
        dict(B=0), dict(B=-1),                                          # B <= 0
        dict(n_fast=0), dict(crop=0), dict(pw=-1),                      # non-positive sizes
        dict(tab=edited(1, 0)), dict(tab=edited(9 + 2, 0)), dict(tab=edited(3, -28)),   # T, H, W of a row
        dict(tab=edited(4, 0)), dict(tab=edited(9 + 5, -24)),           # ... and its scaled size
        dict(tab=edited(9, 0)),                                         # a zero clip address
        dict(tab=edited(6, 3)), dict(tab=edited(7, 7)),                 # y0 + crop > new_h = 10, x0 + crop > new_w = 14
        dict(tab=edited(6, -1)), dict(tab=edited(9 + 6, 17)),           # a negative offset; 17 + 8 > 24
        dict(tab=edited(18 + 3, 5)), dict(tab=edited(18 + 4, -1)),      # frame 5 of T_0 = 5; a negative frame
        dict(tab=edited(18 + 7, 8)),                                    # frame 8 of T_1 = 8
        dict(n_slow=5),                                                 # n_slow > n_fast
        dict(tab=edited(27, 4)), dict(tab=edited(26, -1)),              # a Slow position outside [0, n_fast)
        dict(tab=edited(27, 0)), dict(tab=edited(26, 3)),               # ... repeated, decreasing
        dict(slow=None), dict(n_slow=0),                                # slow without n_slow and the reverse
        dict(pw=1), dict(wp=7),                                         # Wp < crop + 2 pw
        dict(B=65536), dict(n_fast=65536),                              # beyond the grid's y / z extent
    ]
    for gray in (False, True):
        for kw in refusals:
            assert call(gray, **kw) == sfhip.SF_EINVAL, (gray, kw)
    assert call(False, mean=None) == sfhip.SF_EINVAL
    # misaligned buffers: the RGB entry stores 16 bytes at a time, the one-channel entry needs a float's alignment
    for kw in (dict(fast=ctypes.c_void_p(4096 + 4)), dict(slow=ctypes.c_void_p(4096 + 8))):
        assert call(False, **kw) == sfhip.SF_EINVAL, kw
    for kw in (dict(fast=ctypes.c_void_p(4096 + 2)), dict(slow=ctypes.c_void_p(4096 + 1))):
        assert call(True, **kw) == sfhip.SF_EINVAL, kw
