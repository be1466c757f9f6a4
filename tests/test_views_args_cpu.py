"""Multi-view testing, host side (no GPU): the view table of `datasets.utils.test_view_params` against hand-checked
cases, against the reference's recorded frame indices (tests/golden/view_indices.json, written by
make_golden_views.py) and — where the reference tree is present — against its own decoder functions; and the
construction of `utils.meters.DeviceTestMeter`."""
import json
import os

import pytest
import torch

from slowfast.config.defaults import get_cfg
from slowfast.datasets import utils as ds
from slowfast.utils import meters


def _cfg(num_frames=8, sampling_rate=2, views=3, crops=3, crop=16, target_fps=30):
    cfg = get_cfg()
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.DATA.TARGET_FPS = num_frames, sampling_rate, target_fps
    cfg.DATA.TEST_CROP_SIZE = crop
    cfg.TEST.NUM_ENSEMBLE_VIEWS, cfg.TEST.NUM_SPATIAL_CROPS = views, crops
    return cfg


# span = 2 * 8 = 16 frames, delta = 40 - 16 = 24, start = 24 * idx / 3 = 0, 8, 16, end = start + 15;
# linspace(start, start + 15, 8) has the step 15 / 7 = 2.142...: offsets 0, 2.14, 4.29, 6.43, 8.57, 10.71, 12.86, 15
_OFFSETS = [0, 2, 4, 6, 8, 10, 12, 15]


@pytest.mark.parametrize("h,w", [(20, 28), (28, 20)])
def test_nine_views_in_reference_order(h, w):
    views = ds.test_view_params(_cfg(), 40, h, w)
    assert len(views) == 9
    # short side 20 -> 16, long side floor(28 / 20 * 16) = 22: the crop slides over 22 - 16 = 6, centre ceil(6 / 2) = 3
    for i, (frames, p) in enumerate(views):
        t_idx, s_idx = i // 3, i % 3
        assert frames.dtype == torch.int64 and frames.tolist() == [8 * t_idx + o for o in _OFFSETS], i
        assert frames[0] == 24 * t_idx // 3
        off = (0, 3, 6)[s_idx]
        if w > h:  # landscape: left / centre / right
            assert p == ds.SpatialParams(16, 22, 0, off, False, 16), i
        else:      # portrait: top / centre / bottom
            assert p == ds.SpatialParams(22, 16, off, 0, False, 16), i


def test_video_shorter_than_the_span():
    views = ds.test_view_params(_cfg(), 10, 20, 28)
    assert len(views) == 9
    for frames, _ in views:  # delta = 0: every temporal view starts at 0 and runs off the end, clamped at frame 9
        assert frames.tolist() == [0, 2, 4, 6, 8, 9, 9, 9]


def test_one_frame_video():
    views = ds.test_view_params(_cfg(), 1, 16, 16)
    assert len(views) == 9
    for frames, p in views:
        assert frames.tolist() == [0] * 8
        assert p == ds.SpatialParams(16, 16, 0, 0, False, 16)  # 16 x 16 at crop 16: no resampling, nothing to slide


def test_fps_none_means_target_fps():
    a = ds.test_view_params(_cfg(), 40, 20, 28)
    b = ds.test_view_params(_cfg(), 40, 20, 28, fps=30)
    c = ds.test_view_params(_cfg(), 40, 20, 28, fps=15)  # half the rate: the clip spans 8 decoded frames
    assert all(x[0].tolist() == y[0].tolist() and x[1] == y[1] for x, y in zip(a, b))
    assert c[0][0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and c[8][0].tolist()[0] == 32 * 2 // 3


def _restated(c):
    cfg = _cfg(c["num_frames"], c["sampling_rate"], c["num_clips"], 3, 16, c["target_fps"])
    views = ds.test_view_params(cfg, c["total"], 20, 28, fps=c["fps"])
    assert len(views) == 3 * c["num_clips"]
    for i in range(0, len(views), 3):  # the spatial crops of one temporal view share its frames
        assert views[i][0].tolist() == views[i + 1][0].tolist() == views[i + 2][0].tolist()
    return [views[3 * i][0].tolist() for i in range(c["num_clips"])]


def _recorded(repo_root):
    with open(os.path.join(repo_root, "tests", "golden", "view_indices.json")) as f:
        return json.load(f)


def test_frame_indices_match_the_recording(repo_root):
    rec = _recorded(repo_root)
    assert len(rec) >= 8
    for c in rec:
        assert _restated(c) == c["indices"], c


def test_frame_indices_match_the_reference(repo_root):
    import make_golden_views as gen
    try:
        decoder = gen.load_reference_decoder()
    except ImportError as e:
        pytest.skip("the reference's decoder is not importable here: %s" % e)
    rec = _recorded(repo_root)
    assert [{k: v for k, v in c.items() if k != "indices"} for c in rec] == gen.CASES
    for c in rec:
        want = gen.reference_indices(decoder, c)
        assert want == c["indices"], c  # the fixture is what the reference says today
        assert _restated(c) == want, c


def test_view_table_layout():
    views = ds.test_view_params(_cfg(), 40, 28, 20)
    tab = ds.view_table(views, ds.slow_frame_indices(8, 4))
    assert tab.dtype == torch.int32 and tab.numel() == 9 * 5 + 9 * 8 + 2
    assert tab[:10].tolist() == [22, 16, 0, 0, 0, 22, 16, 3, 0, 0]
    assert tab[45:53].tolist() == _OFFSETS and tab[-2:].tolist() == [0, 7]


def test_device_meter_constructs_and_is_exported():
    assert meters.DeviceTestMeter.__module__ == "slowfast.utils.meters"
    assert issubclass(meters.DeviceTestMeter, meters.TestMeter)
    m = meters.DeviceTestMeter(4, 9, 7, 12, multi_label=False, ensemble_method="max")
    assert (m.num_clips, m.overall_iters, m.ensemble_method) == (9, 12, "max")
    for name in ("update_stats", "iter_tic", "iter_toc", "log_iter_stats", "reset", "finalize_metrics"):
        assert callable(getattr(m, name))
    m.reset()
    m.iter_tic()
    m.iter_toc()
    assert m.log_iter_stats(0)["split"] == "test_iter"
    for cls in (meters.TestMeter, meters.DeviceTestMeter):
        with pytest.raises(NotImplementedError, match="Ensemble Method mean is not supported"):
            cls(4, 9, 7, 12, ensemble_method="mean")
    with pytest.raises(NotImplementedError, match="multi-label"):
        meters.DeviceTestMeter(4, 9, 7, 12, multi_label=True).finalize_metrics()


def test_binding_declares_the_view_entries():
    import sfhip
    for name in ("sf_clip_views", "sf_clip_views_gray", "sf_ensemble_update"):
        assert name in sfhip._SIGNATURES
    assert callable(sfhip.clip_views) and callable(sfhip.ensemble_update)
    with pytest.raises(sfhip.SfhipError):  # no CPU fallback
        sfhip.clip_views(torch.zeros(2, 4, 4, 3, dtype=torch.uint8), torch.zeros(8, dtype=torch.int32),
                         torch.zeros(8, dtype=torch.int32), 0, 4, [0.45] * 3, [0.225] * 3, torch.zeros(1, 2, 4, 4, 4))


def test_argument_checks_are_host_only():
    """Every refusal of sf_clip_views / sf_ensemble_update is decided on the host before anything is launched, so it
    can be asked for without a GPU: the pointers below are never dereferenced on a device."""
    import ctypes
    import sfhip
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    L = sfhip.lib()
    views = ds.test_view_params(_cfg(), 40, 20, 28)
    tab = ds.view_table(views, ds.slow_frame_indices(8, 4))
    m3 = (ctypes.c_float * 3)(0.45, 0.45, 0.45)
    mp = ctypes.cast(m3, ctypes.c_void_p)
    fake = ctypes.c_void_p(4096)  # stands for a device pointer

    def call(tab=tab, video=fake, table=fake, fast=fake, slow=fake, V=9, n_fast=8, n_slow=2, T=40):
        return L.sf_clip_views(video, T, 20, 28, ctypes.c_void_p(tab.data_ptr()) if tab is not None else None, table, V,
                               n_fast, n_slow, 16, 0, mp, mp, fast, slow, 0, 0, 16, None)

    for kw in (dict(video=None), dict(table=None), dict(tab=None), dict(fast=None), dict(V=0), dict(V=-1),
               dict(n_slow=9, n_fast=8), dict(slow=None), dict(n_slow=0), dict(T=31)):  # T = 31: frame 31 is outside
        assert call(**kw) == sfhip.SF_EINVAL, kw
    for col, val in ((2, 1), (3, 7), (2, -1), (0, 0)):  # y0 + crop > new_h, x0 + crop > new_w, negative, no height
        bad = tab.clone()
        bad[5 * 4 + col] = val
        assert call(tab=bad) == sfhip.SF_EINVAL, (col, val)
    bad = tab.clone()
    bad[-1] = 8  # a Slow position outside the Fast frames
    assert call(tab=bad) == sfhip.SF_EINVAL
    bad[-1] = 0  # ... and one that repeats
    assert call(tab=bad) == sfhip.SF_EINVAL
    ip = ctypes.cast(fake, ctypes.POINTER(ctypes.c_int))
    for kw in (dict(B=0), dict(K=0), dict(Nv=0), dict(mode=2), dict(preds=None)):
        a = dict(preds=fake, B=5, K=7, Nv=4, mode=0)
        a.update(kw)
        assert L.sf_ensemble_update(a["preds"], fake, None, fake, ip, ip, ip, a["B"], a["K"], a["Nv"], a["mode"],
                                    None) == sfhip.SF_EINVAL, kw
