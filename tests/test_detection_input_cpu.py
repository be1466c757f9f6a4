"""The detection (AVA) input step, host side (no GPU): `det_clip_params` and `det_boxes` against the reference's own
`Ava._images_and_boxes_preprocessing`, recorded in tests/golden/detection_input.npz (decisions, RNG consumption, boxes
bit for bit; re-derived from the reference where its tree is present), `det_sequence`, the layout of `det_table`, the
collation of boxes and metadata against the reference's `detection_collate`, what the host refuses, and every refusal
of sf_clip_batch_det, all decided before a launch."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _det_input as rec


def _names():
    return sorted(rec.recording()[1])


def test_the_recording_holds_the_cases():
    z, cases = rec.recording()
    assert {c["split"] for c in cases.values()} == {"train", "val", "test"}
    assert {c["bgr"] for c in cases.values()} == {True, False}
    want = {n: c["want"] for n, c in cases.items()}
    assert want["train_landscape"]["new_hw"] != [20, 28] and want["train_portrait_bgr"]["new_hw"][0] > 14
    assert any(v != 0 for v in want["train_pca"]["offsets"]) and want["train_noresize"]["new_hw"] == [20, 28]
    assert want["val_center"]["flip"] is False and want["val_center_flip"]["flip"] is True
    assert z["test_landscape/imgs"].shape == (3, 4, 8, 11) and z["test_portrait_flip_bgr/imgs"].shape == (3, 4, 10, 8)
    assert any(w["flip"] for n, w in want.items() if n.startswith("train")) and any(
        not w["flip"] for n, w in want.items() if n.startswith("train"))
    # boxes that cross the window on every side (clipped to all four edges) and one wholly outside (collapsed)
    all_sides = []
    for n, c in cases.items():
        assert rec.replay(n)[0].crop == c["crop"]  # every case replays through det_clip_params
        b, lim = z[n + "/boxes"], c["crop"] - 1.0
        assert b.dtype == np.float64 and b.shape == (10, 4) and b.min() >= 0.0 and b.max() <= lim
        if bool(((b[:, 0] == 0) & (b[:, 1] == 0) & (b[:, 2] == lim) & (b[:, 3] == lim)).any()):
            all_sides.append(n)
        assert bool(((b[:, 0] == b[:, 2]) | (b[:, 1] == b[:, 3])).any()), n
    assert {"train_landscape", "train_portrait_bgr", "train_pca"} <= set(all_sides), all_sides


@pytest.mark.parametrize("name", _names())
def test_decisions_rng_and_boxes_equal_the_recording(name):
    """Seeded alike, det_clip_params takes the reference's scale, crop, flip and lighting offsets and leaves numpy's
    generator where the reference leaves it (the next draw is recorded); det_boxes gives the reference's float64 boxes
    bit for bit."""
    z, cases = rec.recording()
    c, want = cases[name], cases[name]["want"]
    p, boxes, nxt = rec.replay(name)
    assert [p.new_h, p.new_w] == want["new_hw"] and (p.y, p.x, p.flip) == (want["y"], want["x"], want["flip"])
    assert [np.float32(o) for o in p.offsets] == [np.float32(o) for o in want["offsets"]]
    assert nxt == want["next_numpy"]
    win = tuple(z[name + "/imgs"].shape[2:])
    assert (p.win_h, p.win_w) == win and p.crop == c["crop"]
    assert (p.win_h, p.win_w) == ((p.new_h, p.new_w) if c["split"] == "test" else (c["crop"], c["crop"]))
    ref = z[name + "/boxes"]
    assert boxes.dtype == np.float64 and boxes.shape == ref.shape
    assert np.array_equal(boxes.view(np.int64), ref.view(np.int64)), name


def test_recording_is_what_the_reference_says():
    import make_golden_detection_input as gen
    if not os.path.isdir(gen.DS):
        pytest.skip("the reference's tree is not present here")
    try:
        ava_dataset, transform, utils = gen.load_reference()
    except ImportError as e:
        pytest.skip("the reference's loader modules are not importable here: %s" % e)
    z, cases = rec.recording()
    assert [{k: v for k, v in c.items() if k != "want"} for c in cases.values()] == json.loads(json.dumps(gen.CASES))
    for name, c in cases.items():
        imgs, boxes, seen = gen.reference_record(ava_dataset, transform, c, rec.clip_of(c))
        assert seen == c["want"] and np.array_equal(boxes, z[name + "/boxes"]), name
        assert np.array_equal(imgs, z[name + "/imgs"]), name
        assert np.array_equal(boxes, rec.replay(name)[1]), name  # the reference, run now, against det_boxes
    for key, seq in json.loads(str(z["seq"])).items():
        assert utils.get_sequence(*[int(v) for v in key.split("/")]) == seq


def test_det_sequence_clamps_at_both_ends():
    from slowfast.datasets import utils as ds
    z, _ = rec.recording()
    assert ds.det_sequence(3, 8, 2, 40) == [0, 0, 0, 1, 3, 5, 7, 9]            # the start runs off the front
    assert ds.det_sequence(38, 8, 2, 40) == [30, 32, 34, 36, 38, 39, 39, 39]   # ... the end off the back
    assert ds.det_sequence(20, 8, 2, 40) == list(range(12, 28, 2))
    assert ds.det_sequence(0, 4, 1, 3) == [0, 0, 0, 0, 0, 1, 2, 2]             # both
    for key, seq in json.loads(str(z["seq"])).items():                          # the reference's get_sequence
        assert ds.det_sequence(*[int(v) for v in key.split("/")]) == seq, key


def test_what_the_host_refuses():
    from slowfast.datasets import utils as ds
    _, cases = rec.recording()
    c = cases["train_landscape"]
    state = np.random.get_state()[1].copy()
    with pytest.raises(NotImplementedError, match="pytorch"):
        ds.det_clip_params(rec.case_cfg(c, backend="cv2"), "train", 20, 28)
    cfg = rec.case_cfg(cases["train_pca"])
    cfg.AVA.TRAIN_PCA_JITTER_ONLY = False
    with pytest.raises(NotImplementedError, match="grayscale"):
        ds.det_clip_params(cfg, "train", 20, 28)
    assert np.array_equal(np.random.get_state()[1], state)  # refused before any draw
    with pytest.raises(NotImplementedError):
        ds.det_clip_params(rec.case_cfg(c), "minival", 20, 28)
    cfg = rec.case_cfg(c)
    cfg.DATA.TRAIN_JITTER_SCALES = [8, 8]
    with pytest.raises(ValueError, match="random_crop"):  # 16 x 16 -> 8 x 8: already the crop
        ds.det_clip_params(cfg, "train", 16, 16)
    # full colour jitter is only refused where the reference would run it
    cfg = rec.case_cfg(cases["val_center"])
    cfg.AVA.TRAIN_USE_COLOR_AUGMENTATION, cfg.AVA.TRAIN_PCA_JITTER_ONLY = True, False
    assert ds.det_clip_params(cfg, "val", 20, 28).offsets == (0.0, 0.0, 0.0)


def _videos_and_samples(names, cuda=False):
    _, cases = rec.recording()
    videos = [torch.from_numpy(rec.clip_of(cases[n]).copy()) for n in names]
    if cuda:
        videos = [v.cuda() for v in videos]
    samples = [(torch.arange(4), rec.replay(n)[0]) for n in names]
    return videos, samples


def test_det_table_layout():
    from slowfast.datasets import utils as ds
    names = ["train_pca", "val_center_flip"]
    videos, samples = _videos_and_samples(names)
    samples[1] = (torch.tensor([3, 3, 0, 1]), samples[1][1])
    tab = ds.det_table(videos, samples, ds.slow_frame_indices(4, 2))
    assert ds.DET_ROW == 12 and tab.dtype == torch.int64 and tab.is_contiguous() and tab.numel() == 2 * 12 + 2 * 4 + 2
    p0, p1 = samples[0][1], samples[1][1]
    bits = [int(np.float32(o).view(np.uint32)) for o in p0.offsets]
    assert all(0 < b < 2 ** 32 for b in bits)
    assert tab[:12].tolist() == [videos[0].data_ptr(), 4, 20, 28, p0.new_h, p0.new_w, p0.y, p0.x, 0] + bits
    assert tab[12:24].tolist() == [videos[1].data_ptr(), 4, 20, 28, 8, 11, 0, 2, 1, 0, 0, 0]
    assert tab[24:32].tolist() == [0, 1, 2, 3, 3, 3, 0, 1] and tab[32:].tolist() == [0, 3]
    single = ds.det_table(videos, samples, torch.zeros(0, dtype=torch.long))
    assert single.numel() == 32 and torch.equal(single, tab[:32])
    # the offsets are in the order they are added to SOURCE channels 0..2: rgb[2 - channel] (transform.py:660-661)
    z, cases = rec.recording()
    np.random.seed(cases["train_pca"]["seed"])
    np.random.uniform(), np.random.randint(0, 2), np.random.randint(0, 6), np.random.uniform()  # scale, y, x, flip
    alpha = np.random.normal(0, 0.1, size=(1, 3))
    rgb = (z["eigvec"].astype(np.float32) * alpha * z["eigval"].astype(np.float32).reshape(1, 3)).sum(axis=1)
    assert [np.float32(o) for o in p0.offsets] == [np.float32(rgb[2]), np.float32(rgb[1]), np.float32(rgb[0])]


def test_collation_equals_the_reference():
    """`collate_boxes` / `collate_detection_extras` give `detection_collate`'s float32 boxes, ori_boxes and int64
    metadata (recorded from the reference's loader) bit for bit."""
    from slowfast.datasets import utils as ds
    z, _ = rec.recording()
    names, boxes, ori, meta = rec.collated()
    got = ds.collate_boxes([rec.replay(n)[1] for n in names])
    assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.int32), boxes.view(np.int32))
    k = len(z["boxes01"])
    o, m = ds.collate_detection_extras([z["boxes01"]] * len(names), [[[i + 3, 900 + i]] * k for i in range(len(names))])
    assert o.dtype == torch.float32 and np.array_equal(o.numpy().view(np.int32), ori.view(np.int32))
    assert m.dtype == torch.int64 and np.array_equal(m.numpy(), meta)


def test_binding_declares_the_entry_and_windows_must_agree():
    import sfhip
    from slowfast.datasets import utils as ds
    assert "sf_clip_batch_det" in sfhip._SIGNATURES and "sf_clip_batch_det" in sfhip.EXPORTS
    assert callable(sfhip.clip_batch_det) and callable(ds.gpu_detection_batch)
    tab = torch.zeros(2 * 16 + 2, dtype=torch.int64)
    with pytest.raises(sfhip.SfhipError):  # no CPU fallback
        sfhip.clip_batch_det(tab, tab, 2, (8, 8), [0.45] * 3, [0.225] * 3, torch.zeros(2, 4, 8, 8, 4))
    videos, samples = _videos_and_samples(["train_landscape", "val_center"])
    boxes = [rec.replay(n)[1] for n in ("train_landscape", "val_center")]
    with pytest.raises(sfhip.SfhipError):
        ds.gpu_detection_batch(videos, samples, boxes, [0.45] * 3, [0.225] * 3, 2)
    videos, samples = _videos_and_samples(["val_center", "test_landscape"])  # 8 x 8 and 8 x 11
    with pytest.raises(ValueError, match="window"):
        ds.gpu_detection_batch(videos, samples, boxes, [0.45] * 3, [0.225] * 3, 2)


def test_argument_checks_are_host_only():
    """Every refusal of sf_clip_batch_det is decided on the host before anything is launched, so it can be asked for
    without a GPU: the addresses below are never dereferenced on a device."""
    import sfhip
    from slowfast.datasets import utils as ds
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    L = sfhip.lib()
    videos = [torch.zeros(5, 20, 28, 3, dtype=torch.uint8), torch.zeros(8, 24, 24, 3, dtype=torch.uint8)]
    p0 = ds.DetParams(10, 14, 1, 3, False, 8, 11, 8, (0.0, 0.0, 0.0))       # window 8 x 11 in a 10 x 14 frame
    p1 = ds.DetParams(24, 24, 16, 0, True, 8, 11, 8, (0.01, -0.02, 0.03))
    samples = [(torch.tensor([0, 1, 3, 4]), p0), (torch.tensor([2, 2, 7, 7]), p1)]
    tab = ds.det_table(videos, samples, ds.slow_frame_indices(4, 2))         # 2 x 12 rows, 8 indices, [0, 3]
    m3 = (ctypes.c_float * 3)(0.45, 0.45, 0.45)
    mp = ctypes.cast(m3, ctypes.c_void_p)
    fake = ctypes.c_void_p(4096)  # stands for a device pointer

    def call(tab=tab, table=fake, fast=fake, slow=fake, B=2, n_fast=4, n_slow=2, win_h=8, win_w=11, ph=0, pw=0, wp=11,
             mean=mp, std=mp):
        host = ctypes.c_void_p(tab.data_ptr()) if tab is not None else None
        return L.sf_clip_batch_det(host, table, B, n_fast, n_slow, win_h, win_w, 0, mean, std, fast, slow, ph, pw, wp,
                                   None)

    def edited(pos, val):
        bad = tab.clone()
        bad[pos] = val
        return bad

    def f32(v):
        return int(np.float32(v).view(np.uint32))

    refusals = [
        dict(tab=None), dict(table=None), dict(fast=None), dict(mean=None), dict(std=None),   # null pointers
        dict(B=0), dict(B=-1),                                          # B <= 0
        dict(n_fast=0), dict(win_h=0), dict(win_w=0), dict(win_w=-11), dict(ph=-1), dict(pw=-1),  # non-positive sizes
        dict(tab=edited(1, 0)), dict(tab=edited(12 + 2, 0)), dict(tab=edited(3, -28)),  # T, H, W of a row
        dict(tab=edited(4, 0)), dict(tab=edited(12 + 5, -24)),          # ... and its scaled size
        dict(tab=edited(12, 0)),                                        # a zero clip address
        dict(tab=edited(6, 3)), dict(tab=edited(7, 4)),                 # y0 + 8 > new_h = 10, x0 + 11 > new_w = 14
        dict(win_h=10), dict(win_w=12),                                 # the window outside the scaled frame, either way
        dict(tab=edited(6, -1)), dict(tab=edited(12 + 6, 17)), dict(tab=edited(12 + 7, 14)),  # negative; 17 + 8 > 24; 14 + 11 > 24
        dict(tab=edited(24 + 3, 5)), dict(tab=edited(24 + 4, -1)),      # frame 5 of T_0 = 5; a negative frame
        dict(tab=edited(24 + 7, 8)),                                    # frame 8 of T_1 = 8
        dict(n_slow=5),                                                 # n_slow > n_fast
        dict(tab=edited(33, 4)), dict(tab=edited(32, -1)),              # a Slow position outside [0, n_fast)
        dict(tab=edited(33, 0)), dict(tab=edited(32, 3)),               # ... repeated, decreasing
        dict(slow=None), dict(n_slow=0),                                # slow without n_slow and the reverse
        dict(pw=1), dict(wp=10), dict(pw=3, wp=16),                     # Wp < win_w + 2 pw
        dict(B=65536), dict(n_fast=65536),                              # beyond the grid's y / z extent
        dict(tab=edited(9, f32(np.inf))), dict(tab=edited(12 + 10, f32(-np.inf))), dict(tab=edited(11, f32(np.nan))),
        dict(tab=edited(12 + 9, -1)), dict(tab=edited(10, 2 ** 32)),    # not a float32 bit pattern at all
        dict(fast=ctypes.c_void_p(4096 + 4)), dict(slow=ctypes.c_void_p(4096 + 8)),  # not 16-byte aligned
    ]
    for kw in refusals:
        assert call(**kw) == sfhip.SF_EINVAL, kw
    # a plane beyond the 32-bit index of one frame
    assert call(win_h=8, ph=2 ** 28, wp=11) == sfhip.SF_EINVAL
