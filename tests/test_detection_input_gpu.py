"""The detection (AVA) input step on the GPU: one launch per batch (datasets.utils.gpu_detection_batch ->
sf_clip_batch_det) against the reference's own `Ava._images_and_boxes_preprocessing` recorded in float64
(tests/golden/detection_input.npz), with the layout's zeros, owned-memory margins, the Slow selection, the device-side
row check, the collated boxes, and a detection model fed from the packed clips."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import _det_input as rec

pytestmark = pytest.mark.gpu

N_FAST = 4
SENTINEL, MARGIN = 12345.0, 64  # floats either side of each output buffer (256 B: the buffers stay 16-byte aligned)

# The recorded cases as batches: one output window and one AVA.BGR per batch, every clip its own allocation and size.
BATCHES = {
    "square_rgb": ["train_landscape", "train_pca", "train_noresize", "val_center", "val_center_flip"],  # 8 x 8
    "square_bgr": ["train_portrait_bgr", "val_portrait_bgr"],                                             # 8 x 8
    "test_landscape": ["test_landscape"],                                                                 # 8 x 11
    "test_portrait": ["test_portrait_flip_bgr"],                                                          # 10 x 8
}
BATCH_OF = {n: b for b, names in BATCHES.items() for n in names}

# (batch, alpha, (ph, pw), Wp): Wp 14 and 16 with pad (3, 3), pad (0, 0), the 11-wide window with pad (3, 3) (Wp 17);
# alpha None: a single-pathway model
LAYOUTS = [
    ("square_rgb", 2, (3, 3), 14),
    ("square_rgb", 2, (3, 3), 16),
    ("square_bgr", None, (3, 3), 16),
    ("square_bgr", 2, (0, 0), None),
    ("test_landscape", 2, (3, 3), None),
    ("test_landscape", None, (0, 0), None),
    ("test_portrait", 2, (3, 3), 14),
]


def _inputs(batch):
    """(videos on the GPU, samples, boxes, mean, std, reverse) of a batch, from the recorded seeds."""
    z, cases = rec.recording()
    names = BATCHES[batch]
    videos = [torch.from_numpy(rec.clip_of(cases[n]).copy()).cuda() for n in names]
    samples = [(torch.arange(N_FAST), rec.replay(n)[0]) for n in names]
    boxes = [rec.replay(n)[1] for n in names]
    bgr = {cases[n]["bgr"] for n in names}
    assert len(bgr) == 1
    return videos, samples, boxes, z["mean"].tolist(), z["std"].tolist(), not bgr.pop()


@functools.lru_cache(maxsize=None)
def _run(batch, alpha, pad, wp):
    """gpu_detection_batch on a batch, computed once per layout and left unchanged: (packed clips, bboxes, C-ABI calls)."""
    import sfhip
    from slowfast.datasets import utils as ds
    videos, samples, boxes, mean, std, reverse = _inputs(batch)
    calls = sfhip.CALLS
    packed, bboxes = ds.gpu_detection_batch(videos, samples, boxes, mean, std, alpha, reverse_input_channel=reverse,
                                            pad=pad, wp=wp)
    torch.cuda.synchronize()
    return packed, bboxes, sfhip.CALLS - calls


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _guarded(shape):
    """A NaN-filled buffer of `shape` between two sentinel margins -> (whole allocation, the buffer's view)."""
    n = int(np.prod(shape))
    whole = torch.full((MARGIN + n + MARGIN,), SENTINEL, dtype=torch.float32, device="cuda")
    whole[MARGIN:MARGIN + n] = float("nan")
    return whole, whole[MARGIN:MARGIN + n].view(shape)


def _margins_intact(whole):
    return bool((whole[:MARGIN] == SENTINEL).all()) and bool((whole[-MARGIN:] == SENTINEL).all())


def _borders_are_zero(buf, win_h, win_w, ph, pw):
    assert buf.shape[2] == win_h + 2 * ph and buf.shape[3] >= win_w + 2 * pw
    parts = [buf[:, :, :ph], buf[:, :, ph + win_h:], buf[:, :, :, :pw], buf[:, :, :, pw + win_w:], buf[..., 3]]
    return all(p.numel() == 0 or bool((p.contiguous().view(torch.int32) == 0).all()) for p in parts)  # +0.0 exactly


@pytest.mark.parametrize("name", sorted(BATCH_OF))
def test_pixels_against_the_float64_recording(name):
    """Every recorded case, inside its batch, against the reference's float64 run.  The bound is the project's form:
    max(1e-6, 4 x the reference's own float32-vs-float64 error on that case) — the reference's float32 run forms the
    bilinear source coordinate in float32 as the kernel does, so its error carries what the number formats cost on
    this very input.  Figures: DESIGN.md, "Detection input step"."""
    z, _ = rec.recording()
    batch = BATCH_OF[name]
    b = BATCHES[batch].index(name)
    packed, _, calls = _run(batch, 2, (3, 3), None)
    assert calls == 1 and len(packed) == 2
    slow, fast = packed
    want = rec.imgs64(name)                                       # [C, T, win_h, win_w]
    ref_err = float(np.abs(z[name + "/imgs"].astype(np.float64) - want).max())
    bound = max(1e-6, 4.0 * ref_err)
    assert fast.shape == (len(BATCHES[batch]), 3, N_FAST) + want.shape[2:]
    got = fast.to_ncthw()[b].cpu().double().numpy()
    err = float(np.abs(got - want).max())
    print("%s: kernel vs float64 %.3e, reference float32 vs float64 %.3e, bound %.3e" % (name, err, ref_err, bound))
    assert err <= bound, (name, err, bound)
    got_slow = slow.to_ncthw()[b].cpu().double().numpy()
    assert float(np.abs(got_slow - want[:, [0, 3]]).max()) <= bound  # slow_frame_indices(4, 2) = [0, 3]


@pytest.mark.parametrize("batch,alpha,pad,wp", LAYOUTS)
def test_layout_zeros_margins_and_slow_frames(batch, alpha, pad, wp):
    import sfhip
    from slowfast.datasets import utils as ds
    ph, pw = pad
    packed, _, calls = _run(batch, alpha, pad, wp)
    assert calls == 1 and len(packed) == (1 if alpha is None else 2)  # one table upload, one launch
    fast_p = packed[-1]
    win_h, win_w = fast_p.H, fast_p.W
    B = len(BATCHES[batch])
    assert fast_p.buf.shape == (B, N_FAST, win_h + 2 * ph, win_w + 2 * pw if wp is None else wp, 4)
    assert (fast_p.ph, fast_p.pw, fast_p.C) == (ph, pw, 3)
    # the same launch into NaN-filled buffers inside sentinel-filled allocations: every element written, none beside
    videos, samples, boxes, mean, std, reverse = _inputs(batch)
    slow_idx = ds.slow_frame_indices(N_FAST, alpha) if alpha is not None else torch.zeros(0, dtype=torch.long)
    n_slow = slow_idx.numel()
    shape = tuple(fast_p.buf.shape)
    fast_all, fast = _guarded(shape)
    slow_all, slow = _guarded((B, n_slow) + shape[2:]) if n_slow else (None, None)
    table_host = ds.det_table(videos, samples, slow_idx)
    sfhip.clip_batch_det(table_host, table_host.cuda(), n_slow, (win_h, win_w), mean, std, fast, slow, reverse=reverse,
                         ph=ph, pw=pw)
    torch.cuda.synchronize()
    assert _margins_intact(fast_all) and (slow_all is None or _margins_intact(slow_all))
    assert not bool(torch.isnan(fast).any()) and (slow is None or not bool(torch.isnan(slow).any()))
    assert _same_bits(fast, fast_p.buf) and (slow is None or _same_bits(slow, packed[0].buf))
    assert _borders_are_zero(fast, win_h, win_w, ph, pw) and (slow is None or _borders_are_zero(slow, win_h, win_w, ph, pw))
    assert bool((fast[:, :, ph:ph + win_h, pw:pw + win_w, :3] != 0).any())
    if slow is not None:  # Slow frame j holds the bits of Fast frame slow_frame_indices(4, 2)[j] = (0, 3)[j]
        assert slow_idx.tolist() == [0, 3]
        assert _same_bits(slow[:, 0], fast[:, 0]) and _same_bits(slow[:, 1], fast[:, 3])
        assert not _same_bits(fast[:, 0], fast[:, 3])


def test_geometry_does_not_change_the_pixels():
    """The window's values are the same bits whatever the pad and the pitch."""
    a = _run("square_rgb", 2, (3, 3), 14)[0]
    b = _run("square_rgb", 2, (3, 3), 16)[0]
    c = _run("square_rgb", 2, (3, 3), None)[0]
    for x, y in ((a, b), (a, c)):
        assert _same_bits(x[0].to_ncthw(), y[0].to_ncthw()) and _same_bits(x[1].to_ncthw(), y[1].to_ncthw())


def test_channel_reversal_is_a_permutation_of_the_same_bits():
    """AVA.BGR either way on one batch: the stored channels are each other's mirror, bit for bit."""
    from slowfast.datasets import utils as ds
    videos, samples, boxes, mean, std, _ = _inputs("square_rgb")
    (s0, f0), _ = ds.gpu_detection_batch(videos, samples, boxes, mean, std, 2, reverse_input_channel=False, pad=(3, 3))
    (s1, f1), _ = ds.gpu_detection_batch(videos, samples, boxes, mean, std, 2, reverse_input_channel=True, pad=(3, 3))
    torch.cuda.synchronize()
    assert _same_bits(f0.to_ncthw(), f1.to_ncthw().flip(1)) and _same_bits(s0.to_ncthw(), s1.to_ncthw().flip(1))
    assert not _same_bits(f0.to_ncthw(), f1.to_ncthw())


def test_a_device_row_that_fails_the_check_writes_zeros():
    """The host copy is valid, the device copy of clip 1's row is not (a negative crop offset; a zero address; a window
    past the scaled frame): the kernel's own check turns that clip into zeros — it reads nothing for it — and leaves
    the other clips as they were.  A device frame index past the span is clamped."""
    import sfhip
    from slowfast.datasets import utils as ds
    packed, _, _ = _run("square_rgb", 2, (3, 3), 14)
    videos, samples, boxes, mean, std, reverse = _inputs("square_rgb")
    slow_idx = ds.slow_frame_indices(N_FAST, 2)
    table_host = ds.det_table(videos, samples, slow_idx)
    p1 = samples[1][1]
    for col, val in ((6, -1), (0, 0), (7, p1.new_w - 8 + 1)):  # y0; the clip's address; x0 + 8 > new_w
        table = table_host.clone()
        table[ds.DET_ROW * 1 + col] = val
        fast = torch.full_like(packed[1].buf, float("nan"))
        slow = torch.full_like(packed[0].buf, float("nan"))
        sfhip.clip_batch_det(table_host, table.cuda(), 2, (8, 8), mean, std, fast, slow, reverse=reverse, ph=3, pw=3)
        torch.cuda.synchronize()
        for got, ref in ((fast, packed[1].buf), (slow, packed[0].buf)):
            assert bool((got[1].contiguous().view(torch.int32) == 0).all()), (col, "the corrupted clip is zeros")
            assert _same_bits(got[0], ref[0]) and _same_bits(got[2:], ref[2:]), (col, "the others are unchanged")
    table = table_host.clone()
    fi = ds.DET_ROW * len(videos)
    table[fi + 3] = 99    # clip 0, Fast frame 3: past the span -> frame T - 1 = 3, what it was
    table[fi + 4] = -7    # clip 1, Fast frame 0: before it -> frame 0, what it was
    fast = torch.full_like(packed[1].buf, float("nan"))
    slow = torch.full_like(packed[0].buf, float("nan"))
    sfhip.clip_batch_det(table_host, table.cuda(), 2, (8, 8), mean, std, fast, slow, reverse=reverse, ph=3, pw=3)
    torch.cuda.synchronize()
    assert _same_bits(fast, packed[1].buf) and _same_bits(slow, packed[0].buf)


def test_bboxes_equal_detection_collate_bitwise():
    """The returned boxes are the reference's `detection_collate` tensor (recorded from its loader), float32 [K, 5], bit
    for bit, and live in the table's one upload."""
    names, want, _, _ = rec.collated()
    assert names == BATCHES["square_rgb"]
    _, bboxes, calls = _run("square_rgb", 2, (3, 3), 14)
    assert calls == 1 and bboxes.is_cuda and bboxes.dtype == torch.float32 and tuple(bboxes.shape) == want.shape == (50, 5)
    assert np.array_equal(bboxes.cpu().numpy().view(np.int32), want.view(np.int32))
    # a view of the uploaded int64 table: behind 5 rows of 12, 5 x 4 frame indices and 2 Slow positions
    assert bboxes.storage_offset() == 2 * (5 * 12 + 5 * N_FAST + 2) and bboxes.is_contiguous()
    assert bboxes.untyped_storage().nbytes() == 8 * (5 * 12 + 5 * N_FAST + 2) + 4 * 250
    assert [int(v) for v in bboxes[:, 0].cpu().tolist()] == [i for i in range(5) for _ in range(10)]


def test_detection_model_takes_the_packed_clips():
    """The smallest detection model tests/test_detection_gpu.py builds (slow_r50_ava_s64: the Slow-only ResNet with the
    RoI head, 4 frames of 64 x 64) on a square train window: the packed clips and boxes of gpu_detection_batch give the
    bits their to_ncthw() tensors give.  The window is 64 x 64, the size the model's fixtures run at — the network's
    stride leaves nothing of the recording's 8 x 8 frames — so the clips and decisions are drawn here."""
    from _util import load_case, seeded_state_dict
    from slowfast.config.defaults import get_cfg
    from slowfast.datasets import utils as ds
    from slowfast.models import build_model
    z, meta = load_case("slow_r50_ava_s64")
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    cfg.AVA.IMG_PROC_BACKEND = "pytorch"
    cfg.DATA.TRAIN_JITTER_SCALES = [72, 88]
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    model.load_state_dict(seeded_state_dict(z["sd_keys"], z["sd_shapes"], meta["param_seed"]), strict=True)
    model.eval()
    rs = np.random.RandomState(31)
    spans = [(9, 80, 104), (6, 96, 72)]
    videos = [torch.from_numpy(rs.randint(0, 256, (t, h, w, 3)).astype(np.uint8)).cuda() for t, h, w in spans]
    np.random.seed(17)
    params = [ds.det_clip_params(cfg, "train", h, w) for _, h, w in spans]
    assert all((p.win_h, p.win_w) == (64, 64) for p in params)
    half = cfg.DATA.NUM_FRAMES * 2 // 2  # a sampling rate of 2 around the key frame
    samples = [(torch.tensor(ds.det_sequence(c, half, 2, t)), p) for c, (t, _, _), p in zip((4, 1), spans, params)]
    assert all(len(f) == cfg.DATA.NUM_FRAMES for f, _ in samples)
    boxes01 = rec.recording()[0]["boxes01"][:4]
    boxes = [ds.det_boxes(boxes01, h, w, p) for (_, h, w), p in zip(spans, params)]
    ph, pw, wp = ds.stem_input_geometry(model, 64)
    packed, bboxes = ds.gpu_detection_batch(videos, samples, boxes, cfg.DATA.MEAN, cfg.DATA.STD, None,
                                            reverse_input_channel=not cfg.AVA.BGR, pad=(ph, pw), wp=wp)
    assert len(packed) == 1 and packed[0].shape == (2, 3, cfg.DATA.NUM_FRAMES, 64, 64) and tuple(bboxes.shape) == (8, 5)
    with torch.no_grad():
        got = model(packed, bboxes)
        want = model([p.to_ncthw() for p in packed], bboxes.clone())
    torch.cuda.synchronize()
    assert tuple(got.shape) == (8, cfg.MODEL.NUM_CLASSES) and bool(torch.isfinite(got).all())
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 and float(got.std()) > 0
    assert _same_bits(got, want)
