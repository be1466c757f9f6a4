"""Mixup / CutMix inside the one-launch training input step (datasets.utils.gpu_train_batch_mix -> sf_clip_batch_mix /
sf_clip_batch_mix_gray) against the unmixed batch the existing gpu_train_batch writes, mixed afterwards with separate
torch operations: equal bits — the pixel arithmetic is the existing device function, the mix two rounded products and a
rounded sum, never an fma — for both pathways, with owned-memory margins, zero borders and the device-side row check."""
import functools

import numpy as np
import pytest
import torch

import _mix_ref as ref

pytestmark = pytest.mark.gpu

B, CROP, N_FAST, ALPHA, PAD = 3, 12, 4, 2, (1, 3)
SPANS = [(5, 20, 28), (4, 24, 18), (6, 16, 16)]  # (T_i, H_i, W_i): every clip its own allocation and size
MEAN3, STD3 = [0.45, 0.40, 0.50], [0.225, 0.25, 0.2]
SENTINEL, MARGIN = 12345.0, 64
PARTNER = (2, 1, 0)  # B - 1 - b: clip 1 is its own partner
BOXES = {"interior": (3, 2, 9, 7), "two_edges": (0, 5, 6, 12), "empty": (4, 4, 4, 9), "full": (0, 0, 12, 12)}


def _ds():
    from slowfast.datasets import utils
    return utils


def _samples(ds):
    """Clip 0: resampled (20 x 28 -> 15 x 21).  Clip 1: not resampled, flipped, a repeated frame.  Clip 2: resampled
    (16 x 16 -> 13 x 13), the crop against the left edge."""
    return [(torch.tensor([0, 1, 3, 4]), ds.SpatialParams(15, 21, 2, 5, False, CROP)),
            (torch.tensor([2, 2, 3, 0]), ds.SpatialParams(24, 18, 10, 4, True, CROP)),
            (torch.tensor([5, 0, 3, 3]), ds.SpatialParams(13, 13, 1, 0, False, CROP))]


@functools.lru_cache(maxsize=None)
def _unmixed(gray, wp):
    """The parent's route, computed once per layout and left unchanged: gpu_train_batch on the same spans."""
    ds = _ds()
    rs = np.random.RandomState(17)
    videos = [torch.from_numpy(rs.randint(0, 256, (t, h, w) if gray else (t, h, w, 3)).astype(np.uint8)).cuda()
              for t, h, w in SPANS]
    samples = _samples(ds)
    mean, std = ([0.45], [0.225]) if gray else (MEAN3, STD3)
    slow, fast = ds.gpu_train_batch(videos, samples, mean, std, ALPHA, pad=PAD, wp=wp)
    torch.cuda.synchronize()
    return videos, samples, mean, std, slow.buf, fast.buf


def _guarded(shape):
    n = int(np.prod(shape))
    whole = torch.full((MARGIN + n + MARGIN,), SENTINEL, dtype=torch.float32, device="cuda")
    whole[MARGIN:MARGIN + n] = float("nan")
    return whole, whole[MARGIN:MARGIN + n].view(shape)


def _margins_intact(whole):
    return bool((whole[:MARGIN] == SENTINEL).all()) and bool((whole[-MARGIN:] == SENTINEL).all())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _borders_are_zero(buf, rgb):
    ph, pw = PAD
    parts = [buf[:, :, :ph], buf[:, :, ph + CROP:], buf[:, :, :, :pw], buf[:, :, :, pw + CROP:]]
    if rgb:
        parts.append(buf[..., 3])  # the pad channel
    return all(p.numel() == 0 or bool((p.contiguous().view(torch.int32) == 0).all()) for p in parts)  # +0.0 exactly


def _mixed_by_torch(x, rows):
    """What the rows ask for, from the unmixed buffer x [B, T, Hp, Wp, C] with separate torch operations per clip."""
    ph, pw = PAD
    out = []
    for b in range(B):
        p, mode = int(rows[b, 0]), int(rows[b, 1])
        if mode == 1:
            lam_t = torch.tensor(ref.lam_of(rows[b, 2]), dtype=torch.float32, device="cuda")
            own = lam_t * x[b]
            other = (1 - lam_t) * x[p]
            out.append(own + other)
        elif mode == 2:
            y0, x0, y1, x1 = (int(v) for v in rows[b, 3:7])
            mask = torch.zeros(x.shape[2:4], dtype=torch.bool, device="cuda")
            mask[ph + y0:ph + y1, pw + x0:pw + x1] = True
            out.append(torch.where(mask[None, :, :, None], x[p], x[b]))
        else:
            out.append(x[b].clone())
    return torch.stack(out)


def _launch(gray, wp, rows, dev_rows=None):
    """One sf_clip_batch_mix launch into NaN-filled buffers inside sentinel-filled allocations -> (slow, fast)."""
    import sfhip
    ds = _ds()
    videos, samples, mean, std, slow_ref, fast_ref = _unmixed(gray, wp)
    slow_idx = ds.slow_frame_indices(N_FAST, ALPHA)
    host_rows = torch.from_numpy(np.ascontiguousarray(rows))
    table_host = torch.cat([ds.batch_table(videos, samples, slow_idx), host_rows.flatten()]).contiguous()
    table = table_host.clone()
    if dev_rows is not None:
        table[-B * 7:] = torch.from_numpy(np.ascontiguousarray(dev_rows)).flatten()
    fast_all, fast = _guarded(tuple(fast_ref.shape))
    slow_all, slow = _guarded(tuple(slow_ref.shape))
    sfhip.clip_batch_mix(table_host, table.cuda(), slow_idx.numel(), CROP, mean, std, fast, slow, gray=gray,
                         ph=PAD[0], pw=PAD[1])
    torch.cuda.synchronize()
    assert _margins_intact(fast_all) and _margins_intact(slow_all)
    assert not bool(torch.isnan(fast).any()) and not bool(torch.isnan(slow).any())  # every element written
    assert _borders_are_zero(fast, not gray) and _borders_are_zero(slow, not gray)
    return slow, fast


def _check(gray, wp, rows):
    _, _, _, _, slow_ref, fast_ref = _unmixed(gray, wp)
    slow, fast = _launch(gray, wp, rows)
    assert _same_bits(fast, _mixed_by_torch(fast_ref, rows))
    assert _same_bits(slow, _mixed_by_torch(slow_ref, rows))
    assert _same_bits(slow[:, 0], fast[:, 0]) and _same_bits(slow[:, 1], fast[:, 3])  # slow_frame_indices(4, 2) = [0, 3]
    # the numpy restatement says the same
    assert np.array_equal(fast.cpu().numpy().view(np.int32),
                          ref.mix_batch(fast_ref.cpu().numpy(), rows, CROP, *PAD).view(np.int32))
    return slow, fast


def test_mode_0_is_gpu_train_batch_bit_for_bit():
    import sfhip
    ds = _ds()
    videos, samples, mean, std, slow_ref, fast_ref = _unmixed(False, None)
    mix = ds.MixParams(PARTNER, ds.MIX_NONE, 1.0, (0, 0, 0, 0))
    calls = sfhip.CALLS
    (slow, fast), rows = ds.gpu_train_batch_mix(videos, samples, mix, mean, std, ALPHA, pad=PAD)
    assert sfhip.CALLS == calls + 1  # one launch
    torch.cuda.synchronize()
    assert _same_bits(fast.buf, fast_ref) and _same_bits(slow.buf, slow_ref)
    assert fast.shape == (B, 3, N_FAST, CROP, CROP) and (fast.ph, fast.pw) == PAD and fast.Wp == CROP + 2 * PAD[1]
    # the returned rows: a device view of the uploaded table, equal to the host rows
    assert rows.is_cuda and rows.dtype == torch.int64 and tuple(rows.shape) == (B, 7)
    assert torch.equal(rows.cpu(), ds.mix_rows(mix)) and torch.equal(rows.mix_host, ds.mix_rows(mix))
    _check(False, None, ds.mix_rows(mix).numpy())


@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_mode_1_is_the_float32_mix_of_the_unmixed_outputs(lam):
    ds = _ds()
    videos, samples, mean, std, slow_ref, fast_ref = _unmixed(False, None)
    mix = ds.MixParams(PARTNER, ds.MIX_MIXUP, lam, (0, 0, 0, 0))
    (slow, fast), rows = ds.gpu_train_batch_mix(videos, samples, mix, mean, std, ALPHA, pad=PAD)
    torch.cuda.synchronize()
    host = ds.mix_rows(mix)
    assert torch.equal(rows.cpu(), host)
    lam_t = torch.tensor(np.float32(lam), device="cuda")
    partner = torch.tensor(PARTNER, device="cuda")
    for got, x in ((fast.buf, fast_ref), (slow.buf, slow_ref)):
        first = lam_t * x
        second = (1 - lam_t) * x[partner]
        assert _same_bits(got, first + second)
    slow, fast = _check(False, None, host.numpy())
    if lam == 0.3:
        assert not _same_bits(fast[0], fast_ref[0]) and not _same_bits(fast[0], fast_ref[2])
        assert _same_bits(fast[1], (lam_t * fast_ref[1]) + ((1 - lam_t) * fast_ref[1]))  # clip 1 mixes with itself


@pytest.mark.parametrize("box", sorted(BOXES))
def test_mode_2_is_torch_where_on_the_unmixed_outputs(box):
    ds = _ds()
    y0, x0, y1, x1 = BOXES[box]
    lam = 1.0 - (y1 - y0) * (x1 - x0) / float(CROP * CROP)
    rows = ds.mix_rows(ds.MixParams(PARTNER, ds.MIX_CUTMIX, lam, BOXES[box])).numpy()
    slow, fast = _check(False, None, rows)
    _, _, _, _, slow_ref, fast_ref = _unmixed(False, None)
    ph, pw = PAD
    if box == "empty":
        assert _same_bits(fast, fast_ref) and _same_bits(slow, slow_ref)
    elif box == "full":
        assert _same_bits(fast, fast_ref[list(PARTNER)]) and _same_bits(slow, slow_ref[list(PARTNER)])
    else:
        inside = fast[0, :, ph + y0:ph + y1, pw + x0:pw + x1]
        assert _same_bits(inside, fast_ref[2, :, ph + y0:ph + y1, pw + x0:pw + x1])  # every frame, the partner's pixels
        assert _same_bits(fast[0, :, ph + y1:], fast_ref[0, :, ph + y1:])
        assert not _same_bits(fast[0], fast_ref[0])


@pytest.mark.parametrize("wp", [20, 18], ids=["four_pixels_per_store", "one_pixel_per_store"])
def test_gray_clips_with_a_mode_per_row(wp):
    """One-channel clips at both store widths (Wp % 4 == 0, and not), the three modes side by side in one batch."""
    rows = ref.make_rows(PARTNER, [1, 2, 2], [0.3, 0.75, 0.5], [(0, 0, 0, 0), (3, 2, 9, 8), (0, 5, 6, 12)])
    slow, fast = _check(True, wp, rows)
    _, _, _, _, slow_ref, fast_ref = _unmixed(True, wp)
    assert fast.shape[3] == wp and fast.shape[4] == 1
    assert _same_bits(fast[1], fast_ref[1])  # clip 1 is its own partner: CutMix changes nothing
    assert not _same_bits(fast[0], fast_ref[0]) and not _same_bits(fast[2], fast_ref[2])
    rows0 = ref.make_rows(PARTNER, 0, 1.0)
    slow, fast = _check(True, wp, rows0)
    assert _same_bits(fast, fast_ref) and _same_bits(slow, slow_ref)


@pytest.mark.parametrize("gray", [False, True], ids=["rgb", "gray"])
def test_a_device_row_that_fails_the_check_writes_zeros(gray):
    """The host rows are valid, the device copy of clip 0's mix row is not: that clip is zeros — nothing is read for it —
    and the others are what they were."""
    wp = 20 if gray else None
    rows = ref.make_rows(PARTNER, 1, 0.3)
    want = _check(gray, wp, rows)
    for col, val in ((0, 3), (0, -1), (1, 5), (2, ref.lam_bits(2.0)), (5, CROP + 1), (4, -2)):
        dev = rows.copy()
        dev[0, col] = val
        for got, ok in zip(_launch(gray, wp, rows, dev_rows=dev), want):
            assert bool((got[0].contiguous().view(torch.int32) == 0).all()), (col, val)
            assert _same_bits(got[1], ok[1]) and _same_bits(got[2], ok[2]), (col, val)
