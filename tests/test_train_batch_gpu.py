"""The training input step on the GPU: one launch for the whole batch (datasets.utils.gpu_train_batch -> sf_clip_batch /
sf_clip_batch_gray) against the existing route (index_select of the sampled frames, then gpu_input_step: one
sf_clip_prologue launch per clip and pathway) — equal bits, because the pixel arithmetic is one device function — with
owned-memory margins, the device-side row check, and float64 parity of the whole step."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CROP, N_FAST = 8, 4
SPANS = [(5, 20, 28), (8, 24, 24), (6, 30, 22)]  # (T_i, H_i, W_i): every clip its own allocation and size
MEAN3, STD3 = [0.45, 0.40, 0.50], [0.225, 0.25, 0.2]
SENTINEL, MARGIN = 12345.0, 64  # floats either side of each output buffer (256 B: the buffers stay 16-byte aligned)

# name: (gray, alpha, reverse, (ph, pw), Wp).  Wp 14: rows of 14 floats, no 16-byte store for a one-channel clip (one
# pixel per store); Wp 16 and 8: four pixels per store.
CASES = {
    "rgb_a2_pitch14": (False, 2, False, (3, 3), 14),
    "rgb_a2_reverse_pitch16": (False, 2, True, (3, 3), 16),
    "rgb_single_pathway_nopad": (False, None, False, (0, 0), None),
    "rgb_single_pathway_reverse_pad": (False, None, True, (3, 3), 16),
    "gray_a2_scalar_pitch14": (True, 2, False, (3, 3), 14),
    "gray_a2_vec_pitch16": (True, 2, False, (3, 3), 16),
    "gray_single_pathway_nopad": (True, None, False, (0, 0), None),
}


def _samples(ds):
    """Clip 0: resampled (20 x 28 -> 12 x 16).  Clip 1: (new_h, new_w) == (H, W), the no-resample branch, flipped,
    with repeated frame indices.  Clip 2: portrait, resampled (30 x 22 -> 13 x 9), the crop against the right edge."""
    return [(torch.tensor([0, 1, 3, 4]), ds.SpatialParams(12, 16, 3, 5, False, CROP)),
            (torch.tensor([2, 2, 7, 7]), ds.SpatialParams(24, 24, 16, 5, True, CROP)),
            (torch.tensor([5, 0, 3, 3]), ds.SpatialParams(13, 9, 5, 1, False, CROP))]


def _videos(gray, seed=11):
    rs = np.random.RandomState(seed)
    return [torch.from_numpy(rs.randint(0, 256, (t, h, w) if gray else (t, h, w, 3)).astype(np.uint8)).cuda()
            for t, h, w in SPANS]


@functools.lru_cache(maxsize=None)
def _existing_route(name):
    """The parent's route, computed once per case and left unchanged: gather each clip's frames, then gpu_input_step."""
    from slowfast.datasets import utils as ds
    gray, alpha, reverse, pad, wp = CASES[name]
    videos, samples = _videos(gray), _samples(ds)
    mean, std = ([0.45], [0.225]) if gray else (MEAN3, STD3)
    clips = [v.index_select(0, f.cuda()).contiguous() for v, (f, _) in zip(videos, samples)]
    packed = ds.gpu_input_step(clips, [p for _, p in samples], mean, std, alpha, reverse_input_channel=reverse, pad=pad,
                               wp=wp)
    torch.cuda.synchronize()
    return videos, samples, mean, std, packed


def _guarded(shape):
    """A NaN-filled buffer of `shape` between two sentinel margins -> (whole allocation, the buffer's view)."""
    n = int(np.prod(shape))
    whole = torch.full((MARGIN + n + MARGIN,), SENTINEL, dtype=torch.float32, device="cuda")
    whole[MARGIN:MARGIN + n] = float("nan")
    return whole, whole[MARGIN:MARGIN + n].view(shape)


def _margins_intact(whole):
    return bool((whole[:MARGIN] == SENTINEL).all()) and bool((whole[-MARGIN:] == SENTINEL).all())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _borders_are_zero(buf, ph, pw, rgb):
    hp, wp = buf.shape[2], buf.shape[3]
    parts = [buf[:, :, :ph], buf[:, :, ph + CROP:], buf[:, :, :, :pw], buf[:, :, :, pw + CROP:]]
    if rgb:
        parts.append(buf[..., 3])  # the pad channel
    assert hp == CROP + 2 * ph and wp >= CROP + 2 * pw
    return all(p.numel() == 0 or bool((p.contiguous().view(torch.int32) == 0).all()) for p in parts)  # +0.0 exactly


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_launch_equals_the_per_clip_route_bitwise(name):
    import sfhip
    from slowfast.datasets import utils as ds
    gray, alpha, reverse, (ph, pw), wp = CASES[name]
    videos, samples, mean, std, want = _existing_route(name)
    # the dataset-level call: one table upload, one launch
    calls = sfhip.CALLS
    got = ds.gpu_train_batch(videos, samples, mean, std, alpha, reverse_input_channel=reverse, pad=(ph, pw), wp=wp)
    assert sfhip.CALLS == calls + 1
    torch.cuda.synchronize()
    assert len(got) == len(want) == (1 if alpha is None else 2)
    for g, w in zip(got, want):
        assert g.buf.shape == w.buf.shape and g.shape == w.shape and (g.ph, g.pw) == (w.ph, w.pw)
        assert _same_bits(g.buf, w.buf), name
    assert got[-1].shape == (3, 1 if gray else 3, N_FAST, CROP, CROP)
    # the same launch into NaN-filled buffers inside sentinel-filled allocations: every element written, none beside
    slow_idx = ds.slow_frame_indices(N_FAST, alpha) if alpha is not None else torch.zeros(0, dtype=torch.long)
    n_slow = slow_idx.numel()
    shape = tuple(want[-1].buf.shape)
    fast_all, fast = _guarded(shape)
    slow_all, slow = _guarded((3, n_slow) + shape[2:]) if n_slow else (None, None)
    table_host = ds.batch_table(videos, samples, slow_idx)
    sfhip.clip_batch(table_host, table_host.cuda(), n_slow, CROP, mean, std, fast, slow, gray=gray, reverse=reverse,
                     ph=ph, pw=pw)
    torch.cuda.synchronize()
    assert _margins_intact(fast_all) and (slow_all is None or _margins_intact(slow_all))
    assert not bool(torch.isnan(fast).any()) and (slow is None or not bool(torch.isnan(slow).any()))
    assert _same_bits(fast, want[-1].buf) and (slow is None or _same_bits(slow, want[0].buf))
    assert _borders_are_zero(fast, ph, pw, not gray) and (slow is None or _borders_are_zero(slow, ph, pw, not gray))
    assert bool((fast[:, :, ph:ph + CROP, pw:pw + CROP, :1 if gray else 3] != 0).any())


def test_repeated_indices_and_the_slow_positions():
    """Clip 1 takes frames [2, 2, 7, 7]: its Fast frames 0 / 1 and 2 / 3 hold the same bits; slow_frame_indices(4, 2) =
    [0, 3], so Slow frame j is Fast frame (0, 3)[j] of every clip."""
    from slowfast.datasets import utils as ds
    videos, samples, mean, std, _ = _existing_route("rgb_a2_pitch14")
    slow, fast = ds.gpu_train_batch(videos, samples, mean, std, 2, pad=(3, 3), wp=14)
    assert _same_bits(fast.buf[1, 0], fast.buf[1, 1]) and _same_bits(fast.buf[1, 2], fast.buf[1, 3])
    assert not _same_bits(fast.buf[1, 1], fast.buf[1, 2])
    assert _same_bits(slow.buf[:, 0], fast.buf[:, 0]) and _same_bits(slow.buf[:, 1], fast.buf[:, 3])


@pytest.mark.parametrize("name", ["rgb_a2_pitch14", "gray_a2_vec_pitch16"])
def test_a_device_row_that_fails_the_check_writes_zeros(name):
    """The host copy is valid, the device copy of clip 1's row is not (a negative crop offset; a zero address): the
    kernel's own check turns that clip into zeros — it reads nothing for it — and leaves the other clips as they were."""
    import sfhip
    from slowfast.datasets import utils as ds
    gray, alpha, reverse, (ph, pw), wp = CASES[name]
    videos, samples, mean, std, want = _existing_route(name)
    slow_idx = ds.slow_frame_indices(N_FAST, alpha)
    table_host = ds.batch_table(videos, samples, slow_idx)
    for col, val in ((6, -1), (0, 0)):  # y0, the clip's address
        table = table_host.clone()
        table[ds.BATCH_ROW * 1 + col] = val
        fast = torch.full_like(want[1].buf, float("nan"))
        slow = torch.full_like(want[0].buf, float("nan"))
        sfhip.clip_batch(table_host, table.cuda(), slow_idx.numel(), CROP, mean, std, fast, slow, gray=gray,
                         reverse=reverse, ph=ph, pw=pw)
        torch.cuda.synchronize()
        for got, ref in ((fast, want[1].buf), (slow, want[0].buf)):
            assert bool((got[1].contiguous().view(torch.int32) == 0).all()), (col, "the corrupted clip is zeros")
            assert _same_bits(got[0], ref[0]) and _same_bits(got[2], ref[2]), (col, "the others are unchanged")


def _fp64_reference(videos, samples, mean, std, alpha, reverse):
    """tensor_normalize -> F.interpolate(bilinear, align_corners=False) -> crop -> flip -> pack_pathway_output, on the
    CPU in float64, with the float32 mean / std the kernel is handed.  -> [slow, fast] as [B, C, T, crop, crop]."""
    from slowfast.datasets import utils as ds
    m = torch.tensor(mean, dtype=torch.float32).double()
    s = torch.tensor(std, dtype=torch.float32).double()
    out = []
    for v, (frames, p) in zip(videos, samples):
        x = (v.cpu().index_select(0, frames).double() / 255.0 - m) / s  # [T, H, W, C]
        x = x.permute(0, 3, 1, 2)                                        # bilinear acts per (frame, channel) plane
        if (p.new_h, p.new_w) != tuple(x.shape[2:]):
            x = torch.nn.functional.interpolate(x, size=(p.new_h, p.new_w), mode="bilinear", align_corners=False)
        x = x[:, :, p.y:p.y + p.crop, p.x:p.x + p.crop]
        if p.flip:
            x = x.flip(-1)
        out.append(ds.pack_pathway_output(ds.PathwayCfg(alpha, reverse), x.permute(1, 0, 2, 3)))  # of C x T x H x W
    return [torch.stack(path) for path in zip(*out)]


def test_fp64_parity_of_the_whole_step():
    """One case against the float64 restatement, under the bound tests/test_input_step.py sets for gpu_input_step
    (max abs error < 2e-6).

    That bound was set against a float32 reference, which forms the bilinear source coordinate scale * (dst + 0.5) -
    0.5 in float32 exactly as the kernel does.  A float64 reference forms it in float64, and for a general scale the
    two coordinates differ by up to half a float32 ulp of a coordinate below 32 (about 1e-6), which the interpolation
    multiplies by the contrast of neighbouring pixels (up to 5 normalised units on uint8 noise): more than the bound
    allows, and a property of the two number formats, not of the kernel.  So this case takes scales whose coordinates
    are exact in both formats — 20 x 28 -> 40 x 56 (0.5: weights 1/4, 3/4, clamped at the edge), 30 x 22 -> 24 x 16
    (1.25 and 1.375: weights in eighths and sixteenths) and one clip that is not resampled — and what remains is what
    the bound was written for: u / 255 (3e-8), the subtraction (3e-8), the division by std >= 0.2 (those two times 5,
    plus half an ulp of 2.5: 4.2e-7 per tap) and the four roundings of the weighted sum (each at most 1.2e-7):
    under 1e-6 in all.  Flip, channel reversal, crop against both edges and the Slow selection are part of the case."""
    from slowfast.datasets import utils as ds
    videos = _videos(False, seed=23)
    samples = [(torch.tensor([0, 1, 3, 4]), ds.SpatialParams(40, 56, 32, 0, False, CROP)),   # bottom-left corner
               (torch.tensor([2, 2, 7, 7]), ds.SpatialParams(24, 24, 16, 5, True, CROP)),
               (torch.tensor([5, 0, 3, 3]), ds.SpatialParams(24, 16, 9, 8, True, CROP))]     # right edge, flipped
    want = _fp64_reference(videos, samples, MEAN3, STD3, 2, True)
    got = ds.gpu_train_batch(videos, samples, MEAN3, STD3, 2, reverse_input_channel=True, pad=(3, 3), wp=14)
    torch.cuda.synchronize()
    assert [tuple(w.shape) for w in want] == [(3, 3, 2, CROP, CROP), (3, 3, N_FAST, CROP, CROP)]
    for name, g, w in zip(("slow", "fast"), got, want):
        e = float((g.to_ncthw().cpu().double() - w).abs().max())
        print("gpu_train_batch vs float64, %s: max abs %.3e" % (name, e))
        assert e < 2e-6, (name, e)
