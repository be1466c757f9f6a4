"""Jester's colour jitter inside the one-launch training input step (datasets.utils.gpu_train_batch_jitter ->
sf_clip_batch_jitter, sf_frame_grey_means) on the GPU.  Every comparison is exact: the frame means against the numpy
restatement of the contract (tests/_jitter_ref.py), the jittered batch against the existing `gpu_train_batch` on spans
jittered on the host with that restatement.  The one comparison with a tolerance is the reference's own [slow, fast]
(tests/golden/jester_jitter.npz), held as tests/test_input_step.py holds the input step to its golden: max abs < 2e-6."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import _jitter_ref as ref
from _util import GOLDEN

pytestmark = pytest.mark.gpu

MEAN3, STD3 = [0.45, 0.40, 0.50], [0.225, 0.25, 0.2]
N_FAST = 4
SKIP = 0.0

# ---------------------------------------------------------------------------------------------------- the frame means
# (T, H, W) of the clips every brightness factor is run over: one pixel, odd pitches (frame bases at every address
# modulo 4: 5 * 7 * 3 = 105 bytes per frame), a square, and a frame that takes each thread through the loop many times
SIZES = [(3, 1, 1), (4, 5, 7), (3, 16, 16), (5, 33, 47), (2, 257, 1031)]
INDICES = [[2, 0, 2, 1], [1, 2, 3, 3], [0, 0, 1, 2], [4, 1, 1, 3], [1, 0, 1, 1]]  # with duplicates


def _two_level(h, w, k, n_high):
    """A grey frame (R = G = B) of value k with its first n_high pixels at k + 1: grey(.) is the value itself."""
    flat = np.full(h * w, k, np.uint8)
    flat[:n_high] = k + 1
    return np.repeat(flat.reshape(h, w, 1), 3, axis=2)


@functools.lru_cache(maxsize=None)
def _mean_clips():
    rs = np.random.RandomState(41)
    sized = [rs.randint(0, 256, (t, h, w, 3)).astype(np.uint8) for t, h, w in SIZES]
    # 4 x 6 = 24 pixels: 12 at k + 1 is k + 1/2 exactly (rounds up), 11 at k + 1 is one pixel short of it (rounds down)
    halves = np.stack([_two_level(4, 6, 100, 12), _two_level(4, 6, 100, 11)])
    white = np.full((2, 5, 6, 3), 255, np.uint8)
    unread = rs.randint(0, 256, (2, 5, 7, 3)).astype(np.uint8)
    return sized, halves, white, unread


@pytest.mark.parametrize("fb", [0.4, 1.0, 1.4, SKIP])
def test_frame_grey_means_equal_the_restatement(fb):
    import sfhip
    from slowfast.datasets import utils as ds
    sized, halves, white, unread = _mean_clips()
    clips = sized + [halves, white, unread]
    indices = INDICES + [[0, 1, 1, 0], [1, 0, 0, 1], [0, 1, 0, 1]]
    jit = [ds.ColorJitter(fb, 1.2, 0.8)] * len(sized) + [ds.ColorJitter(1.0, 0.5, 1.0), ds.ColorJitter(1.4, 0.9, 0.0),
                                                          ds.ColorJitter(1.3, SKIP, 1.3)]
    B = len(clips)
    videos = [torch.from_numpy(c).cuda() for c in clips]
    # the means look at whole frames: any window inside the scaled frame will do for the rows
    samples = [(torch.tensor(i), ds.SpatialParams(c.shape[1], c.shape[2], 0, 0, False, 1)) for i, c in zip(indices, clips)]
    table_host = torch.cat([ds.batch_table(videos, samples, torch.zeros(0, dtype=torch.long)),
                            ds.jitter_rows(jit).flatten()]).contiguous()
    whole = torch.full((16 + B * N_FAST + 16,), -7, dtype=torch.int32, device="cuda")  # every element has one owner
    means = whole[16:16 + B * N_FAST].view(B, N_FAST)
    sfhip.frame_grey_means(table_host, table_host.cuda(), 0, means)
    torch.cuda.synchronize()
    want = [[ref.grey_mean(c[t], j.bright) if j.contrast > 0 else 0 for t in i] for c, i, j in zip(clips, indices, jit)]
    print("frame means, fb %.1f: %s" % (fb, means.cpu().tolist()))
    assert means.cpu().tolist() == want
    assert bool((whole[:16] == -7).all()) and bool((whole[-16:] == -7).all())
    assert want[len(sized)] == [101, 100, 100, 101]      # k + 1/2 rounds up, one pixel short of it rounds down
    assert want[len(sized) + 1] == [255] * 4             # 1.4 * 255 saturates
    assert want[len(sized) + 2] == [0] * 4               # no contrast stage: nothing read, 0 written


# ---------------------------------------------------------------------------------------------------- the batch
# name: (crop, alpha, reverse, (ph, pw), Wp, spans (T, H, W), samples (frame indices, new_h, new_w, y, x, flip)).
# Per shape: clip 0 is scaled down, clip 1 is not resampled ((new_h, new_w) == (H, W)) and flipped, clip 2 is scaled up.
_CROP8 = ([(5, 20, 28), (8, 24, 24), (6, 7, 9)],
          [([0, 1, 3, 4], 12, 16, 3, 5, False), ([2, 2, 7, 7], 24, 24, 16, 5, True), ([5, 0, 3, 3], 14, 18, 5, 9, False)])
_CROP16 = ([(5, 41, 53), (8, 19, 23), (6, 11, 13)],
           [([0, 1, 3, 4], 20, 26, 4, 9, False), ([2, 2, 7, 7], 19, 23, 3, 7, True), ([5, 0, 3, 3], 22, 26, 6, 10, False)])
SHAPES = {
    "crop8_a2_pitch14": (8, 2, False, (3, 3), 14) + _CROP8,
    "crop8_single_reverse": (8, None, True, (0, 0), None) + _CROP8,
    "crop16_a2_reverse_pitch24": (16, 2, True, (3, 3), 24) + _CROP16,
    "crop16_single": (16, None, False, (1, 2), None) + _CROP16,
}
# per factor set: (bright, contrast, color) of clips 0, 1, 2
FACTORS = {
    "below_one": [(0.4, 0.55, 0.7), (0.9, 0.45, 0.6), (0.5, 0.8, 0.95)],
    "above_one": [(1.4, 1.3, 1.25), (1.1, 1.4, 1.35), (1.3, 1.2, 1.4)],
    "one_exactly": [(1.0, 0.8, 1.2), (0.7, 1.0, 1.3), (1.2, 0.6, 1.0)],
    "one_stage_skipped_a": [(SKIP, 1.3, 0.6), (1.3, SKIP, 0.6), (0.6, 1.3, SKIP)],
    "one_stage_skipped_b": [(0.6, 1.3, SKIP), (SKIP, 0.6, 1.3), (1.3, -1.0, 0.6)],
    "one_stage_skipped_c": [(1.3, SKIP, 1.2), (0.6, 1.3, -0.5), (-2.0, 0.7, 1.3)],
    "all_skipped": [(SKIP, SKIP, SKIP), (-1.0, SKIP, -0.25), (SKIP, -3.0, SKIP)],
}


def _spans(shape):
    rs = np.random.RandomState(17)
    return [rs.randint(0, 256, (t, h, w, 3)).astype(np.uint8) for t, h, w in SHAPES[shape][5]]


def _samples(ds, shape):
    crop = SHAPES[shape][0]
    return [(torch.tensor(f), ds.SpatialParams(nh, nw, y, x, flip, crop)) for f, nh, nw, y, x, flip in SHAPES[shape][6]]


@functools.lru_cache(maxsize=None)
def _host_route(shape, factors):
    """The existing route, computed once per case and left unchanged: every span jittered on the host, frame by frame,
    with the numpy restatement; uploaded; `gpu_train_batch`."""
    from slowfast.datasets import utils as ds
    crop, alpha, reverse, pad, wp = SHAPES[shape][:5]
    jittered = [ref.jitter_clip(s, *f) for s, f in zip(_spans(shape), FACTORS[factors])]
    videos = [torch.from_numpy(j).cuda() for j in jittered]
    packed = ds.gpu_train_batch(videos, _samples(ds, shape), MEAN3, STD3, alpha, reverse_input_channel=reverse, pad=pad,
                                wp=wp)
    torch.cuda.synchronize()
    return jittered, packed


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("factors", sorted(FACTORS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_jittered_batch_equals_host_jitter_then_the_existing_step_bitwise(shape, factors):
    import sfhip
    from slowfast.datasets import utils as ds
    crop, alpha, reverse, (ph, pw), wp = SHAPES[shape][:5]
    jittered, want = _host_route(shape, factors)
    spans = _spans(shape)
    videos = [torch.from_numpy(s).cuda() for s in spans]
    jit = [ds.ColorJitter(*f) for f in FACTORS[factors]]
    calls = sfhip.CALLS
    got = ds.gpu_train_batch_jitter(videos, _samples(ds, shape), jit, MEAN3, STD3, alpha, reverse_input_channel=reverse,
                                    pad=(ph, pw), wp=wp)
    assert sfhip.CALLS == calls + 1  # one ABI call (two launches)
    torch.cuda.synchronize()
    assert len(got) == len(want) == (1 if alpha is None else 2)
    for g, w in zip(got, want):  # whole buffers: borders and the pad channel included
        assert g.buf.shape == w.buf.shape and g.shape == w.shape and (g.ph, g.pw) == (w.ph, w.pw)
        assert _same_bits(g.buf, w.buf), (shape, factors)
    assert got[-1].shape == (3, 3, N_FAST, crop, crop)
    if factors == "all_skipped":  # nothing is jittered: gpu_train_batch on the original spans
        assert all(np.array_equal(j, s) for j, s in zip(jittered, spans))
        plain = ds.gpu_train_batch(videos, _samples(ds, shape), MEAN3, STD3, alpha, reverse_input_channel=reverse,
                                   pad=(ph, pw), wp=wp)
        torch.cuda.synchronize()
        assert all(_same_bits(g.buf, p.buf) for g, p in zip(got, plain))
    else:
        assert all(not np.array_equal(j, s) for j, s in zip(jittered, spans))
    if factors == "above_one":  # both ends of the clip are reached
        assert all(j.min() == 0 and j.max() == 255 for j in jittered)


def test_the_reference_golden_pipeline():
    """RandomColorJitter -> tensor_normalize -> spatial_sampling -> pack_pathway_output as the reference ran them,
    against the device output after to_ncthw, under the bound of tests/test_input_step.py (max abs < 2e-6)."""
    from slowfast.datasets import utils as ds
    z = np.load(os.path.join(GOLDEN, "jester_jitter.npz"))
    mean, std = [float(v) for v in z["mean"]], [float(v) for v in z["std"]]
    cases = json.loads(str(z["pipe_cases"]))
    assert len(cases) >= 2
    for c in cases:
        t, h, w = c["thw"]
        clip = torch.from_numpy(z[c["name"] + "/clip"]).cuda()
        np.random.seed(c["seed"])
        p = ds.sample_spatial_params(h, w, spatial_idx=-1, min_scale=c["min_scale"], max_scale=c["max_scale"],
                                     crop_size=c["crop"], random_horizontal_flip=c["flip"],
                                     inverse_uniform_sampling=c["inv"])
        for pad, wp in (((3, 3), None), ((1, 1), c["crop"] + 4)):
            slow, fast = ds.gpu_train_batch_jitter([clip], [(torch.arange(t), p)], [ds.ColorJitter(*c["factors"])], mean,
                                                   std, c["alpha"], reverse_input_channel=c["reverse"], pad=pad, wp=wp)
            torch.cuda.synchronize()
            for name, packed in (("slow", slow), ("fast", fast)):
                want = torch.from_numpy(z[c["name"] + "/" + name])
                got = packed.to_ncthw().cpu()[0]
                assert got.shape == want.shape
                e = float((got - want).abs().max())
                print("%s %s vs the reference: max abs %.3e" % (c["name"], name, e))
                assert e < 2e-6, (c["name"], name, e)


def test_a_device_row_that_fails_the_check_writes_zeros_for_that_clip_only():
    """The host copy is valid, the device copy of clip 1's batch row has a zero address (then: of its jitter row, a NaN
    factor): both launches check the device rows themselves — clip 1 becomes zeros, its means 0, nothing is read for
    it — and the other clips are what they were."""
    import sfhip
    from slowfast.datasets import utils as ds
    shape, factors = "crop8_a2_pitch14", "below_one"
    crop, alpha, reverse, (ph, pw), wp = SHAPES[shape][:5]
    _, want = _host_route(shape, factors)
    videos = [torch.from_numpy(s).cuda() for s in _spans(shape)]
    slow_idx = ds.slow_frame_indices(N_FAST, alpha)
    jit = [ds.ColorJitter(*f) for f in FACTORS[factors]]
    table_host = torch.cat([ds.batch_table(videos, _samples(ds, shape), slow_idx), ds.jitter_rows(jit).flatten()]).contiguous()
    jit0 = 3 * (ds.BATCH_ROW + N_FAST) + slow_idx.numel()
    for pos, val in ((ds.BATCH_ROW * 1 + 0, 0), (jit0 + 3 * 1 + 1, 0x7fc00000)):
        table = table_host.clone()
        table[pos] = val
        means = torch.full((3, N_FAST), -7, dtype=torch.int32, device="cuda")
        fast = torch.full_like(want[1].buf, float("nan"))
        slow = torch.full_like(want[0].buf, float("nan"))
        sfhip.clip_batch_jitter(table_host, table.cuda(), slow_idx.numel(), crop, MEAN3, STD3, means, fast, slow,
                                reverse=reverse, ph=ph, pw=pw)
        torch.cuda.synchronize()
        assert means[1].tolist() == [0] * N_FAST and bool((means[0] > 0).all()) and bool((means[2] > 0).all())
        for got, w in ((fast, want[1].buf), (slow, want[0].buf)):
            assert bool((got[1].contiguous().view(torch.int32) == 0).all()), (pos, "the corrupted clip is zeros")
            assert _same_bits(got[0], w[0]) and _same_bits(got[2], w[2]), (pos, "the others are unchanged")
