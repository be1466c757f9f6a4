"""The per-clip input step of the reference's Kinetics loader (datasets/kinetics.py:230-248) for the MI355X path.

Host side (this file) keeps what must stay on the host: the random draws of `spatial_sampling`
(datasets/utils.py:151-203 -> transform.py) taken from numpy's global RNG in the reference's order, and the slow
pathway's frame indices (`pack_pathway_output`, datasets/utils.py:73-112).  The arithmetic — uint8 -> float
normalise (`tensor_normalize`, :298-315), bilinear short-side scale, crop, flip, frame selection — runs as one HIP
kernel per pathway (`sf_clip_prologue`) that writes the stems' input layout directly, so the decoded clip crosses
PCIe as uint8 once instead of as two float NCTHW tensors.  Whole batches go in one launch for both pathways: the
views of one test video (`test_view_params` -> `gpu_test_views` -> `sf_clip_views`) and the clips of one training
batch, multigrid's short and long cycles included (`train_clip_params` -> `gpu_train_batch` -> `sf_clip_batch`).
The detection (AVA) loader's preprocessing (datasets/ava_dataset.py:233-338, the "pytorch" backend) orders the
arithmetic differently and carries boxes: `det_clip_params` / `det_boxes` -> `gpu_detection_batch` ->
`sf_clip_batch_det`, again one upload and one launch per batch.  The Jester loader colour-jitters every train / val
clip with PIL before normalising (decoder.py:456-469): `jester_clip_params` -> `gpu_train_batch_jitter` ->
`sf_clip_batch_jitter` does that to the uint8 pixels the resampling taps read, bit for bit."""
from slowfast._overlay import chain_module as _chain_module

_chain_module(globals())  # the reference's namesake (when importable) supplies every name not defined below
import collections
import math
import random

import numpy as np
import torch

import sfhip

SpatialParams = collections.namedtuple("SpatialParams", "new_h new_w y x flip crop")
PathwayCfg = collections.namedtuple("PathwayCfg", "alpha reverse_input_channel")


def _short_side(h, w, min_size, max_size, inverse_uniform_sampling):
    """transform.py:305-327 (random_short_side_scale_jitter): the scaled (height, width)."""
    if inverse_uniform_sampling:
        size = int(round(1.0 / np.random.uniform(1.0 / max_size, 1.0 / min_size)))
    else:
        size = int(round(np.random.uniform(min_size, max_size)))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(math.floor((float(h) / w) * size)), size
    return size, int(math.floor((float(w) / h) * size))


def sample_spatial_params(height, width, spatial_idx=-1, min_scale=256, max_scale=320, crop_size=224,
                          random_horizontal_flip=True, inverse_uniform_sampling=False):
    """The decisions of `spatial_sampling` for one clip of height x width frames, without touching pixels.
    spatial_idx -1: random scale / crop / flip (training); 0, 1, 2: left|top, center, right|bottom uniform crop."""
    assert spatial_idx in [-1, 0, 1, 2]
    if spatial_idx == -1:
        nh, nw = _short_side(height, width, min_scale, max_scale, inverse_uniform_sampling)
        y = x = 0
        if not (nh == crop_size and nw == crop_size):  # transform.py:374-382 (random_crop)
            if nh > crop_size:
                y = int(np.random.randint(0, nh - crop_size))
            if nw > crop_size:
                x = int(np.random.randint(0, nw - crop_size))
        flip = bool(np.random.uniform() < 0.5) if random_horizontal_flip else False  # transform.py:417
        return SpatialParams(nh, nw, y, x, flip, crop_size)
    assert len({min_scale, max_scale, crop_size}) == 1
    nh, nw = _short_side(height, width, min_scale, max_scale, False)
    y = int(math.ceil((nh - crop_size) / 2))  # transform.py:446-458 (uniform_crop)
    x = int(math.ceil((nw - crop_size) / 2))
    if nh > nw:
        y = 0 if spatial_idx == 0 else (nh - crop_size if spatial_idx == 2 else y)
    else:
        x = 0 if spatial_idx == 0 else (nw - crop_size if spatial_idx == 2 else x)
    return SpatialParams(nh, nw, y, x, False, crop_size)


def slow_frame_indices(num_frames, alpha):
    """torch.linspace(0, T-1, T//alpha).long() (datasets/utils.py:96-104): T=32, alpha=4 -> 0,4,8,13,17,22,26,31."""
    return torch.linspace(0, num_frames - 1, num_frames // alpha).long()


def pack_pathway_output(cfg, frames):
    """[slow, fast] from C x T x H x W frames (any device).  `cfg`: a CfgNode (DATA.REVERSE_INPUT_CHANNEL,
    SLOWFAST.ALPHA, MODEL.ARCH ...) or a PathwayCfg."""
    if isinstance(cfg, PathwayCfg):
        alpha, reverse, single = cfg.alpha, cfg.reverse_input_channel, False
    else:
        alpha, reverse = cfg.SLOWFAST.ALPHA, cfg.DATA.REVERSE_INPUT_CHANNEL
        single = cfg.MODEL.ARCH in cfg.MODEL.SINGLE_PATHWAY_ARCH
        if not single and cfg.MODEL.ARCH not in cfg.MODEL.MULTI_PATHWAY_ARCH:
            raise NotImplementedError("Model arch {} is not in {}".format(
                cfg.MODEL.ARCH, cfg.MODEL.SINGLE_PATHWAY_ARCH + cfg.MODEL.MULTI_PATHWAY_ARCH))
    if reverse:
        frames = frames[[2, 1, 0], :, :, :]
    if single:
        return [frames]
    idx = slow_frame_indices(frames.shape[1], alpha).to(frames.device)
    return [torch.index_select(frames, 1, idx), frames]


def tensor_normalize(tensor, mean, std):
    """(uint8 -> float / 255) - mean, / std on the tensor's device (datasets/utils.py:298-315)."""
    if tensor.dtype == torch.uint8:
        tensor = tensor.float() / 255.0
    mean = torch.tensor(mean, device=tensor.device) if isinstance(mean, (list, tuple)) else mean
    std = torch.tensor(std, device=tensor.device) if isinstance(std, (list, tuple)) else std
    return (tensor - mean) / std


def gpu_input_step(clips, params, mean, std, alpha, reverse_input_channel=False, pad=(0, 0), wp=None):
    """The whole input step for a batch on the GPU.

    clips:  list of B decoded clips, uint8 [T, H_i, W_i, 3] device tensors (sizes may differ between clips); grayscale
            clips are uint8 [T, H_i, W_i] or [T, H_i, W_i, 1] with a one-element mean / std
    params: list of B SpatialParams (same crop for all)
    pad/wp: the stem's (ph, pw) and row pitch, from `engine.stem_geometry(first_conv, crop, crop)`
    alpha:  SLOWFAST.ALPHA; None for a single-pathway model (MODEL.ARCH in SINGLE_PATHWAY_ARCH): no slow pathway
    Returns [slow, fast] ([clip] with alpha=None) as sfhip.PackedClip — pass them to the model in place of the NCTHW
    tensors."""
    B = len(clips)
    assert B == len(params) and B > 0
    crop = params[0].crop
    T = clips[0].shape[0]
    ph, pw = pad
    wp = crop + 2 * pw if wp is None else wp
    dev = clips[0].device
    gray = clips[0].dim() == 3 or clips[0].shape[3] == 1
    C, cpad = (1, 1) if gray else (3, 4)
    paths = []  # (buffer, frame indices)
    if alpha is not None:
        idx = slow_frame_indices(T, alpha).to(device=dev, dtype=torch.int32)
        paths.append((torch.empty((B, idx.numel(), crop + 2 * ph, wp, cpad), dtype=torch.float32, device=dev), idx))
    paths.append((torch.empty((B, T, crop + 2 * ph, wp, cpad), dtype=torch.float32, device=dev), None))
    for b, (clip, p) in enumerate(zip(clips, params)):
        assert clip.shape[0] == T and p.crop == crop
        for buf, fi in paths:
            sfhip.clip_prologue(clip, buf[b], (p.new_h, p.new_w), (p.y, p.x), crop, p.flip, mean, std, frame_idx=fi,
                                reverse=reverse_input_channel, ph=ph, pw=pw)
    return [sfhip.PackedClip(buf, C, crop, crop, ph, pw) for buf, _ in paths]


def view_frame_indices(num_frames_total, clip_span, temporal_idx, num_clips, num_frames):
    """The frames view `temporal_idx` of `num_clips` takes from a decoded video of `num_frames_total` frames:
    decoder.py:55-83 (get_start_end_idx, uniform branch) and :35-52 (temporal_sampling).  int64 [num_frames]."""
    delta = max(num_frames_total - clip_span, 0)
    start = delta * temporal_idx / num_clips
    end = start + clip_span - 1
    index = torch.linspace(start, end, num_frames)
    return torch.clamp(index, 0, num_frames_total - 1).long()


def test_view_params(cfg, num_frames_total, height, width, fps=None):
    """The TEST.NUM_ENSEMBLE_VIEWS * TEST.NUM_SPATIAL_CROPS views of one decoded video (num_frames_total frames of
    height x width at `fps`; None: DATA.TARGET_FPS) in the order of the Kinetics dataset in test mode
    (datasets/kinetics.py:95-109, :166-181): view i has temporal index i // NUM_SPATIAL_CROPS and spatial index
    i % NUM_SPATIAL_CROPS.  Returns a list of (frame_indices int64 [DATA.NUM_FRAMES], SpatialParams).  Host arithmetic
    only: no RNG, no GPU."""
    n_views, n_crops = cfg.TEST.NUM_ENSEMBLE_VIEWS, cfg.TEST.NUM_SPATIAL_CROPS
    fps = cfg.DATA.TARGET_FPS if fps is None else fps
    span = cfg.DATA.NUM_FRAMES * cfg.DATA.SAMPLING_RATE * fps / cfg.DATA.TARGET_FPS  # decoder.py:449
    crop = cfg.DATA.TEST_CROP_SIZE
    views = []
    for i in range(n_views * n_crops):
        frames = view_frame_indices(num_frames_total, span, i // n_crops, n_views, cfg.DATA.NUM_FRAMES)
        views.append((frames, sample_spatial_params(height, width, i % n_crops, crop, crop, crop)))
    return views


test_view_params.__test__ = False  # not a pytest function


def view_table(views, n_slow_idx):
    """The int32 host table sf_clip_views reads: V rows (new_h, new_w, y0, x0, flip), the V * n_fast frame indices,
    then the Slow pathway's positions among the Fast frames (`n_slow_idx`: a tensor, possibly empty)."""
    rows = torch.tensor([[p.new_h, p.new_w, p.y, p.x, int(p.flip)] for _, p in views], dtype=torch.int32)
    frames = torch.stack([torch.as_tensor(f) for f, _ in views]).to(torch.int32)
    return torch.cat([rows.flatten(), frames.flatten(), n_slow_idx.to(torch.int32).flatten()]).contiguous()


def gpu_test_views(video, views, mean, std, alpha, reverse_input_channel=False, pad=(0, 0), wp=None):
    """Every test view of ONE decoded video in one kernel launch (sf_clip_views).

    video:  uint8 [T_total, H, W, 3] device tensor (grayscale: [T_total, H, W] or [T_total, H, W, 1])
    views:  list of V (frame_indices, SpatialParams) from `test_view_params` (same crop and frame count for all)
    the rest as `gpu_input_step`.  Returns [slow, fast] ([clip] with alpha=None) PackedClips of batch V holding the bits
    `gpu_input_step` gives for the V gathered clips; a frame both pathways take is resampled once."""
    V = len(views)
    assert V > 0
    crop = views[0][1].crop
    n_fast = len(views[0][0])
    assert all(p.crop == crop and len(f) == n_fast for f, p in views)
    ph, pw = pad
    wp = crop + 2 * pw if wp is None else wp
    dev = video.device
    gray = video.dim() == 3 or video.shape[3] == 1
    C, cpad = (1, 1) if gray else (3, 4)
    slow_idx = slow_frame_indices(n_fast, alpha) if alpha is not None else torch.zeros(0, dtype=torch.long)
    n_slow = slow_idx.numel()
    table_host = view_table(views, slow_idx)
    table = table_host.to(dev)  # the one upload: rows, frame indices and Slow positions together
    fast = torch.empty((V, n_fast, crop + 2 * ph, wp, cpad), dtype=torch.float32, device=dev)
    slow = torch.empty((V, n_slow, crop + 2 * ph, wp, cpad), dtype=torch.float32, device=dev) if n_slow else None
    sfhip.clip_views(video, table_host, table, n_slow, crop, mean, std, fast, slow, reverse=reverse_input_channel,
                     ph=ph, pw=pw)
    out = [sfhip.PackedClip(fast, C, crop, crop, ph, pw)]
    return out if slow is None else [sfhip.PackedClip(slow, C, crop, crop, ph, pw)] + out


def get_random_sampling_rate(long_cycle_sampling_rate, sampling_rate):
    """datasets/utils.py:318-327: with fewer frames in a long cycle the sampling rate is drawn from
    [sampling_rate, long_cycle_sampling_rate] (Python's `random`), so that some clips cover the original span;
    long_cycle_sampling_rate 0: `sampling_rate`, nothing drawn."""
    if long_cycle_sampling_rate > 0:
        assert long_cycle_sampling_rate >= sampling_rate
        return random.randint(sampling_rate, long_cycle_sampling_rate)
    return sampling_rate


def train_clip_params(cfg, num_frames_total, height, width, short_cycle_idx=None, fps=None):
    """The decisions of ONE training sample of the Kinetics / Jester loaders for a decoded span of num_frames_total
    frames of height x width at `fps` (None: DATA.TARGET_FPS), without touching pixels:
    the short-cycle crop and the jitter it implies (datasets/kinetics.py:146-165; short_cycle_idx 0 / 1: the crop is
    MULTIGRID.SHORT_CYCLE_FACTORS[idx] * DEFAULT_S, anything else: DATA.TRAIN_CROP_SIZE), the sampling rate (:186-189),
    the random temporal window (decoder.py:55-83 with clip_idx == -1 over the span of decoder.py:449), temporal_sampling
    (:35-52) and the random scale / crop / flip of spatial_sampling.
    Returns (frame_indices int64 [DATA.NUM_FRAMES], SpatialParams), the tuple `test_view_params` lists.
    RNG order, the reference's: Python `random` for the sampling rate (only with MULTIGRID.LONG_CYCLE_SAMPLING_RATE > 0),
    Python `random` for the window start, then numpy's global RNG for scale, crop y, crop x and flip."""
    min_scale, max_scale = cfg.DATA.TRAIN_JITTER_SCALES[0], cfg.DATA.TRAIN_JITTER_SCALES[1]
    crop_size = cfg.DATA.TRAIN_CROP_SIZE
    if short_cycle_idx in [0, 1]:
        crop_size = int(round(cfg.MULTIGRID.SHORT_CYCLE_FACTORS[short_cycle_idx] * cfg.MULTIGRID.DEFAULT_S))
    if cfg.MULTIGRID.DEFAULT_S > 0:  # a smaller scale is a larger "span" of the sampling grid
        min_scale = int(round(float(min_scale) * crop_size / cfg.MULTIGRID.DEFAULT_S))
    sampling_rate = get_random_sampling_rate(cfg.MULTIGRID.LONG_CYCLE_SAMPLING_RATE, cfg.DATA.SAMPLING_RATE)
    fps = cfg.DATA.TARGET_FPS if fps is None else fps
    span = cfg.DATA.NUM_FRAMES * sampling_rate * fps / cfg.DATA.TARGET_FPS  # decoder.py:449
    start = random.uniform(0, max(num_frames_total - span, 0))              # decoder.py:75-78
    index = torch.linspace(start, start + span - 1, cfg.DATA.NUM_FRAMES)
    frames = torch.clamp(index, 0, num_frames_total - 1).long()
    params = sample_spatial_params(height, width, spatial_idx=-1, min_scale=min_scale, max_scale=max_scale,
                                   crop_size=crop_size, random_horizontal_flip=cfg.DATA.RANDOM_FLIP,
                                   inverse_uniform_sampling=cfg.DATA.INV_UNIFORM_SAMPLE)
    return frames, params


BATCH_ROW = 9  # clip address, T, H, W, new_h, new_w, y0, x0, flip


def batch_table(videos, samples, n_slow_idx):
    """The int64 host table sf_clip_batch reads: B rows (address of videos[b], T_b, H_b, W_b, new_h, new_w, y0, x0,
    flip), the B * n_fast frame indices into each clip's own span (clip-major), then the Slow pathway's positions
    among the Fast frames (`n_slow_idx`: a tensor, possibly empty)."""
    rows = torch.tensor([[v.data_ptr(), v.shape[0], v.shape[1], v.shape[2], p.new_h, p.new_w, p.y, p.x, int(p.flip)]
                         for v, (_, p) in zip(videos, samples)], dtype=torch.int64)
    frames = torch.stack([torch.as_tensor(f) for f, _ in samples]).to(torch.int64)
    return torch.cat([rows.flatten(), frames.flatten(), n_slow_idx.to(torch.int64).flatten()]).contiguous()


def gpu_train_batch(videos, samples, mean, std, alpha, reverse_input_channel=False, pad=(0, 0), wp=None):
    """The whole input step of ONE training batch in one kernel launch (sf_clip_batch), temporal sampling included.

    videos:  list of B decoded spans, uint8 [T_i, H_i, W_i, 3] device tensors, each its own allocation and size
             (grayscale: [T_i, H_i, W_i] or [T_i, H_i, W_i, 1]); they stay alive until the launch has run
    samples: list of B (frame_indices, SpatialParams) from `train_clip_params` (same crop and frame count for all)
    the rest as `gpu_input_step`.  One table upload, one launch.  Returns [slow, fast] ([clip] with alpha=None)
    PackedClips of batch B holding the bits `gpu_input_step` gives for the B gathered clips; a frame both pathways
    take is resampled once."""
    B = len(videos)
    assert B == len(samples) and B > 0
    crop = samples[0][1].crop
    n_fast = len(samples[0][0])
    assert all(p.crop == crop and len(f) == n_fast for f, p in samples)
    ph, pw = pad
    wp = crop + 2 * pw if wp is None else wp
    dev = videos[0].device
    gray = videos[0].dim() == 3 or videos[0].shape[3] == 1
    for v in videos:
        if not v.is_cuda or v.device != dev:
            raise sfhip.SfhipError("gpu_train_batch: every decoded span lives on one GPU, got %s" % v.device)
        assert v.dtype == torch.uint8 and v.dim() in (3, 4) and v.is_contiguous()
        assert (v.dim() == 3 or v.shape[3] == 1) == gray and (gray or v.shape[3] == 3)
    C, cpad = (1, 1) if gray else (3, 4)
    slow_idx = slow_frame_indices(n_fast, alpha) if alpha is not None else torch.zeros(0, dtype=torch.long)
    n_slow = slow_idx.numel()
    table_host = batch_table(videos, samples, slow_idx)
    table = table_host.to(dev)  # the one upload: rows, frame indices and Slow positions together
    fast = torch.empty((B, n_fast, crop + 2 * ph, wp, cpad), dtype=torch.float32, device=dev)
    slow = torch.empty((B, n_slow, crop + 2 * ph, wp, cpad), dtype=torch.float32, device=dev) if n_slow else None
    sfhip.clip_batch(table_host, table, n_slow, crop, mean, std, fast, slow, gray=gray, reverse=reverse_input_channel,
                     ph=ph, pw=pw)
    out = [sfhip.PackedClip(fast, C, crop, crop, ph, pw)]
    return out if slow is None else [sfhip.PackedClip(slow, C, crop, crop, ph, pw)] + out


# ---- mixup / CutMix (upstream SlowFast datasets/mixup.py, after timm): the host keeps the draws, the pixels are mixed
# inside the one-launch input step (sf_clip_batch_mix) and the labels inside the loss (sf_ce_mix) from the same rows.
MIX_NONE, MIX_MIXUP, MIX_CUTMIX = 0, 1, 2
MixParams = collections.namedtuple("MixParams", "partner mode lam box")
MixParams.__doc__ = """The mix decision of one batch of B clips.  partner: B row indices; mode (MIX_NONE / MIX_MIXUP /
MIX_CUTMIX), lam (a Python float in [0, 1]) and box ((y0, x0, y1, x1) in output crop coordinates): one value for the
batch, or a sequence of B values (one per row)."""


def rand_bbox(crop, lam):
    """mixup.py rand_bbox (margin 0) for a crop x crop output: a box of side ratio sqrt(1 - lam) around a centre drawn
    uniformly (numpy's global RNG: cy, then cx), clipped to the crop.  Returns (y0, x0, y1, x1)."""
    ratio = np.sqrt(1.0 - lam)
    cut_h, cut_w = int(crop * ratio), int(crop * ratio)
    cy = int(np.random.randint(0, crop))
    cx = int(np.random.randint(0, crop))
    y0, y1 = int(np.clip(cy - cut_h // 2, 0, crop)), int(np.clip(cy + cut_h // 2, 0, crop))
    x0, x1 = int(np.clip(cx - cut_w // 2, 0, crop)), int(np.clip(cx + cut_w // 2, 0, crop))
    return y0, x0, y1, x1


def sample_mix_params(B, crop, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5):
    """The decision of MixUp._params_per_batch / _mix_batch (mixup.py, mode "batch") for one batch, without touching
    pixels: ONE decision per batch, the partner of row b is B - 1 - b (x.flip(0)).
    RNG order, upstream's, all from numpy's global RNG: rand() against `prob`; with both alphas positive rand() against
    `switch_prob` (CutMix when below); lam ~ beta(alpha, alpha) of the chosen form; for CutMix the box centre cy, then
    cx (`rand_bbox`), after which lam is corrected to 1 - box area / crop^2 (correct_lam).  Nothing beyond the first
    rand() is drawn when it is not below `prob`; lam == 1 after the draw means no mixing, as upstream.
    Returns MixParams; without mixing: mode MIX_NONE, lam 1.0 and an empty box."""
    if B <= 0 or crop <= 0:
        raise ValueError("sample_mix_params: B and crop must be positive, got %r and %r" % (B, crop))
    if mixup_alpha < 0 or cutmix_alpha < 0 or not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
        raise ValueError("sample_mix_params: alphas must not be negative and the probabilities lie in [0, 1]")
    partner = tuple(B - 1 - b for b in range(B))
    none = MixParams(partner, MIX_NONE, 1.0, (0, 0, 0, 0))
    if mixup_alpha <= 0 and cutmix_alpha <= 0:
        return none
    if not np.random.rand() < prob:
        return none
    if mixup_alpha > 0 and cutmix_alpha > 0:
        cutmix = bool(np.random.rand() < switch_prob)
    else:
        cutmix = cutmix_alpha > 0
    alpha = cutmix_alpha if cutmix else mixup_alpha
    lam = float(np.random.beta(alpha, alpha))
    if lam == 1.0:
        return none
    if not cutmix:
        return MixParams(partner, MIX_MIXUP, lam, (0, 0, 0, 0))
    y0, x0, y1, x1 = rand_bbox(crop, lam)
    lam = 1.0 - (y1 - y0) * (x1 - x0) / float(crop * crop)
    return MixParams(partner, MIX_CUTMIX, lam, (y0, x0, y1, x1))


def _per_row(v, B, what):
    if isinstance(v, (int, float, np.integer, np.floating)):
        return [v] * B
    v = list(v)
    if len(v) != B:
        raise ValueError("mix_rows: %s has %d entries for %d rows" % (what, len(v), B))
    return v


def mix_rows(mix):
    """The int64 host rows [B, 7] sf_clip_batch_mix and sf_ce_mix read: partner, mode, lam as the bit pattern of its
    float32 value (low 32 bits), y0, x0, y1, x1.  Both kernels use that float32 lam — pixels and labels are mixed by
    the same number."""
    B = len(mix.partner)
    if B == 0:
        raise ValueError("mix_rows: no rows")
    modes, lams = _per_row(mix.mode, B, "mode"), _per_row(mix.lam, B, "lam")
    box = mix.box
    boxes = [tuple(box)] * B if len(box) == 4 and not isinstance(box[0], (tuple, list)) else _per_row(box, B, "box")
    rows = torch.empty((B, sfhip.SF_MIX_ROW), dtype=torch.int64)
    for b in range(B):
        lam = float(lams[b])
        if not 0.0 <= lam <= 1.0:
            raise ValueError("mix_rows: lam must lie in [0, 1], got %r" % (lams[b],))
        if int(modes[b]) not in (MIX_NONE, MIX_MIXUP, MIX_CUTMIX):
            raise ValueError("mix_rows: mode must be 0 (none), 1 (mixup) or 2 (CutMix), got %r" % (modes[b],))
        if len(boxes[b]) != 4:
            raise ValueError("mix_rows: a box is (y0, x0, y1, x1), got %r" % (boxes[b],))
        bits = int(np.float32(lam).view(np.uint32))
        rows[b] = torch.tensor([int(mix.partner[b]), int(modes[b]), bits] + [int(v) for v in boxes[b]], dtype=torch.int64)
    return rows


def gpu_train_batch_mix(videos, samples, mix, mean, std, alpha, reverse_input_channel=False, pad=(0, 0), wp=None):
    """`gpu_train_batch` with mixup / CutMix inside the launch (sf_clip_batch_mix): `mix` is a MixParams for the B
    clips (`sample_mix_params`).  Still one table upload — the mix rows ride behind the batch table — and one launch.
    Returns (packed, rows): the PackedClips as gpu_train_batch returns them, and the [B, 7] int64 DEVICE view of the mix
    rows inside the uploaded table, which the loss takes (`HipCrossEntropy(...)(preds, labels, mix=rows)`); its
    `mix_host` attribute is the host copy the loss entry checks."""
    B = len(videos)
    assert B == len(samples) and B > 0
    if len(mix.partner) != B:
        raise ValueError("gpu_train_batch_mix: mix rows for %d clips, the batch has %d" % (len(mix.partner), B))
    crop = samples[0][1].crop
    n_fast = len(samples[0][0])
    assert all(p.crop == crop and len(f) == n_fast for f, p in samples)
    ph, pw = pad
    wp = crop + 2 * pw if wp is None else wp
    dev = videos[0].device
    gray = videos[0].dim() == 3 or videos[0].shape[3] == 1
    for v in videos:
        if not v.is_cuda or v.device != dev:
            raise sfhip.SfhipError("gpu_train_batch_mix: every decoded span lives on one GPU, got %s" % v.device)
        assert v.dtype == torch.uint8 and v.dim() in (3, 4) and v.is_contiguous()
        assert (v.dim() == 3 or v.shape[3] == 1) == gray and (gray or v.shape[3] == 3)
    C, cpad = (1, 1) if gray else (3, 4)
    slow_idx = slow_frame_indices(n_fast, alpha) if alpha is not None else torch.zeros(0, dtype=torch.long)
    n_slow = slow_idx.numel()
    rows_host = mix_rows(mix)
    table_host = torch.cat([batch_table(videos, samples, slow_idx), rows_host.flatten()]).contiguous()
    table = table_host.to(dev)  # the one upload: rows, frame indices, Slow positions and mix rows together
    fast = torch.empty((B, n_fast, crop + 2 * ph, wp, cpad), dtype=torch.float32, device=dev)
    slow = torch.empty((B, n_slow, crop + 2 * ph, wp, cpad), dtype=torch.float32, device=dev) if n_slow else None
    sfhip.clip_batch_mix(table_host, table, n_slow, crop, mean, std, fast, slow, gray=gray,
                         reverse=reverse_input_channel, ph=ph, pw=pw)
    out = [sfhip.PackedClip(fast, C, crop, crop, ph, pw)]
    rows = table[table.numel() - B * sfhip.SF_MIX_ROW:].view(B, sfhip.SF_MIX_ROW)
    rows.mix_host = rows_host
    return (out if slow is None else [sfhip.PackedClip(slow, C, crop, crop, ph, pw)] + out), rows


# ---- Jester's colour jitter (datasets/decoder.py:456-469 -> transform.RandomColorJitter, transform.py:692-717): the host
# keeps the three draws per clip, the pixels are jittered inside the one-launch input step (sf_clip_batch_jitter).
ColorJitter = collections.namedtuple("ColorJitter", "bright contrast color")
ColorJitter.__doc__ = """The factors ImageEnhance.Brightness, .Contrast and .Color take for every frame of ONE clip
(Python floats; the kernels use their float32 values, as PIL does).  A factor <= 0 skips its stage."""


def sample_color_jitter(lo=0.4, hi=1.4):
    """decoder.py:458-460: bright, contrast, color ~ uniform(lo, hi) from Python's `random`, in that order."""
    bright = random.uniform(lo, hi)
    contrast = random.uniform(lo, hi)
    color = random.uniform(lo, hi)
    return ColorJitter(bright, contrast, color)


def jester_clip_params(cfg, mode, num_frames_total, height, width, short_cycle_idx=None, fps=None):
    """The decisions of ONE sample of the Jester loader (datasets/jester.py:142-165, :186-189, :212-247) in `mode`
    "train" or "val" — both are sampled and jittered like training clips there — for a decoded span of
    num_frames_total frames of height x width: `train_clip_params`' decisions and the colour jitter of
    decode(..., jester=True).  Returns (frame_indices, SpatialParams, ColorJitter).
    RNG order, the reference's: Python `random` for the sampling rate (only with MULTIGRID.LONG_CYCLE_SAMPLING_RATE > 0),
    the window start, then bright, contrast, color; numpy's global RNG for scale, crop y, crop x and flip (drawn after
    decode returns; the two generators do not meet).  The reference does not jitter test views: mode "test" raises."""
    if mode == "test":
        raise NotImplementedError("the Jester loader neither jitters nor randomly samples its test views "
                                  "(decode(..., jester_test=True)): take them from test_view_params")
    if mode not in ("train", "val"):
        raise NotImplementedError("Does not support {} mode".format(mode))
    # the numpy draws of train_clip_params use the other generator, so taking the jitter after them keeps both streams
    frames, params = train_clip_params(cfg, num_frames_total, height, width, short_cycle_idx=short_cycle_idx, fps=fps)
    return frames, params, sample_color_jitter()


def jitter_rows(jitters):
    """The int64 host rows [B, 3] sf_clip_batch_jitter reads behind the batch table: per clip the brightness, contrast
    and colour factors as the bit patterns of their float32 values (low 32 bits).  None: a clip that is not jittered
    (three zeros: every stage skipped)."""
    rows = torch.empty((len(jitters), sfhip.SF_JITTER_ROW), dtype=torch.int64)
    for b, j in enumerate(jitters):
        vals = (0.0, 0.0, 0.0) if j is None else tuple(float(v) for v in j)
        if len(vals) != 3 or not all(abs(v) <= float(np.finfo(np.float32).max) for v in vals):  # NaN fails too
            raise ValueError("jitter_rows: a clip takes three finite factors (bright, contrast, color), got %r" % (j,))
        rows[b] = torch.tensor([_f32_bits(v) for v in vals], dtype=torch.int64)
    return rows


def gpu_train_batch_jitter(videos, samples, jitters, mean, std, alpha, reverse_input_channel=False, pad=(0, 0),
                           wp=None):
    """`gpu_train_batch` with Jester's colour jitter inside the call (sf_clip_batch_jitter): `jitters` holds one
    ColorJitter (or None) per clip, as `jester_clip_params` returns them.  Still one table upload — the jitter rows ride
    behind the batch table — and one ABI call, which is two launches: the grey mean of every sampled frame (the
    contrast stage's reference), then the clip launch.  RGB spans only.  Returns [slow, fast] ([clip] with alpha=None)
    PackedClips holding the bits `gpu_train_batch` gives for spans jittered frame by frame with PIL."""
    B = len(videos)
    assert B == len(samples) and B > 0
    if len(jitters) != B:
        raise ValueError("gpu_train_batch_jitter: jitter factors for %d clips, the batch has %d" % (len(jitters), B))
    crop = samples[0][1].crop
    n_fast = len(samples[0][0])
    assert all(p.crop == crop and len(f) == n_fast for f, p in samples)
    ph, pw = pad
    wp = crop + 2 * pw if wp is None else wp
    dev = videos[0].device
    for v in videos:
        if v.dim() == 3 or v.shape[3] == 1:
            raise ValueError("gpu_train_batch_jitter: the colour jitter is defined for RGB spans [T, H, W, 3], got %s" %
                             (tuple(v.shape),))
        if not v.is_cuda or v.device != dev:
            raise sfhip.SfhipError("gpu_train_batch_jitter: every decoded span lives on one GPU, got %s" % v.device)
        assert v.dtype == torch.uint8 and v.dim() == 4 and v.shape[3] == 3 and v.is_contiguous()
    slow_idx = slow_frame_indices(n_fast, alpha) if alpha is not None else torch.zeros(0, dtype=torch.long)
    n_slow = slow_idx.numel()
    table_host = torch.cat([batch_table(videos, samples, slow_idx), jitter_rows(jitters).flatten()]).contiguous()
    table = table_host.to(dev)  # the one upload: rows, frame indices, Slow positions and jitter rows together
    means = torch.empty((B, n_fast), dtype=torch.int32, device=dev)  # the first launch writes every element
    fast = torch.empty((B, n_fast, crop + 2 * ph, wp, 4), dtype=torch.float32, device=dev)
    slow = torch.empty((B, n_slow, crop + 2 * ph, wp, 4), dtype=torch.float32, device=dev) if n_slow else None
    sfhip.clip_batch_jitter(table_host, table, n_slow, crop, mean, std, means, fast, slow,
                            reverse=reverse_input_channel, ph=ph, pw=pw)
    out = [sfhip.PackedClip(fast, 3, crop, crop, ph, pw)]
    return out if slow is None else [sfhip.PackedClip(slow, 3, crop, crop, ph, pw)] + out


# ---- the detection (AVA) input step: datasets/ava_dataset.py:233-338 with AVA.IMG_PROC_BACKEND "pytorch", and the box
# collation of datasets/loader.py:18-52.  The host keeps the draws and the boxes; pixels go through sf_clip_batch_det.
DetParams = collections.namedtuple("DetParams", "new_h new_w y x flip win_h win_w crop offsets")
DET_ROW = 12  # clip address, T, H, W, new_h, new_w, y0, x0, flip, three lighting offsets (float32 bit patterns)


def det_sequence(center_idx, half_len, sample_rate, num_frames):
    """datasets/utils.py:50-70 (get_sequence): the frames of the clip around `center_idx`, clamped into the video."""
    return [min(max(i, 0), num_frames - 1) for i in range(center_idx - half_len, center_idx + half_len, sample_rate)]


def det_clip_params(cfg, split, height, width):
    """The decisions of `Ava._images_and_boxes_preprocessing` for one clip of height x width frames, without touching
    pixels -> DetParams.  `offsets` are the PCA-lighting offsets (float32 values) in the order they are added to source
    channels 0..2; (win_h, win_w) is the output window and `crop` the size the boxes are finally clipped to.
    numpy's global RNG, the reference's order: train — scale, crop y, crop x (each only when the extent exceeds the
    size), flip (always drawn; this backend ignores DATA.RANDOM_FLIP), then normal(0, 0.1, (1, 3)) with
    AVA.TRAIN_USE_COLOR_AUGMENTATION; val / test — one scale draw and, with AVA.TEST_FORCE_FLIP, one flip draw."""
    if cfg.AVA.IMG_PROC_BACKEND != "pytorch":
        raise NotImplementedError(
            "AVA.IMG_PROC_BACKEND %r resamples with OpenCV, which the device input step does not reproduce: select "
            "AVA.IMG_PROC_BACKEND \"pytorch\"" % (cfg.AVA.IMG_PROC_BACKEND,))
    if split not in ("train", "val", "test"):
        raise NotImplementedError("{} split not supported yet!".format(split))
    offsets = (0.0, 0.0, 0.0)
    if split == "train":
        lighting = cfg.AVA.TRAIN_USE_COLOR_AUGMENTATION
        if lighting and not cfg.AVA.TRAIN_PCA_JITTER_ONLY:
            raise NotImplementedError(
                "AVA.TRAIN_PCA_JITTER_ONLY False: in the reference's pytorch backend transform.grayscale aliases its "
                "input, so contrast and saturation jitter collapse the clip to one grey image; that is not reproduced "
                "here — keep AVA.TRAIN_PCA_JITTER_ONLY True")
        size = cfg.DATA.TRAIN_CROP_SIZE
        nh, nw = _short_side(height, width, cfg.DATA.TRAIN_JITTER_SCALES[0], cfg.DATA.TRAIN_JITTER_SCALES[1], False)
        if nh == size and nw == size:
            raise ValueError("the scaled frame is already %d x %d: the reference's random_crop returns a bare tensor "
                             "there and its caller fails to unpack it" % (size, size))
        if nh < size or nw < size:
            raise ValueError("the scaled frame %d x %d is smaller than the %d x %d crop" % (nh, nw, size, size))
        y = int(np.random.randint(0, nh - size)) if nh > size else 0  # transform.py:376-383
        x = int(np.random.randint(0, nw - size)) if nw > size else 0
        flip = bool(np.random.uniform() < 0.5)                        # transform.py:415
        if lighting:                                                  # transform.py:651-661
            alpha = np.random.normal(0, 0.1, size=(1, 3))
            eig_vec = np.array(cfg.AVA.TRAIN_PCA_EIGVEC).astype(np.float32)
            eig_val = np.reshape(np.array(cfg.AVA.TRAIN_PCA_EIGVAL).astype(np.float32), (1, 3))
            rgb = np.sum(eig_vec * np.repeat(alpha, 3, axis=0) * np.repeat(eig_val, 3, axis=0), axis=1)  # float64
            offsets = tuple(float(np.float32(rgb[2 - c])) for c in range(3))  # a float32 tensor + a Python scalar
        return DetParams(nh, nw, y, x, flip, size, size, size, offsets)
    size = cfg.DATA.TEST_CROP_SIZE
    nh, nw = _short_side(height, width, size, size, False)  # one draw, as the reference spends it
    if split == "val":
        y = int(math.ceil((nh - size) / 2))  # transform.py:447-448 (uniform_crop, spatial_idx 1)
        x = int(math.ceil((nw - size) / 2))
        win_h = win_w = size
    else:
        y, x, win_h, win_w = 0, 0, nh, nw  # no crop: the window is the whole scaled frame
    flip = bool(np.random.uniform() < 1) if cfg.AVA.TEST_FORCE_FLIP else False
    return DetParams(nh, nw, y, x, flip, win_h, win_w, size, offsets)


def _clip_boxes(boxes, height, width):
    """transform.py:471-490 (clip_boxes_to_image)."""
    out = boxes.copy()
    out[:, [0, 2]] = np.minimum(width - 1.0, np.maximum(0.0, boxes[:, [0, 2]]))
    out[:, [1, 3]] = np.minimum(height - 1.0, np.maximum(0.0, boxes[:, [1, 3]]))
    return out


def det_boxes(boxes01, height, width, params):
    """The box pipeline of `Ava._images_and_boxes_preprocessing` in numpy float64: [k, 4] boxes (x1, y1, x2, y2) in
    [0, 1] of a height x width frame -> pixels of the output window, through the decisions `params` holds.
    The final clip is to (crop, crop) in every split — in `test`, where the frame is wider, too: the reference's
    behaviour."""
    p = params
    boxes = np.array(boxes01, dtype=np.float64, copy=True).reshape(-1, 4)
    boxes[:, [0, 2]] *= width
    boxes[:, [1, 3]] *= height
    boxes = _clip_boxes(boxes, height, width)
    if (p.new_h, p.new_w) != (height, width):  # transform.py:320-327: one factor for both axes
        if width < height:
            boxes = boxes * float(p.new_h) / height
        else:
            boxes = boxes * float(p.new_w) / width
    boxes[:, [0, 2]] = boxes[:, [0, 2]] - p.x  # transform.py:352-354 (crop_boxes)
    boxes[:, [1, 3]] = boxes[:, [1, 3]] - p.y
    if p.flip:                                 # transform.py:418-420
        boxes[:, [0, 2]] = p.win_w - boxes[:, [2, 0]] - 1
    return _clip_boxes(boxes, p.crop, p.crop)


def _f32_bits(v):
    return int(np.array(v, dtype=np.float32).view(np.uint32))


def det_table(videos, samples, n_slow_idx):
    """The int64 host table sf_clip_batch_det reads: B rows (address of videos[b], T_b, H_b, W_b, new_h, new_w, y0, x0,
    flip, three lighting offsets as float32 bit patterns), the B * n_fast frame indices (clip-major), then the Slow
    pathway's positions among the Fast frames (`n_slow_idx`: a tensor, possibly empty)."""
    rows = torch.tensor([[v.data_ptr(), v.shape[0], v.shape[1], v.shape[2], p.new_h, p.new_w, p.y, p.x, int(p.flip)] +
                         [_f32_bits(o) for o in p.offsets] for v, (_, p) in zip(videos, samples)], dtype=torch.int64)
    frames = torch.stack([torch.as_tensor(f) for f, _ in samples]).to(torch.int64)
    return torch.cat([rows.flatten(), frames.flatten(), n_slow_idx.to(torch.int64).flatten()]).contiguous()


def collate_boxes(boxes_list):
    """`detection_collate` for "boxes" / "ori_boxes" (datasets/loader.py:35-44): [K, 5] float32 — the sample's index in
    the batch, then the box — from B arrays [k_i, 4], on the host."""
    rows = [np.concatenate([np.full((len(b), 1), float(i)), np.asarray(b, dtype=np.float64).reshape(-1, 4)], axis=1)
            for i, b in enumerate(boxes_list)]
    return torch.tensor(np.concatenate(rows, axis=0)).float()


def collate_detection_extras(ori_boxes_list, metadata_list):
    """(ori_boxes [K, 5] float32, metadata [K, 2] int64) as `detection_collate` gives them (datasets/loader.py:35-48),
    on the host: what DeviceAVAMeter.update_stats takes beside the predictions, once moved to the GPU."""
    metadata = torch.tensor([list(m) for md in metadata_list for m in md]).view(-1, 2)
    return collate_boxes(ori_boxes_list), metadata


def gpu_detection_batch(videos, samples, boxes_list, mean, std, alpha, reverse_input_channel=False, pad=(0, 0),
                        wp=None):
    """The whole input step of ONE detection batch in one kernel launch (sf_clip_batch_det), boxes included.

    videos:     list of B frame spans, uint8 [T_i, H_i, W_i, 3] device tensors in BGR order, each its own allocation;
                they stay alive until the launch has run
    samples:    list of B (frame_indices, DetParams): indices into the span (`det_sequence`, or range(T) for a span that
                holds exactly the clip) and `det_clip_params`' decisions; one window and one frame count for the batch
    boxes_list: list of B [k_i, 4] arrays from `det_boxes`
    mean, std:  DATA.MEAN / DATA.STD, applied in source (BGR) order as the reference does
    reverse_input_channel: `not AVA.BGR`
    the rest as `gpu_input_step`.  One table upload, one launch.  Returns ([slow, fast] PackedClips ([clip] with
    alpha=None), bboxes): bboxes is the [K, 5] float32 device tensor `detection_collate` gives, computed on the host
    and carried as float32 bit patterns in the tail of the table's upload — a view of the uploaded table."""
    B = len(videos)
    assert B == len(samples) == len(boxes_list) and B > 0
    p0 = samples[0][1]
    n_fast = len(samples[0][0])
    for f, p in samples:
        if (p.win_h, p.win_w) != (p0.win_h, p0.win_w):
            raise ValueError("the clips of one batch share one output window: got %d x %d and %d x %d" % (
                p0.win_h, p0.win_w, p.win_h, p.win_w))
        assert len(f) == n_fast
    win_h, win_w = p0.win_h, p0.win_w
    ph, pw = pad
    wp = win_w + 2 * pw if wp is None else wp
    dev = videos[0].device
    for v in videos:
        if not v.is_cuda or v.device != dev:
            raise sfhip.SfhipError("gpu_detection_batch: every frame span lives on one GPU, got %s" % v.device)
        assert v.dtype == torch.uint8 and v.dim() == 4 and v.shape[3] == 3 and v.is_contiguous()
    slow_idx = slow_frame_indices(n_fast, alpha) if alpha is not None else torch.zeros(0, dtype=torch.long)
    n_slow = slow_idx.numel()
    head = det_table(videos, samples, slow_idx)
    bboxes = collate_boxes(boxes_list)  # float32 [K, 5]
    K = bboxes.shape[0]
    tail = torch.zeros((5 * K + 1) // 2 * 2, dtype=torch.float32)
    tail[:5 * K] = bboxes.flatten()
    table_host = torch.cat([head, tail.view(torch.int64)]).contiguous()
    table = table_host.to(dev)  # the one upload: rows, frame indices, Slow positions and the boxes together
    fast = torch.empty((B, n_fast, win_h + 2 * ph, wp, 4), dtype=torch.float32, device=dev)
    slow = torch.empty((B, n_slow, win_h + 2 * ph, wp, 4), dtype=torch.float32, device=dev) if n_slow else None
    sfhip.clip_batch_det(table_host, table, n_slow, (win_h, win_w), mean, std, fast, slow,
                         reverse=reverse_input_channel, ph=ph, pw=pw)
    out = [sfhip.PackedClip(fast, 3, win_h, win_w, ph, pw)]
    out = out if slow is None else [sfhip.PackedClip(slow, 3, win_h, win_w, ph, pw)] + out
    return out, table[head.numel():].view(torch.float32)[:5 * K].view(K, 5)


def stem_input_geometry(model, crop, width=None):
    """(ph, pw, Wp) shared by the model's pathway stems (their first convolutions have the same H/W kernel,
    stride and padding) for crop x crop frames (crop x width with `width`: a rectangular window)."""
    from slowfast.models import engine
    geos = set()
    stem = next(model.children())  # s1 (s0 for GhostNet): one `pathway{p}_stem` per pathway
    for m in stem.modules():
        if isinstance(m, torch.nn.Conv3d) and m.in_channels <= 4 and m.groups == 1:
            geos.add(engine.stem_geometry(m, crop, crop if width is None else width))
    if len(geos) != 1:
        raise ValueError("pathway stems disagree on the input geometry: %s" % sorted(geos))
    return geos.pop()
