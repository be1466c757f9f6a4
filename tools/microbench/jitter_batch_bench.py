#!/usr/bin/env python3
"""Jester's colour jitter inside the one-launch training input step: the frame-mean launch (`sf_frame_grey_means`) and
the pair `sf_clip_batch_jitter` issues (means, then the jittered clip launch) against the plain `sf_clip_batch` launch
on the same spans and batch table.

Two shapes, every clip's frames, scale, crop and flip from `train_clip_params` and its factors from
`sample_color_jitter` (seeded), stem padding (3, 3), alpha 4:
  jester:   8 decoded spans of 37 frames of 100 x 176 uint8 RGB, 16 Fast + 4 Slow frames at crop 112 (scales 128 .. 160)
  kinetics: 8 decoded spans of 64 frames of 256 x 340, 32 Fast + 8 Slow frames at crop 224 (scales 256 .. 320)
What is timed is the LAUNCHES alone: tables uploaded and buffers allocated beforehand, REPS calls between two HIP
events.  Every arm warmed up, then ROUNDS rounds in which the arms alternate; the figure is the median round, the
spread its min .. max.  The C ABI issues the pair in one call, so the jittered clip launch on its own is the pair minus
the means launch (a difference of two medians, named as such).  Bytes: the means launch reads 3 B per source pixel of
every sampled frame, the clip launch writes 16 B per output pixel of both pathways.  Clocks not pinned.
usage: tools/microbench/jitter_batch_bench.py [out.txt]"""
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import sfhip  # noqa: E402
from slowfast.config.defaults import get_cfg  # noqa: E402
from slowfast.datasets import utils as ds  # noqa: E402

SHAPES = {  # B, frames per span, H, W, Fast frames, crop, jitter scales
    "jester": (8, 37, 100, 176, 16, 112, [128, 160]),
    "kinetics": (8, 64, 256, 340, 32, 224, [256, 320]),
}
ALPHA, PAD = 4, (3, 3)
ROUNDS, REPS = 15, 20
MEAN, STD = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225]


def measure(shape):
    B, t_span, H, W, n_fast, crop, scales = SHAPES[shape]
    cfg = get_cfg()
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.DATA.TRAIN_CROP_SIZE = n_fast, 2, crop
    cfg.DATA.TRAIN_JITTER_SCALES, cfg.MULTIGRID.DEFAULT_S = scales, 0
    random.seed(1)
    np.random.seed(1)
    videos = [torch.randint(0, 256, (t_span, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    drawn = [ds.jester_clip_params(cfg, "train", t_span, H, W) for _ in range(B)]
    samples, jitters = [(f, p) for f, p, _ in drawn], [j for _, _, j in drawn]
    slow_idx = ds.slow_frame_indices(n_fast, ALPHA)
    n_slow = slow_idx.numel()
    ph, pw = PAD
    wp = crop + 2 * pw
    fast = torch.empty((B, n_fast, crop + 2 * ph, wp, 4), dtype=torch.float32, device="cuda")
    slow = torch.empty((B, n_slow, crop + 2 * ph, wp, 4), dtype=torch.float32, device="cuda")
    means = torch.empty((B, n_fast), dtype=torch.int32, device="cuda")
    base = ds.batch_table(videos, samples, slow_idx)
    base_dev = base.cuda()
    host = torch.cat([base, ds.jitter_rows(jitters).flatten()]).contiguous()
    dev = host.cuda()
    none = torch.cat([base, ds.jitter_rows([None] * B).flatten()]).contiguous()
    arms = [
        ("sf_clip_batch", lambda: sfhip.clip_batch(base, base_dev, n_slow, crop, MEAN, STD, fast, slow, ph=ph, pw=pw)),
        ("sf_frame_grey_means", lambda: sfhip.frame_grey_means(host, dev, n_slow, means)),
        ("sf_clip_batch_jitter (the pair)", lambda: sfhip.clip_batch_jitter(host, dev, n_slow, crop, MEAN, STD, means, fast,
                                                                            slow, ph=ph, pw=pw)),
    ]
    # the outputs must not change: with every stage skipped the pair writes the plain launch's bits
    arms[0][1]()
    want = (fast.clone(), slow.clone())
    sfhip.clip_batch_jitter(none, none.cuda(), n_slow, crop, MEAN, STD, means, fast, slow, ph=ph, pw=pw)
    torch.cuda.synchronize()
    same = torch.equal(fast.view(torch.int32), want[0].view(torch.int32)) and \
        torch.equal(slow.view(torch.int32), want[1].view(torch.int32))
    del want
    for _, fn in arms:  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for _ in range(ROUNDS):
        for name, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / REPS)  # us per call
    written = (fast.numel() + slow.numel()) * 4
    read = B * n_fast * H * W * 3
    med = {n: statistics.median(t) for n, t in times.items()}
    plain, mean_t, pair = med["sf_clip_batch"], med["sf_frame_grey_means"], med["sf_clip_batch_jitter (the pair)"]
    lines = ["%s: %d spans of %d x %d x %d x 3 uint8, %d + %d frames at crop %d, pad %s: the means launch reads %.1f MB, the "
             "clip launch writes %.1f MB; all stages skipped bitwise equal to sf_clip_batch: %s; HIP events around %d "
             "calls, median of %d alternating rounds (min .. max)" % (
                 shape, B, t_span, H, W, n_fast, n_slow, crop, PAD, read / 1e6, written / 1e6, same, REPS, ROUNDS)]
    for name, _ in arms:
        ts = times[name]
        lines.append("%-38s %8.1f us (%7.1f .. %7.1f)  %5.2fx of sf_clip_batch" % (
            name, med[name], min(ts), max(ts), med[name] / plain))
    lines.append("%-38s %8.1f us  %5.2fx of sf_clip_batch  (pair - means, a difference of medians)" % (
        "the jittered clip launch", pair - mean_t, (pair - mean_t) / plain))
    lines.append("%-38s means %.2f TB/s of the bytes read; clip launch %.2f TB/s of the bytes written (plain: %.2f)" % (
        "rates", read / mean_t / 1e6, written / (pair - mean_t) / 1e6, written / plain / 1e6))
    lines.append("expectation: the pair under twice sf_clip_batch -> %s (%.2fx)" % (
        "met" if pair < 2 * plain else "NOT met", pair / plain))
    return lines


def main():
    assert torch.cuda.is_available(), "jitter_batch_bench.py measures on an MI355X: no GPU, no figure"
    text = "\n".join("\n".join(measure(shape)) for shape in SHAPES)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
