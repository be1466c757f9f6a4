#!/usr/bin/env python3
"""The training input step of one batch: the per-clip route against the one-launch form.

Decoded spans: 64 frames of 256 x 340 uint8 RGB each, one allocation per clip; stem padding (3, 3); alpha = 4; every
clip's frames, scale, crop and flip from `train_clip_params` (seeded).  Shapes:
  full size    8 spans, 32 frames at crop 224 (the default schedule's step)
  long cycle   64 spans, 8 frames at crop 158 (MULTIGRID long cycle: 8x the batch, a quarter of the frames,
               LONG_CYCLE_SAMPLING_RATE 8)
Arms (each produces the [slow, fast] PackedClips of the batch):
  per-clip           gather each clip's frames (index_select), then `gpu_input_step`: 2 B `sf_clip_prologue` launches
  per-clip, gathered the same with the clips gathered beforehand (the gathers are not timed)
  one launch         `gpu_train_batch`: one table upload + one `sf_clip_batch` launch, the gather inside the kernel
Method: every arm warmed up, then ROUNDS rounds in which the arms alternate; an arm's round is REPS calls between two
device synchronisations on the host clock (so the host's launch work counts, which is what the one-launch form
removes), the figure is the median round, the spread its min .. max.  C-ABI calls per arm from sfhip.CALLS.  Clocks
not pinned.  usage: tools/microbench/input_batch_bench.py [out.txt]"""
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import sfhip  # noqa: E402
from slowfast.config.defaults import get_cfg  # noqa: E402
from slowfast.datasets import utils as ds  # noqa: E402

T_SPAN, H, W, ALPHA, PAD = 64, 256, 340, 4, (3, 3)
ROUNDS, REPS = 9, 5
MEAN, STD = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225]
# name: (B, DATA.NUM_FRAMES, DATA.TRAIN_CROP_SIZE, MULTIGRID.LONG_CYCLE_SAMPLING_RATE)
SHAPES = [("full size", 8, 32, 224, 0), ("long cycle", 64, 8, 158, 8)]


def alternate(arms):
    """{name: [seconds per call, one per round]} and {name: C-ABI calls per call}."""
    calls = {}
    for name, fn in arms:
        fn()
        c0 = sfhip.CALLS
        fn()
        calls[name] = sfhip.CALLS - c0
    torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for _ in range(ROUNDS):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / REPS)
    return times, calls


def measure(name, B, n_frames, crop, long_rate):
    cfg = get_cfg()
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.DATA.TRAIN_CROP_SIZE = n_frames, 2, crop
    cfg.MULTIGRID.DEFAULT_S, cfg.MULTIGRID.LONG_CYCLE_SAMPLING_RATE = 224, long_rate
    random.seed(1)
    np.random.seed(1)
    videos = [torch.randint(0, 256, (T_SPAN, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    samples = [ds.train_clip_params(cfg, T_SPAN, H, W) for _ in range(B)]
    params = [p for _, p in samples]
    frame_idx = [f.cuda() for f, _ in samples]
    gathered = [v.index_select(0, f).contiguous() for v, f in zip(videos, frame_idx)]

    def per_clip():
        clips = [v.index_select(0, f) for v, f in zip(videos, frame_idx)]
        return ds.gpu_input_step(clips, params, MEAN, STD, ALPHA, pad=PAD)

    def one_launch():
        return ds.gpu_train_batch(videos, samples, MEAN, STD, ALPHA, pad=PAD)

    arms = [("per-clip", per_clip),
            ("per-clip, gathered", lambda: ds.gpu_input_step(gathered, params, MEAN, STD, ALPHA, pad=PAD)),
            ("one launch", one_launch)]
    a, b = per_clip(), one_launch()
    same = all(torch.equal(x.buf.view(torch.int32), y.buf.view(torch.int32)) for x, y in zip(a, b))
    out_mb = sum(x.buf.numel() for x in b) * 4 / 1e6
    del a, b
    times, calls = alternate(arms)
    med = {n: statistics.median(times[n]) for n, _ in arms}
    lines = ["%s: %d spans of %d x %d x %d, %d frames at crop %d, alpha %d, %.0f MB written; outputs bitwise equal: %s; "
             "median of %d alternating rounds of %d calls (min .. max)" % (
                 name, B, T_SPAN, H, W, n_frames, samples[0][1].crop, ALPHA, out_mb, same, ROUNDS, REPS)]
    for arm, _ in arms:
        ts = times[arm]
        lines.append("%-28s %9.1f us (%8.1f .. %8.1f)  %3d C-ABI calls  %5.2fx of per-clip" % (
            arm, med[arm] * 1e6, min(ts) * 1e6, max(ts) * 1e6, calls[arm], med["per-clip"] / med[arm]))
    return lines


def main():
    assert torch.cuda.is_available(), "input_batch_bench.py measures on an MI355X: no GPU, no figure"
    lines = []
    for shape in SHAPES:
        lines += measure(*shape)
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
