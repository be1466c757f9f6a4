#!/usr/bin/env python3
"""Mixup / CutMix inside the one-launch training input step: `sf_clip_batch_mix` in modes 0 (none), 1 (mixup) and 2
(CutMix) against the plain `sf_clip_batch` launch on the same spans.

Bench shape: 8 decoded spans of 64 frames of 256 x 340 uint8 RGB, one allocation per clip; 32 Fast + 8 Slow frames at
crop 224 (alpha 4), stem padding (3, 3); every clip's frames, scale, crop and flip from `train_clip_params` (seeded);
partner of clip b is 7 - b; mixup at lam = 0.3, CutMix with the box of lam = 0.5 around the centre.
What is timed is the LAUNCH alone: tables uploaded and output buffers allocated beforehand, REPS launches between two HIP
events.  Every arm warmed up, then ROUNDS rounds in which the arms alternate; the figure is the median round, the
spread its min .. max.  Bytes: what the launch must write (both pathways) and the uint8 taps it reads at least once
(4 taps x 3 B per output pixel and sampled clip, an upper bound: neighbouring pixels share taps in cache).  Clocks not
pinned.  usage: tools/microbench/mix_batch_bench.py [out.txt]"""
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

B, T_SPAN, H, W, N_FAST, CROP, ALPHA, PAD = 8, 64, 256, 340, 32, 224, 4, (3, 3)
ROUNDS, REPS = 15, 20
MEAN, STD = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225]


def main():
    assert torch.cuda.is_available(), "mix_batch_bench.py measures on an MI355X: no GPU, no figure"
    cfg = get_cfg()
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.DATA.TRAIN_CROP_SIZE = N_FAST, 2, CROP
    cfg.MULTIGRID.DEFAULT_S = 224
    random.seed(1)
    np.random.seed(1)
    videos = [torch.randint(0, 256, (T_SPAN, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    samples = [ds.train_clip_params(cfg, T_SPAN, H, W) for _ in range(B)]
    slow_idx = ds.slow_frame_indices(N_FAST, ALPHA)
    n_slow = slow_idx.numel()
    ph, pw = PAD
    wp = CROP + 2 * pw
    fast = torch.empty((B, N_FAST, CROP + 2 * ph, wp, 4), dtype=torch.float32, device="cuda")
    slow = torch.empty((B, n_slow, CROP + 2 * ph, wp, 4), dtype=torch.float32, device="cuda")
    base = ds.batch_table(videos, samples, slow_idx)
    partner = tuple(B - 1 - b for b in range(B))
    side = int(CROP * np.sqrt(0.5))
    lo = (CROP - side) // 2
    mixes = [("mix, mode 0 (none)", ds.MixParams(partner, ds.MIX_NONE, 1.0, (0, 0, 0, 0))),
             ("mix, mode 1 (mixup)", ds.MixParams(partner, ds.MIX_MIXUP, 0.3, (0, 0, 0, 0))),
             ("mix, mode 2 (CutMix)", ds.MixParams(partner, ds.MIX_CUTMIX, 1.0 - side * side / float(CROP * CROP),
                                                   (lo, lo, lo + side, lo + side)))]
    base_dev = base.cuda()
    arms = [("sf_clip_batch", lambda: sfhip.clip_batch(base, base_dev, n_slow, CROP, MEAN, STD, fast, slow, ph=ph,
                                                       pw=pw))]
    for name, mix in mixes:
        host = torch.cat([base, ds.mix_rows(mix).flatten()]).contiguous()
        dev = host.cuda()
        arms.append(("sf_clip_batch_mix, " + name[5:], lambda host=host, dev=dev: sfhip.clip_batch_mix(
            host, dev, n_slow, CROP, MEAN, STD, fast, slow, ph=ph, pw=pw)))
    # the outputs must not change: mode 0 writes the plain launch's bits
    arms[0][1]()
    want = (fast.clone(), slow.clone())
    arms[1][1]()
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
            times[name].append(e0.elapsed_time(e1) * 1e3 / REPS)  # us per launch
    written = (fast.numel() + slow.numel()) * 4
    taps = B * N_FAST * CROP * CROP * 4 * 3
    med = {n: statistics.median(t) for n, t in times.items()}
    lines = ["%d spans of %d x %d x %d x 3 uint8, %d + %d frames at crop %d, pad %s: %.1f MB written per launch, at most "
             "%.1f MB of uint8 taps per sampled clip; mode 0 bitwise equal to sf_clip_batch: %s; HIP events around %d "
             "launches, median of %d alternating rounds (min .. max)" % (
                 B, T_SPAN, H, W, N_FAST, n_slow, CROP, PAD, written / 1e6, taps / 1e6, same, REPS, ROUNDS)]
    for name, _ in arms:
        ts = times[name]
        lines.append("%-38s %8.1f us (%7.1f .. %7.1f)  %5.2fx of sf_clip_batch  %5.2f TB/s of the bytes written" % (
            name, med[name], min(ts), max(ts), med[name] / med["sf_clip_batch"], written / med[name] / 1e6))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
