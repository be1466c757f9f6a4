#!/usr/bin/env python3
"""Multi-view testing of one video (tools/test_net.py's protocol): the per-clip input path against the one-launch view
sampler, and the host test meter against the device one.

Video: 300 frames of 256 x 340 uint8 RGB; 10 x 3 views of 32 frames, alpha = 4, crop 256, stem padding (3, 3).
Input arms (each produces the [slow, fast] PackedClips of all 30 views):
  per-clip          gather the 30 clips (index_select), then `gpu_input_step` over them: 60 `sf_clip_prologue` launches
  per-clip, gathered the same with the 30 clips gathered beforehand (the gathers are not timed)
  one launch        `gpu_test_views`: one table upload + one `sf_clip_views` launch
Meter arms (one update of 30 predictions x 400 classes, 100 videos, predictions on the GPU):
  TestMeter(cpu)    the host meter: one device-to-host copy per batch
  TestMeter(cuda)   the same class with its accumulators on the device (torch index ops)
  DeviceTestMeter   one `sf_ensemble_update` launch
Method: every arm warmed up, then ROUNDS rounds in which the arms alternate; an arm's round is REPS calls between two
device synchronisations on the host clock (so the host's launch work counts, which is what the one-launch form
removes), the figure is the median round, the spread its min .. max.  C-ABI calls per arm from sfhip.CALLS.  Clocks
not pinned.  usage: tools/microbench/views_bench.py [out.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import torch  # noqa: E402
import sfhip  # noqa: E402
from slowfast.config.defaults import get_cfg  # noqa: E402
from slowfast.datasets import utils as ds  # noqa: E402
from slowfast.utils.meters import DeviceTestMeter, TestMeter  # noqa: E402

T_TOTAL, H, W, CROP, N_FRAMES, ALPHA, PAD = 300, 256, 340, 256, 32, 4, (3, 3)
ROUNDS, REPS, METER_REPS = 9, 5, 50
MEAN, STD = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225]


def alternate(arms, reps):
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
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps)
    return times, calls


def report(title, arms, times, calls, base):
    lines = [title]
    med = {n: statistics.median(times[n]) for n, _ in arms}
    for name, _ in arms:
        ts = times[name]
        lines.append("%-28s %9.1f us (%8.1f .. %8.1f)  %3d C-ABI calls  %5.2fx of %s" % (
            name, med[name] * 1e6, min(ts) * 1e6, max(ts) * 1e6, calls[name], med[base] / med[name], base))
    return lines


def main():
    assert torch.cuda.is_available(), "views_bench.py measures on an MI355X: no GPU, no figure"
    cfg = get_cfg()
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.DATA.TEST_CROP_SIZE = N_FRAMES, 2, CROP
    cfg.TEST.NUM_ENSEMBLE_VIEWS, cfg.TEST.NUM_SPATIAL_CROPS = 10, 3
    video = torch.randint(0, 256, (T_TOTAL, H, W, 3), dtype=torch.uint8, device="cuda")
    views = ds.test_view_params(cfg, T_TOTAL, H, W)
    params = [p for _, p in views]
    frame_idx = [f.cuda() for f, _ in views]
    gathered = [video.index_select(0, f).contiguous() for f in frame_idx]

    def per_clip():
        clips = [video.index_select(0, f) for f in frame_idx]
        return ds.gpu_input_step(clips, params, MEAN, STD, ALPHA, pad=PAD)

    arms = [("per-clip", per_clip),
            ("per-clip, gathered", lambda: ds.gpu_input_step(gathered, params, MEAN, STD, ALPHA, pad=PAD)),
            ("one launch", lambda: ds.gpu_test_views(video, views, MEAN, STD, ALPHA, pad=PAD))]
    a, b = per_clip(), ds.gpu_test_views(video, views, MEAN, STD, ALPHA, pad=PAD)
    same = all(torch.equal(x.buf.view(torch.int32), y.buf.view(torch.int32)) for x, y in zip(a, b))
    out_mb = sum(x.buf.numel() for x in b) * 4 / 1e6
    del a, b
    times, calls = alternate(arms, REPS)
    lines = report("input step: %d views of %d frames from a %d x %d x %d video, crop %d, alpha %d, %.0f MB written; "
                   "outputs bitwise equal: %s; median of %d alternating rounds of %d calls (min .. max)" % (
                       len(views), N_FRAMES, T_TOTAL, H, W, CROP, ALPHA, out_mb, same, ROUNDS, REPS),
                   arms, times, calls, "per-clip")

    n_videos, n_cls, n_clips = 100, 400, len(views)
    preds = torch.randn(n_clips, n_cls, device="cuda").softmax(1)
    labels = torch.full((n_clips,), 7, device="cuda")
    clip_ids = torch.arange(n_clips, device="cuda") + 5 * n_clips
    meters = [("TestMeter(cpu)", TestMeter(n_videos, n_clips, n_cls, 1)),
              ("TestMeter(cuda)", TestMeter(n_videos, n_clips, n_cls, 1, device="cuda")),
              ("DeviceTestMeter", DeviceTestMeter(n_videos, n_clips, n_cls, 1))]
    marms = [(name, (lambda m: lambda: m.update_stats(preds, labels, clip_ids))(m)) for name, m in meters]
    mtimes, mcalls = alternate(marms, METER_REPS)
    lines += report("meter update: %d predictions x %d classes into %d videos; median of %d alternating rounds of %d "
                    "updates (min .. max)" % (n_clips, n_cls, n_videos, ROUNDS, METER_REPS),
                    marms, mtimes, mcalls, "TestMeter(cpu)")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
