#!/usr/bin/env python3
"""The streaming demo's per-frame work around the forward (tools/demo_net.py:160-305): the device frame ring against a
torch restatement of the reference's host path.

Stream: 720 x 1280 uint8 BGR frames, DATA.TEST_CROP_SIZE 256 (-> 256 x 455), S = 64 (NUM_FRAMES 32 x SAMPLING_RATE 2),
alpha 4, stem padding (3, 3), 400 classes.  The forward itself is not part of either arm.
Arms (each is what one incoming frame costs once the buffer is full):
  reference host path  the S scaled float32 frames are already in a list (the reference's cv2.resize of the new frame
                       is not timed: cv2 is not part of this project); torch.stack of the list, tensor_normalize (no
                       /255: float input), permute, the two index_selects, .cuda() of both pathways, then
                       torch.nonzero(preds > 0.1).reshape(-1).cpu() on device predictions
  device ring          StreamingDemo's three library calls: DeviceFrameRing.push of a host frame (pinned staging,
                       one 2.8 MB upload, sf_stream_push), window() (sf_stream_window), sf_label_select and the copy
                       of its row to the host
Method: every arm warmed up, then ROUNDS rounds in which the arms alternate; an arm's round is its REPS calls between
two device synchronisations on the host clock, the figure is the median round, the spread its min .. max.
The copy kernel alone: REPS launches between two device events, bytes from the shapes (16 B read per Fast pixel, 16 B
written per Fast and per Slow pixel) over the median time, against the 8 TB/s HBM peak.  Clocks not pinned.
usage: tools/microbench/stream_demo.py [out.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import sfhip  # noqa: E402
from slowfast.config.defaults import get_cfg  # noqa: E402
from slowfast.utils import stream  # noqa: E402

H, W, SIZE, N_FRAMES, RATE, ALPHA, PAD, CLASSES = 720, 1280, 256, 32, 2, 4, (3, 3), 400
ROUNDS, REPS = 7, {"reference host path": 2, "device ring": 50}
COPY_REPS = 200
MEAN, STD = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225]
HBM_PEAK = 8.0e12


def main():
    assert torch.cuda.is_available(), "stream_demo.py measures on an MI355X: no GPU, no figure"
    cfg = get_cfg()
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.SLOWFAST.ALPHA, cfg.MODEL.ARCH = N_FRAMES, RATE, ALPHA, "slowfast"
    S = N_FRAMES * RATE
    new_h, new_w = stream.demo_scaled_size(SIZE, H, W)
    wp = (new_w + 2 * PAD[1] + 1) // 2 * 2
    fast_pos, slow_pos = stream.demo_window_indices(cfg)
    rs = np.random.RandomState(3)
    preds = torch.rand(1, CLASSES, device="cuda") * 0.12  # a handful of classes above 0.1
    thr = torch.tensor(0.1)

    # the reference's state: a list of S scaled float32 frames (0 .. 255), as cv2_transform.scale returns them
    held = [torch.from_numpy(rs.randint(0, 256, (new_h, new_w, 3)).astype(np.float32)) for _ in range(S)]
    mean, std = torch.tensor(MEAN), torch.tensor(STD)

    def reference():
        inputs = (torch.stack(held) - mean) / std
        inputs = inputs.permute(3, 0, 1, 2).unsqueeze(0)
        fast = torch.index_select(inputs, 2, fast_pos)
        slow = torch.index_select(fast, 2, slow_pos)
        out = [slow.cuda(non_blocking=True), fast.cuda(non_blocking=True)]
        ids = torch.nonzero(preds.squeeze() > 0.1).reshape(-1).cpu()
        held.append(held.pop(0))
        return out, ids

    ring = stream.DeviceFrameRing(SIZE, H, W, MEAN, STD, S, pad=PAD, wp=wp)
    fidx = fast_pos.to(device="cuda", dtype=torch.int32)
    sidx = slow_pos.to(device="cuda", dtype=torch.int32)
    frames = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(4)]
    for i in range(S):
        ring.push(frames[i % 4])
    rows = torch.empty((1, 2 + CLASSES), dtype=torch.int32, device="cuda")
    rows_host = torch.empty((1, 2 + CLASSES), dtype=torch.int32).pin_memory()
    turn = [0]

    def device():
        turn[0] += 1
        ring.push(frames[turn[0] % 4])
        out = ring.window(fidx, sidx)
        sfhip.label_select(preds, 0.1, rows)
        rows_host.copy_(rows, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        n = int(rows_host[0, 0])
        return out, rows_host[0, 2:2 + n]

    arms = [("reference host path", reference), ("device ring", device)]
    calls = {}
    for name, fn in arms:
        fn()
        c0 = sfhip.CALLS
        _, ids = fn()
        calls[name] = sfhip.CALLS - c0
        assert ids.tolist() == torch.nonzero(preds[0].cpu() > thr).reshape(-1).tolist(), name
    torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for _ in range(ROUNDS):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS[name]):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / REPS[name])
    med = {n: statistics.median(times[n]) for n, _ in arms}
    lines = ["per-frame cost around the forward: %d x %d BGR stream, size %d -> %d x %d, S = %d, %d fast + %d slow frames, "
             "%d classes; median of %d alternating rounds (min .. max)" % (
                 H, W, SIZE, new_h, new_w, S, N_FRAMES, slow_pos.numel(), CLASSES, ROUNDS)]
    for name, _ in arms:
        ts = times[name]
        lines.append("%-22s %10.1f us (%9.1f .. %9.1f)  %2d calls per round  %d C-ABI calls  %6.2fx of the reference" % (
            name, med[name] * 1e6, min(ts) * 1e6, max(ts) * 1e6, REPS[name], calls[name],
            med["reference host path"] / med[name]))

    # the copy kernel alone, device time
    plane = (new_h + 2 * PAD[0]) * wp
    nbytes = 16 * plane * (2 * N_FRAMES + slow_pos.numel())
    for _ in range(10):
        ring.window(fidx, sidx)
    ts = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(COPY_REPS):
            ring.window(fidx, sidx)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3 / COPY_REPS)
    t = statistics.median(ts)
    lines.append("sf_stream_window alone: %.1f MB moved per launch (%.1f read + %.1f written), %.1f us per launch in a train "
                 "of %d (min %.1f .. max %.1f over %d rounds, device events): %.2f TB/s, %.0f %% of the %.0f TB/s HBM peak"
                 % (nbytes / 1e6, 16 * plane * N_FRAMES / 1e6, 16 * plane * (N_FRAMES + slow_pos.numel()) / 1e6, t * 1e6,
                    COPY_REPS, min(ts) * 1e6, max(ts) * 1e6, ROUNDS, nbytes / t / 1e12, 100 * nbytes / t / HBM_PEAK,
                    HBM_PEAK / 1e12))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
