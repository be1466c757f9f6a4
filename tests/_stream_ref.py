"""Restatements for the streaming-demo tests: the reference's frame-list loop (tools/demo_net.py:160-305), its box
scaling (cv2_transform.scale_boxes), the window gather and a float64 version of one pushed frame."""
import math

import numpy as np
import torch

MEAN3, STD3 = [0.45, 0.40, 0.50], [0.225, 0.25, 0.2]


def reference_loop(n_pushes, S, hop):
    """The reference's loop over frames numbered 0 .. n_pushes-1 with a literal Python list: append, infer when the
    list holds S frames, then frames.pop(0) (hop 1) or frames = [] (hop S).  -> [(push number, [frame numbers])]."""
    assert hop in (1, S)
    frames, fired = [], []
    for n in range(n_pushes):
        if len(frames) != S:
            frames.append(n)
        if len(frames) == S:
            fired.append((n, list(frames)))
            if hop == 1:
                frames.pop(0)
            else:
                frames = []
    return fired


def ref_scale_boxes(size, boxes, height, width):
    """cv2_transform.scale_boxes on a float32 tensor, then demo_net.py:189-192's index column."""
    boxes = torch.as_tensor(boxes, dtype=torch.float32).clone()
    if not ((width <= height and width == size) or (height <= width and height == size)):
        if width < height:
            new_height = int(math.floor((float(height) / width) * size))
            boxes *= float(new_height) / height
        else:
            new_width = int(math.floor((float(width) / height) * size))
            boxes *= float(new_width) / width
    return torch.cat([torch.full((boxes.shape[0], 1), float(0)), boxes], axis=1)


def window_positions(num_frames, sampling_rate, alpha):
    """demo_net.py:204-221 -> (fast positions in the window, slow positions among the fast frames)."""
    S = num_frames * sampling_rate
    fast = torch.linspace(0, S - 1, num_frames).long()
    slow = torch.linspace(0, num_frames - 1, num_frames // alpha).long() if alpha else torch.zeros(0, dtype=torch.long)
    return fast, slow


def gather_window(slots_by_frame, window_frames, fast_pos, slow_pos):
    """The window's pathways from per-frame planes: slots_by_frame[n] is the checked plane of frame number n (a tensor);
    window_frames the S frame numbers of the window, oldest first.  -> (fast [n_fast, ...], slow [n_slow, ...] or None)."""
    fast = torch.stack([slots_by_frame[window_frames[int(i)]] for i in fast_pos])
    slow = fast.index_select(0, slow_pos.to(fast.device)) if slow_pos.numel() else None
    return fast, slow


def push_fp64(frame_bgr, new_h, new_w, mean=MEAN3, std=STD3):
    """One BGR uint8 frame [H, W, 3] (host) -> float64 [3, new_h, new_w] in RGB order: (u / 255 - mean) / std with the
    float32 mean / std the kernel is handed, then F.interpolate(bilinear, align_corners=False) — the restatement of
    tests/test_train_batch_gpu.py."""
    m = torch.tensor(mean, dtype=torch.float32).double()
    s = torch.tensor(std, dtype=torch.float32).double()
    rgb = frame_bgr.cpu().flip(-1)
    x = ((rgb.double() / 255.0 - m) / s).permute(2, 0, 1).unsqueeze(0)
    if (new_h, new_w) != tuple(x.shape[2:]):
        x = torch.nn.functional.interpolate(x, size=(new_h, new_w), mode="bilinear", align_corners=False)
    return x[0]


def frames_u8(n, h, w, seed):
    rs = np.random.RandomState(seed)
    return [torch.from_numpy(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)) for _ in range(n)]
