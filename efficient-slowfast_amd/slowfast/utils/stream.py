"""The streaming demo of the reference (tools/demo_net.py:160-305) with its frame buffer on the GPU.

The reference keeps a Python list of the last S = DATA.NUM_FRAMES * DATA.SAMPLING_RATE scaled frames and, for every
incoming frame once the list is full, stacks, normalises, permutes, index_selects and uploads all of them before the
forward, then reads the labels back through torch.nonzero.  Only the newest frame is new.  Here every frame is uploaded
once as uint8 and scaled / normalised once into a device ring (`sf_stream_push`); a window is one copy launch for both
pathways (`sf_stream_window`) and the labels one launch and one small read-back (`sf_label_select`).

Host side (this file) keeps what is host logic: the size rule of cv2_transform.scale, the two linspace index tables,
the ring's bookkeeping (which slot, when a window fires), the box scaling of cv2_transform.scale_boxes and the label
names.  The person detector (detectron2) and the drawing stay with the caller.

Two departures from the reference, both described in INTEGRATION.md ("Streaming demo"): frames are always divided by
255 before normalisation (the reference does so only when no resize happened), and the resampling is the project's
float bilinear, not cv2.resize's fixed-point uint8 one."""
import collections
import math

import numpy as np
import torch

import sfhip
from slowfast.datasets import utils as ds

LABEL_THRESHOLD = 0.1  # demo_net.py:265 and :293


def demo_scaled_size(size, h, w):
    """cv2_transform.scale's size rule (cv2_transform.py:89-100): the (height, width) of an h x w frame whose short side
    is scaled to `size`; unchanged when the short side already has that size (the early return)."""
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(math.floor((float(h) / w) * size)), size
    return size, int(math.floor((float(w) / h) * size))


def demo_window_indices(cfg):
    """(fast, slow) int64 host tensors as demo_net.py:204-221 composes them: `fast` are the NUM_FRAMES positions
    linspace(0, S-1, NUM_FRAMES).long() in the window of S frames, `slow` the positions
    linspace(0, NUM_FRAMES-1, NUM_FRAMES // ALPHA).long() among the fast frames (empty for a single-pathway arch)."""
    arch = cfg.MODEL.ARCH
    if arch not in cfg.MODEL.SINGLE_PATHWAY_ARCH and arch not in cfg.MODEL.MULTI_PATHWAY_ARCH:
        raise NotImplementedError("Model arch {} is not in {}".format(
            arch, cfg.MODEL.SINGLE_PATHWAY_ARCH + cfg.MODEL.MULTI_PATHWAY_ARCH))
    n = cfg.DATA.NUM_FRAMES
    S = n * cfg.DATA.SAMPLING_RATE
    fast = torch.linspace(0, S - 1, n).long()
    if arch in cfg.MODEL.SINGLE_PATHWAY_ARCH:
        return fast, torch.zeros(0, dtype=torch.long)
    return fast, torch.linspace(0, n - 1, n // cfg.SLOWFAST.ALPHA).long()


def demo_boxes(size, boxes, h, w):
    """Person boxes [n, 4] in display coordinates (h x w) -> the float32 host tensor [n, 5] the detection head takes:
    cv2_transform.scale_boxes (cv2_transform.py:119-132; one factor for all four coordinates, none on the early return)
    and the batch-index column 0 in front (demo_net.py:183-192)."""
    boxes = torch.as_tensor(np.asarray(boxes), dtype=torch.float32).reshape(-1, 4).clone()
    new_h, new_w = demo_scaled_size(size, h, w)
    if (new_h, new_w) != (h, w):
        boxes *= (float(new_h) / h) if w < h else (float(new_w) / w)
    return torch.cat([torch.full((boxes.shape[0], 1), float(0)), boxes], dim=1)


def labels_for(ids, names):
    """The names of one row's selected ids; ["Unknown"] when nothing was selected (demo_net.py:299-302)."""
    out = [names[int(i)] for i in ids]
    return out if out else ["Unknown"]


class RingSchedule(object):
    """The bookkeeping of the reference's frame list (append; infer when it holds S frames; then drop the `hop` oldest:
    hop 1 is `frames.pop(0)`, hop S the commented `frames = []`) for a ring of S slots.  Host integers only."""

    def __init__(self, S, hop=1):
        if S <= 0 or not 1 <= hop <= S:
            raise ValueError("RingSchedule: S must be positive and hop in [1, S], got S=%r hop=%r" % (S, hop))
        self.S, self.hop, self.count = S, hop, 0

    def push(self):
        """Count one frame -> the slot it goes to."""
        slot = self.count % self.S
        self.count += 1
        return slot

    @property
    def full(self):
        return self.count >= self.S

    @property
    def fires(self):
        """Does the reference run the model after the frame just pushed?"""
        return self.full and (self.count - self.S) % self.hop == 0

    @property
    def head(self):
        """The slot of the oldest of the last S frames."""
        return self.count % self.S

    def window_frames(self):
        """The numbers (0-based push order) of the S frames of the current window, oldest first."""
        return list(range(self.count - self.S, self.count))


class DeviceFrameRing(object):
    """The last S scaled, normalised frames of an h x w BGR stream, on the GPU in the stem's PackedClip layout.

    size: DATA.TEST_CROP_SIZE (the short side); mean / std: DATA.MEAN / DATA.STD (RGB order); pad / wp: the stem's
    (ph, pw) and row pitch for the scaled frame (`datasets.utils.stem_input_geometry(model, new_h, new_w)`).
    Everything is allocated here; push() and window() allocate nothing."""

    def __init__(self, size, h, w, mean, std, S, pad=(0, 0), wp=None):
        if not torch.cuda.is_available():
            raise sfhip.SfhipError("DeviceFrameRing: the frame ring lives on an MI355X GPU (no CPU fallback)")
        self.h, self.w, self.S = int(h), int(w), int(S)
        self.new_h, self.new_w = demo_scaled_size(size, self.h, self.w)
        self.ph, self.pw = pad
        self.wp = self.new_w + 2 * self.pw if wp is None else wp
        self.mean, self.std = [float(v) for v in mean], [float(v) for v in std]
        self.sched = RingSchedule(self.S)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.ring = torch.empty((self.S, self.new_h + 2 * self.ph, self.wp, 4), dtype=torch.float32, device=dev)
        self._stage = torch.empty((self.h, self.w, 3), dtype=torch.uint8).pin_memory()
        self._frame = torch.empty((self.h, self.w, 3), dtype=torch.uint8, device=dev)
        self._copied = torch.cuda.Event()  # the staging buffer is free again once its last copy has run
        self._out = {}                     # (n_fast, n_slow) -> (fast, slow): the window's two output buffers

    count = property(lambda self: self.sched.count)

    def push(self, frame):
        """One frame, uint8 [h, w, 3] in BGR order: a numpy array or host tensor (copied through the pinned staging
        buffer, non-blocking) or a device tensor -> its slot, count % S."""
        if isinstance(frame, np.ndarray):
            frame = torch.from_numpy(frame)
        if frame.dtype != torch.uint8 or tuple(frame.shape) != (self.h, self.w, 3):
            raise ValueError("DeviceFrameRing.push: a frame is uint8 [%d, %d, 3], got %s %s" % (
                self.h, self.w, frame.dtype, tuple(frame.shape)))
        if frame.is_cuda:
            dev_frame = frame.contiguous()
        else:
            self._copied.synchronize()  # the previous frame's copy (long done in a running stream)
            self._stage.copy_(frame)
            self._frame.copy_(self._stage, non_blocking=True)
            self._copied.record()
            dev_frame = self._frame
        slot = self.sched.push()
        sfhip.stream_push(dev_frame, self.ring, slot, (self.new_h, self.new_w), self.mean, self.std, ph=self.ph,
                          pw=self.pw)
        return slot

    def window(self, fast_idx, slow_idx=None):
        """[slow, fast] ([fast] without slow positions) PackedClips of batch 1 for the window of the last S frames:
        fast_idx / slow_idx are int32 device tensors (`demo_window_indices`, uploaded once by the caller).  The two
        buffers are reused by every call with the same frame counts."""
        if not self.sched.full:
            raise RuntimeError("DeviceFrameRing.window: the ring holds %d of %d frames" % (self.count, self.S))
        n_fast = fast_idx.numel()
        n_slow = 0 if slow_idx is None else slow_idx.numel()
        if (n_fast, n_slow) not in self._out:
            shape = tuple(self.ring.shape[1:])
            fast = torch.empty((n_fast,) + shape, dtype=torch.float32, device=self.ring.device)
            slow = torch.empty((n_slow,) + shape, dtype=torch.float32, device=self.ring.device) if n_slow else None
            self._out[(n_fast, n_slow)] = (fast, slow)
        fast, slow = self._out[(n_fast, n_slow)]
        sfhip.stream_window(self.ring, self.sched.head, fast_idx, slow_idx if n_slow else None, fast, slow)
        out = [sfhip.PackedClip(fast.unsqueeze(0), 3, self.new_h, self.new_w, self.ph, self.pw)]
        return out if slow is None else [sfhip.PackedClip(slow.unsqueeze(0), 3, self.new_h, self.new_w, self.ph,
                                                          self.pw)] + out


DemoLabels = collections.namedtuple("DemoLabels", "ids argmax")
DemoLabels.__doc__ = """What one window of the demo yields: `ids` — per row of the predictions (one row for
classification, one per box for detection) the list of class indices above the threshold, ascending; `argmax` — per row
the first maximal class (-1 for a row of NaNs).  Both empty for a detection window without boxes."""


class StreamingDemo(object):
    """demo_net.py's loop body for one stream: push(frame) per incoming frame.

    cfg: DATA.NUM_FRAMES, DATA.SAMPLING_RATE, DATA.TEST_CROP_SIZE, DATA.MEAN / STD, SLOWFAST.ALPHA, MODEL.ARCH,
    DETECTION.ENABLE; model: the built model in eval mode on the current GPU; hop: frames dropped after a window (1:
    the reference's `frames.pop(0)`, S: its commented "empty the buffer").  The ring is built on the first frame, from
    its height and width.  After a window fired, `last_inputs` / `last_preds` hold what the model was given and gave."""

    def __init__(self, cfg, model, hop=1, threshold=LABEL_THRESHOLD):
        self.cfg, self.model, self.threshold = cfg, model, float(threshold)
        self.S = cfg.DATA.NUM_FRAMES * cfg.DATA.SAMPLING_RATE
        self.sched = RingSchedule(self.S, hop)
        self.detection = bool(cfg.DETECTION.ENABLE)
        fast, slow = demo_window_indices(cfg)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.fast_idx = fast.to(device=dev, dtype=torch.int32)  # uploaded once
        self.slow_idx = slow.to(device=dev, dtype=torch.int32) if slow.numel() else None
        self.ring = None
        self.last_inputs = self.last_preds = None
        self._rows = self._rows_host = None

    def _select(self, preds):
        """sf_label_select on preds [R, C] and the one small device-to-host copy -> DemoLabels."""
        R, C = preds.shape
        if self._rows is None or self._rows.shape[0] < R or self._rows.shape[1] != 2 + C:
            self._rows = torch.empty((R, 2 + C), dtype=torch.int32, device=preds.device)
            self._rows_host = torch.empty((R, 2 + C), dtype=torch.int32).pin_memory()
        rows, host = self._rows[:R], self._rows_host[:R]
        sfhip.label_select(preds, self.threshold, rows)
        host.copy_(rows, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        table = host.tolist()
        return DemoLabels([r[2:2 + r[0]] for r in table], [r[1] for r in table])

    def push(self, frame, boxes=None):
        """One incoming frame (uint8 [h, w, 3], BGR).  None while the ring fills and between hops; otherwise the
        DemoLabels of the window ending at this frame.  With DETECTION.ENABLE `boxes` are the person boxes [n, 4] in
        display (frame) coordinates; no boxes: an empty result and no forward, as the reference does."""
        if self.ring is None:
            h, w = int(frame.shape[0]), int(frame.shape[1])
            size = self.cfg.DATA.TEST_CROP_SIZE
            new_h, new_w = demo_scaled_size(size, h, w)
            ph, pw, wp = ds.stem_input_geometry(self.model, new_h, new_w)
            self.ring = DeviceFrameRing(size, h, w, self.cfg.DATA.MEAN, self.cfg.DATA.STD, self.S, pad=(ph, pw), wp=wp)
        self.ring.push(frame)
        self.sched.push()
        if not self.sched.fires:
            return None
        if self.detection:
            if boxes is None:
                raise ValueError("StreamingDemo.push: DETECTION.ENABLE needs the person boxes of the window")
            bboxes = demo_boxes(self.cfg.DATA.TEST_CROP_SIZE, boxes, self.ring.h, self.ring.w)
            if bboxes.shape[0] == 0:
                self.last_inputs = self.last_preds = None
                return DemoLabels([], [])
        inputs = self.ring.window(self.fast_idx, self.slow_idx)
        with torch.no_grad():
            if self.detection:
                preds = self.model(inputs, bboxes.to(self.fast_idx.device, non_blocking=True))
            else:
                preds = self.model(inputs)
        self.last_inputs, self.last_preds = inputs, preds
        return self._select(preds.reshape(preds.shape[0], -1).contiguous())
