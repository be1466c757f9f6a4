"""Streaming demo, host side (no GPU): the size rule, the window index tables, the ring's bookkeeping against a
literal restatement of the reference's frame list, and the box scaling."""
import pytest
import torch

import _stream_ref as ref
from slowfast.config.defaults import get_cfg
from slowfast.utils import stream


@pytest.mark.parametrize("size,h,w,want", [
    (40, 20, 28, (40, 56)),
    (16, 48, 32, (24, 16)),
    (16, 16, 24, (16, 24)),  # early return: the short side already has the size
    (24, 24, 24, (24, 24)),  # early return
    (24, 18, 12, (36, 24)),
])
def test_scaled_size(size, h, w, want):
    assert stream.demo_scaled_size(size, h, w) == want


def _cfg(num_frames, sampling_rate, alpha, arch="slowfast"):
    cfg = get_cfg()
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.SLOWFAST.ALPHA, cfg.MODEL.ARCH = num_frames, sampling_rate, alpha, arch
    return cfg


@pytest.mark.parametrize("t,rate,alpha,fast,slow", [
    (4, 2, 2, [0, 2, 4, 7], [0, 7]),
    (16, 2, 4, list(range(0, 30, 2)) + [31], [0, 10, 20, 31]),
    (32, 2, 4, list(range(0, 62, 2)) + [63], [0, 8, 16, 26, 34, 44, 52, 63]),
])
def test_window_indices(t, rate, alpha, fast, slow):
    f, s = stream.demo_window_indices(_cfg(t, rate, alpha))
    assert f.dtype == torch.int64 and s.dtype == torch.int64
    assert f.tolist() == fast
    assert s.numel() == t // alpha
    assert f[s].tolist() == slow  # the slow frames as window positions
    rf, rs = ref.window_positions(t, rate, alpha)
    assert f.tolist() == rf.tolist() and s.tolist() == rs.tolist()
    f1, s1 = stream.demo_window_indices(_cfg(t, rate, alpha, arch="slow"))
    assert f1.tolist() == fast and s1.numel() == 0 and s1.dtype == torch.int64
    with pytest.raises(NotImplementedError, match="Model arch x3d is not in"):
        stream.demo_window_indices(_cfg(t, rate, alpha, arch="x3d"))


@pytest.mark.parametrize("hop", [1, 8])
def test_schedule_matches_the_reference_list(hop):
    S, n = 8, 3 * 8 + 1
    want = ref.reference_loop(n, S, hop)
    slots = stream.RingSchedule(S)       # the ring's own count: which slot a frame goes to
    sched = stream.RingSchedule(S, hop)  # the demo's count: when a window fires
    held = {}                            # slot -> frame number
    got = []
    for k in range(n):
        slot = slots.push()
        assert slot == k % S
        held[slot] = k
        sched.push()
        assert sched.full == (k >= S - 1)
        if sched.fires:
            assert sched.window_frames() == [held[(sched.head + i) % S] for i in range(S)]  # what the slots hold
            got.append((k, sched.window_frames()))
    assert got == want
    assert [k for k, _ in got] == (list(range(S - 1, n)) if hop == 1 else [7, 15, 23])
    for bad in ((0, 1), (8, 0), (8, 9)):
        with pytest.raises(ValueError):
            stream.RingSchedule(*bad)


@pytest.mark.parametrize("size,h,w", [(16, 20, 28), (16, 28, 20), (16, 16, 24)])  # landscape, portrait, early return
def test_boxes(size, h, w):
    boxes = [[1.5, 2.25, 9.0, 11.75], [0.0, 3.0, 19.5, 15.0]]
    got = stream.demo_boxes(size, boxes, h, w)
    want = ref.ref_scale_boxes(size, boxes, h, w)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 5)
    assert torch.equal(got, want)
    assert got[:, 0].tolist() == [0.0, 0.0]
    if (h, w) == (16, 24):
        assert got[:, 1:].tolist() == boxes
    else:
        assert not torch.equal(got[:, 1:], torch.tensor(boxes))
    none = stream.demo_boxes(size, torch.zeros(0, 4), h, w)
    assert tuple(none.shape) == (0, 5) and none.dtype == torch.float32


def test_labels_for():
    names = ["a", "b", "c", "d"]
    assert stream.labels_for([1, 3], names) == ["b", "d"]
    assert stream.labels_for([], names) == ["Unknown"]
    assert stream.labels_for(torch.tensor([2]), names) == ["c"]


def test_no_cpu_fallback():
    import sfhip
    for name in ("sf_stream_push", "sf_stream_window", "sf_label_select"):
        assert name in sfhip._SIGNATURES
    ring = torch.zeros(8, 16, 22, 4)
    with pytest.raises(sfhip.SfhipError):
        sfhip.stream_push(torch.zeros(20, 28, 3, dtype=torch.uint8), ring, 0, (16, 22), ref.MEAN3, ref.STD3)
    with pytest.raises(sfhip.SfhipError):
        sfhip.stream_window(ring, 0, torch.zeros(4, dtype=torch.int32), None, torch.zeros(4, 16, 22, 4))
    with pytest.raises(sfhip.SfhipError):
        sfhip.label_select(torch.zeros(1, 5), 0.1, torch.zeros(1, 7, dtype=torch.int32))
