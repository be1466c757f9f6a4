"""The streaming demo's three kernels on the GPU: sf_stream_push against sf_clip_prologue (equal bits: one device
function) and against float64, sf_stream_window against a gather of the checked slots over a wrapping ring, and
sf_label_select against torch.nonzero / torch.argmax."""
import functools

import numpy as np
import pytest
import torch

import _stream_ref as ref

pytestmark = pytest.mark.gpu

S, N_FAST, ALPHA, PAD = 8, 4, 2, (3, 3)
MEAN3, STD3 = ref.MEAN3, ref.STD3


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _prologue_planes(frames_bgr, size, wp):
    """sf_clip_prologue on the channel-swapped frames as one clip, crop = size: [n, size + 2 ph, wp, 4]."""
    import sfhip
    clip = torch.stack(frames_bgr).flip(-1).contiguous().cuda()
    dst = torch.full((len(frames_bgr), size + 2 * PAD[0], wp, 4), float("nan"), dtype=torch.float32, device="cuda")
    sfhip.clip_prologue(clip, dst, (size, size), (0, 0), size, False, MEAN3, STD3, ph=PAD[0], pw=PAD[1])
    return dst


@pytest.mark.parametrize("size", [24, 20])  # 20 x 20 -> 24 x 24 resampled; -> 20 x 20: the no-resample branch
def test_push_equals_clip_prologue_bitwise(size):
    import sfhip
    frame = ref.frames_u8(1, 20, 20, seed=5)[0]
    wp = size + 2 * PAD[1] + 2  # a pitch tail of two pixels
    want = _prologue_planes([frame], size, wp)[0]
    ring = torch.full((S, size + 2 * PAD[0], wp, 4), float("nan"), dtype=torch.float32, device="cuda")
    sfhip.stream_push(frame.cuda(), ring, 5, (size, size), MEAN3, STD3, ph=PAD[0], pw=PAD[1])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ring[5]).all())  # borders and the pitch tail included
    assert _same_bits(ring[5], want)
    inner = ring[5, PAD[0]:PAD[0] + size, PAD[1]:PAD[1] + size]
    assert bool((inner[..., :3] != 0).any()) and bool((inner[..., 3].contiguous().view(torch.int32) == 0).all())
    outer = ring[5].clone()
    outer[PAD[0]:PAD[0] + size, PAD[1]:PAD[1] + size] = 0
    assert bool((outer.view(torch.int32) == 0).all())  # +0.0 exactly
    others = torch.cat([ring[:5], ring[6:]])
    assert bool(torch.isnan(others).all())


@pytest.mark.parametrize("h,w,size,new_hw", [(20, 28, 40, (40, 56)), (48, 32, 16, (24, 16)), (28, 20, 40, (56, 40))])
def test_push_rectangular_against_float64(h, w, size, new_hw):
    """Scales whose source coordinates are exact in float32 and float64 (0.5, 2.0: weights in quarters), for the reason
    tests/test_train_batch_gpu.py gives; that file's bound, 2e-6.  The frame goes through the ring's pinned staging."""
    from slowfast.utils import stream
    frame = ref.frames_u8(1, h, w, seed=9)[0]
    wp = new_hw[1] + 2 * PAD[1] + 1
    ring = stream.DeviceFrameRing(size, h, w, MEAN3, STD3, S, pad=PAD, wp=wp)
    assert (ring.new_h, ring.new_w) == new_hw
    ring.ring.fill_(float("nan"))
    assert ring.push(frame.numpy()) == 0 and ring.count == 1
    torch.cuda.synchronize()
    plane = ring.ring[0]
    assert bool(torch.isfinite(plane).all()) and bool(torch.isnan(ring.ring[1:]).all())
    got = plane[PAD[0]:PAD[0] + new_hw[0], PAD[1]:PAD[1] + new_hw[1], :3].permute(2, 0, 1).cpu().double()
    want = ref.push_fp64(frame, *new_hw)
    e = float((got - want).abs().max())
    print("sf_stream_push %dx%d -> %dx%d vs float64: max abs %.3e" % (h, w, new_hw[0], new_hw[1], e))
    assert e < 2e-6, e
    with pytest.raises(RuntimeError, match="holds 1 of 8"):
        ring.window(torch.zeros(N_FAST, dtype=torch.int32, device="cuda"))


@functools.lru_cache(maxsize=None)
def _wrapping_stream():
    """2 S + 3 distinct 20 x 20 frames at size 24 and their planes as sf_clip_prologue writes them (the planes
    test_push_equals_clip_prologue_bitwise checks), computed once and left unchanged."""
    frames = ref.frames_u8(2 * S + 3, 20, 20, seed=17)
    wp = 24 + 2 * PAD[1] + 2
    planes = _prologue_planes(frames, 24, wp)
    torch.cuda.synchronize()
    return frames, wp, planes


@pytest.mark.parametrize("single", [False, True])
def test_window_over_a_wrapping_ring(single):
    from slowfast.utils import stream
    frames, wp, planes = _wrapping_stream()
    fast_pos, slow_pos = ref.window_positions(N_FAST, S // N_FAST, None if single else ALPHA)
    assert fast_pos.tolist() == [0, 2, 4, 7] and slow_pos.tolist() == ([] if single else [0, 3])
    fidx = fast_pos.to(device="cuda", dtype=torch.int32)
    sidx = None if single else slow_pos.to(device="cuda", dtype=torch.int32)
    ring = stream.DeviceFrameRing(24, 20, 20, MEAN3, STD3, S, pad=PAD, wp=wp)
    want_windows = dict(ref.reference_loop(len(frames), S, 1))
    heads = set()
    for n, frame in enumerate(frames):
        slot = ring.push(frame)
        assert slot == n % S
        assert _same_bits(ring.ring[slot], planes[n])  # the slot is a checked plane
        if n not in want_windows:
            continue
        heads.add(ring.sched.head)
        out = ring.window(fidx, sidx)
        want_fast, want_slow = ref.gather_window(planes, want_windows[n], fast_pos, slow_pos)
        fast = out[-1]
        assert tuple(fast.buf.shape) == (1, N_FAST, 30, wp, 4) and fast.shape == (1, 3, N_FAST, 24, 24)
        assert (fast.ph, fast.pw, fast.Wp) == (3, 3, wp)
        assert _same_bits(fast.buf[0], want_fast), n
        if single:
            assert len(out) == 1
        else:
            assert len(out) == 2 and tuple(out[0].buf.shape) == (1, 2, 30, wp, 4)
            assert _same_bits(out[0].buf[0], want_slow), n
    assert len(want_windows) == S + 4 and heads == set(range(S))  # the ring wrapped: every head, 0 and non-0
    assert ring.window(fidx, sidx)[-1].buf.data_ptr() == fast.buf.data_ptr()  # the output buffers are reused


def test_window_table_entries_outside_their_range_give_zeros():
    import sfhip
    from slowfast.utils import stream
    frames, wp, planes = _wrapping_stream()
    ring = stream.DeviceFrameRing(24, 20, 20, MEAN3, STD3, S, pad=PAD, wp=wp)
    for frame in frames[:S + 3]:
        ring.push(frame)
    window = list(range(3, S + 3))
    fast_pos, slow_pos = ref.window_positions(N_FAST, S // N_FAST, ALPHA)
    good_fast, good_slow = ref.gather_window(planes, window, fast_pos, slow_pos)
    for bad_fast, bad_slow in (([0, S, 4, 7], [0, 3]), ([0, 2, 4, -1], [0, 3]), ([0, 2, 4, 7], [0, N_FAST]),
                               ([0, 2, 4, 7], [-1, 3]), ([0, S, 4, 7], [1, 3])):
        fast = torch.full((N_FAST, 30, wp, 4), float("nan"), dtype=torch.float32, device="cuda")
        slow = torch.full((2, 30, wp, 4), float("nan"), dtype=torch.float32, device="cuda")
        sfhip.stream_window(ring.ring, ring.sched.head, torch.tensor(bad_fast, dtype=torch.int32, device="cuda"),
                            torch.tensor(bad_slow, dtype=torch.int32, device="cuda"), fast, slow)
        torch.cuda.synchronize()
        zero_fast = [j for j, w in enumerate(bad_fast) if not 0 <= w < S]
        for j in range(N_FAST):
            if j in zero_fast:
                assert bool((fast[j].view(torch.int32) == 0).all()), (bad_fast, j)
            else:
                assert _same_bits(fast[j], good_fast[j]), (bad_fast, j)
        for j, sj in enumerate(bad_slow):
            if not 0 <= sj < N_FAST or sj in zero_fast:
                assert bool((slow[j].view(torch.int32) == 0).all()), (bad_fast, bad_slow, j)
            else:
                assert _same_bits(slow[j], fast[sj]), (bad_fast, bad_slow, j)
        assert _same_bits(good_slow[1], good_fast[3])


THR = 0.5


def _rows(C, seed):
    """Random rows, then: all below the threshold, all above, one value exactly equal to it, ties at the maximum, NaNs
    mixed in, all NaN."""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.rand(C, generator=g) for _ in range(4)]
    rows.append(torch.rand(C, generator=g) * 0.4)
    rows.append(torch.rand(C, generator=g) * 0.4 + 0.55)
    eq = torch.rand(C, generator=g)
    eq[C // 2] = THR
    rows.append(eq)
    tie = torch.rand(C, generator=g) * 0.9
    tie[[C // 3, C - 1, (2 * C) // 3]] = 0.95
    rows.append(tie)
    nan = torch.rand(C, generator=g)
    nan[::3] = float("nan")
    rows.append(nan)
    rows.append(torch.full((C,), float("nan")))
    return torch.stack(rows)


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("C", [1, 3, 64, 65, 201])
def test_label_select(C, R):
    import sfhip
    preds = _rows(C, seed=100 + C).cuda()
    assert preds.shape[0] % R == 0
    SENT = -7
    for r0 in range(0, preds.shape[0], R):
        chunk = preds[r0:r0 + R].contiguous()
        out = torch.full((R, 2 + C), SENT, dtype=torch.int32, device="cuda")
        sfhip.label_select(chunk, THR, out)
        torch.cuda.synchronize()
        for i in range(R):
            row, got = chunk[i], out[i].cpu()
            want = torch.nonzero(row > THR).reshape(-1).cpu()
            count = int(got[0])
            assert count == want.numel(), (C, r0 + i)
            assert got[2:2 + count].tolist() == want.tolist(), (C, r0 + i)
            assert bool((got[2 + count:] == SENT).all()), (C, r0 + i)  # entries past count are left as they were
            if bool(torch.isnan(row).all()):
                assert int(got[1]) == -1 and count == 0
            else:
                clean = torch.where(torch.isnan(row), torch.full_like(row, float("-inf")), row)
                assert int(got[1]) == int(torch.argmax(clean)), (C, r0 + i)
    # the special rows are what they claim to be
    host = preds.cpu()
    assert not bool((host[4] > THR).any()) and bool((host[5] > THR).all())
    assert float(host[6, C // 2]) == THR and int(torch.argmax(host[7])) == C // 3
