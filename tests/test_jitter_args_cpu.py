"""Host side of the colour-jittered input step (sf_frame_grey_means, sf_clip_batch_jitter; sfhip.frame_grey_means,
sfhip.clip_batch_jitter, datasets.utils.jitter_rows / gpu_train_batch_jitter): the binding's rows and every refusal —
decided before any launch, so callable without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

FAKE = 4096  # a non-null, 16-byte aligned "device address": a refused call never dereferences it


def _ds():
    from slowfast.datasets import utils
    return utils


def _bits(v):
    return int(np.array(v, dtype=np.float32).view(np.uint32))


def test_signature_table_has_the_new_symbols():
    import sfhip
    vp, ci, pi = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    want = {"sf_frame_grey_means": (ci, [vp, vp, ci, ci, ci, pi, vp]),
            "sf_clip_batch_jitter": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, pi, vp, vp, ci, ci, ci, vp])}
    for name, sig in want.items():
        assert sfhip._SIGNATURES[name] == sig, name
        assert name in sfhip.EXPORTS and hasattr(sfhip.lib(), name)
    assert sfhip.SF_JITTER_ROW == 3
    assert callable(sfhip.frame_grey_means) and callable(sfhip.clip_batch_jitter)
    assert callable(_ds().gpu_train_batch_jitter) and callable(_ds().jester_clip_params)


def test_jitter_rows_round_trip_float32_bits():
    ds = _ds()
    jit = [ds.ColorJitter(0.4, 1.4, 1.0), None, ds.ColorJitter(0.7234567891234, -1.0, 0.0), (1.1, 0.9, 1.3)]
    rows = ds.jitter_rows(jit)
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (4, 3) and rows.is_contiguous()
    assert bool(((rows >= 0) & (rows <= 0xffffffff)).all())  # the high half is zero
    back = rows.numpy().astype(np.uint32).view(np.float32)
    want = np.array([[0.4, 1.4, 1.0], [0, 0, 0], [0.7234567891234, -1.0, 0.0], [1.1, 0.9, 1.3]], dtype=np.float32)
    assert np.array_equal(back.view(np.uint32), want.view(np.uint32))
    assert rows[0, 2].item() == 0x3f800000 and rows[1].tolist() == [0, 0, 0] and rows[2, 1].item() == 0xbf800000
    for bad in ([ds.ColorJitter(float("nan"), 1, 1)], [ds.ColorJitter(1, float("inf"), 1)], [(1.0, 1.0)],
                [ds.ColorJitter(1, 1, 1e39)]):  # 1e39 is inf as a float32
        with pytest.raises(ValueError, match="jitter_rows"):
            ds.jitter_rows(bad)


def _batch_inputs():
    ds = _ds()
    videos = [torch.zeros(5, 20, 28, 3, dtype=torch.uint8), torch.zeros(8, 24, 24, 3, dtype=torch.uint8)]
    samples = [(torch.tensor([0, 1, 3, 4]), ds.SpatialParams(10, 14, 1, 3, False, 8)),
               (torch.tensor([2, 2, 7, 7]), ds.SpatialParams(24, 24, 16, 0, True, 8))]
    jit = [ds.ColorJitter(0.5, 1.25, 0.75), ds.ColorJitter(1.4, 0.0, 1.0)]
    tab = torch.cat([ds.batch_table(videos, samples, ds.slow_frame_indices(4, 2)), ds.jitter_rows(jit).flatten()])
    return videos, samples, jit, tab.contiguous()


def test_argument_checks_of_both_entries_are_host_only():
    import sfhip
    L = sfhip.lib()
    E = sfhip.SF_EINVAL
    videos, samples, jit, tab = _batch_inputs()
    assert tab.numel() == 2 * 9 + 2 * 4 + 2 + 2 * 3
    JIT0 = 28  # the first jitter row
    m3 = (ctypes.c_float * 3)(0.45, 0.45, 0.45)
    mp = ctypes.cast(m3, ctypes.c_void_p)
    fake = ctypes.c_void_p(FAKE)
    ip = ctypes.POINTER(ctypes.c_int)

    def iptr(addr):
        return ctypes.cast(ctypes.c_void_p(addr), ip) if addr else None

    def clip(tab=tab, table=fake, means=FAKE, fast=fake, slow=fake, B=2, n_fast=4, n_slow=2, crop=8, pw=0, wp=8, mean=mp,
             std=mp):
        host = ctypes.c_void_p(tab.data_ptr()) if tab is not None else None
        return L.sf_clip_batch_jitter(host, table, B, n_fast, n_slow, crop, 0, mean, std, iptr(means), fast, slow, 0, pw,
                                      wp, None)

    def grey(tab=tab, table=fake, means=FAKE, B=2, n_fast=4, n_slow=2):
        host = ctypes.c_void_p(tab.data_ptr()) if tab is not None else None
        return L.sf_frame_grey_means(host, table, B, n_fast, n_slow, iptr(means), None)

    def edited(pos, val):
        bad = tab.clone()
        bad[pos] = val
        return bad

    both = [
        # null pointers, sizes
        dict(tab=None), dict(table=None), dict(means=0), dict(B=0), dict(B=-1), dict(n_fast=0), dict(n_slow=5),
        dict(n_slow=-1), dict(B=65536), dict(n_fast=65536),
        # `means` not 4-byte aligned
        dict(means=FAKE + 1), dict(means=FAKE + 2), dict(means=FAKE + 3),
        # the batch rows: address, T, H, W, scaled extents; a frame index outside the span; the Slow positions
        dict(tab=edited(0, 0)), dict(tab=edited(1, 0)), dict(tab=edited(9 + 2, 0)), dict(tab=edited(3, -28)),
        dict(tab=edited(4, 0)), dict(tab=edited(9 + 5, -24)), dict(tab=edited(6, -1)),
        dict(tab=edited(18 + 3, 5)), dict(tab=edited(18 + 4, -1)), dict(tab=edited(18 + 7, 8)),
        dict(tab=edited(27, 4)), dict(tab=edited(26, -1)), dict(tab=edited(27, 0)), dict(tab=edited(26, 3)),
        # the factor words: NaN, +inf, -inf, a non-zero high half, a negative word — in every column of both rows
        dict(tab=edited(JIT0 + 0, _bits(float("nan")))), dict(tab=edited(JIT0 + 1, _bits(float("inf")))),
        dict(tab=edited(JIT0 + 2, _bits(-float("inf")))), dict(tab=edited(JIT0 + 3, 0x7fc00001)),
        dict(tab=edited(JIT0 + 4, _bits(1.0) + (1 << 32))), dict(tab=edited(JIT0 + 5, -1)),
        dict(tab=edited(JIT0 + 0, 1 << 32)), dict(tab=edited(JIT0 + 5, _bits(1.0) - (1 << 63))),
    ]
    for kw in both:
        assert grey(**kw) == E, kw
        assert clip(**kw) == E, kw
    only_clip = [
        dict(fast=None), dict(crop=0), dict(pw=-1), dict(pw=1), dict(wp=7), dict(mean=None), dict(std=None),
        dict(slow=None),                       # n_slow without slow
        dict(n_slow=0, tab=tab),               # ... and slow without n_slow
        dict(tab=edited(6, 3)), dict(tab=edited(7, 7)), dict(tab=edited(9 + 6, 17)),   # the crop window leaves the frame
        dict(fast=ctypes.c_void_p(FAKE + 4)), dict(slow=ctypes.c_void_p(FAKE + 8)),    # 16-byte stores
    ]
    for kw in only_clip:
        assert clip(**kw) == E, kw
    # the crop window is not the means' business: the same rows pass its host check up to the launch — which a fake
    # address must not reach, so only the refusal list above is called


def test_wrappers_refuse_before_the_gpu_is_needed():
    import sfhip
    ds = _ds()
    videos, samples, jit, tab = _batch_inputs()
    means, fast = torch.zeros((2, 4), dtype=torch.int32), torch.zeros(2, 4, 8, 8, 4)
    with pytest.raises(sfhip.SfhipError):  # no CPU fallback
        sfhip.frame_grey_means(tab, tab, 2, means)
    with pytest.raises(sfhip.SfhipError):
        sfhip.clip_batch_jitter(tab, tab, 2, 8, [0.45] * 3, [0.225] * 3, means, fast)
    with pytest.raises(sfhip.SfhipError):
        ds.gpu_train_batch_jitter(videos, samples, jit, [0.45] * 3, [0.225] * 3, 2)
    with pytest.raises(ValueError, match="jitter factors"):
        ds.gpu_train_batch_jitter(videos, samples, jit + [None], [0.45] * 3, [0.225] * 3, 2)
    gray = [v[..., 0].contiguous() for v in videos]
    with pytest.raises(ValueError, match="RGB"):
        ds.gpu_train_batch_jitter(gray, samples, jit, [0.45], [0.225], 2)
    with pytest.raises(ValueError, match="RGB"):
        ds.gpu_train_batch_jitter([v[..., :1].contiguous() for v in videos], samples, jit, [0.45], [0.225], 2)


@pytest.mark.parametrize("delta", [-1, 1, -6])
def test_table_length_is_checked(monkeypatch, delta):
    """The wrappers hold the table to B * (9 + n_fast + 3) + n_slow words before the C entry sees it (the C ABI cannot
    know the length): a table without its jitter rows, or one word off, is refused.  The tensors pose as device
    tensors so that the length check is what speaks."""
    import sfhip
    videos, samples, jit, tab = _batch_inputs()
    called = []
    monkeypatch.setattr(sfhip, "_call", lambda *a, **k: called.append(a))

    class OnGpu(torch.Tensor):
        is_cuda = True

    means = torch.zeros((2, 4), dtype=torch.int32).as_subclass(OnGpu)
    short = tab[:tab.numel() + delta].contiguous() if delta < 0 else torch.cat([tab, tab[:delta]]).contiguous()
    with pytest.raises(AssertionError):
        sfhip.frame_grey_means(short, short.as_subclass(OnGpu), 2, means)
    assert not called
    sfhip.frame_grey_means(tab, tab.as_subclass(OnGpu), 2, means)  # the right length reaches the call
    assert len(called) == 1 and called[0][0] == "sf_frame_grey_means"
