"""Multi-view testing on the GPU, op level: the one-launch view sampler (sf_clip_views / sf_clip_views_gray) against
the per-clip path (sfhip.clip_prologue view by view and pathway by pathway) — equal bits, because the pixel arithmetic
is one device function — with owned-memory margins, its argument checks, and sf_ensemble_update against the host
TestMeter (bitwise for sum: the batch is folded in the host loop's order)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CROP, N_FAST = 16, 8
MEAN3, STD3 = [0.45, 0.40, 0.50], [0.225, 0.25, 0.2]
SENTINEL, MARGIN = 12345.0, 64  # floats either side of each output buffer (256 B: the buffers stay 16-byte aligned)

# name: (T_total, H, W, gray, V, alpha, reverse, (ph, pw), Wp, flipped views)
CASES = {
    "rgb_landscape_a4_flip": (40, 20, 28, False, 9, 4, False, (3, 3), None, (1, 4)),
    "rgb_portrait_a8_reverse_oddpitch": (40, 28, 20, False, 9, 8, True, (1, 1), CROP + 2 + 3, ()),
    "rgb_noresample_v1": (40, 16, 16, False, 1, 4, False, (0, 0), None, ()),
    "rgb_clamped_frames": (10, 20, 28, False, 9, 4, False, (3, 3), None, ()),
    "rgb_single_pathway": (40, 20, 28, False, 9, None, False, (3, 3), None, (0,)),
    "gray_landscape_a4_vec_flip": (40, 20, 28, True, 9, 4, False, (3, 3), 24, (2,)),
    "gray_portrait_a8_scalar_pitch": (40, 28, 20, True, 9, 8, False, (3, 3), 23, (5,)),  # 23 floats: no 16-byte rows
    "gray_noresample_v1_clamped": (10, 16, 16, True, 1, 4, False, (0, 0), None, ()),
}


def _cfg():
    from slowfast.config.defaults import get_cfg
    cfg = get_cfg()
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.DATA.TEST_CROP_SIZE = N_FAST, 2, CROP
    cfg.TEST.NUM_ENSEMBLE_VIEWS, cfg.TEST.NUM_SPATIAL_CROPS = 3, 3
    return cfg


def _setup(name):
    from slowfast.datasets import utils as ds
    t, h, w, gray, v, alpha, reverse, pad, wp, flipped = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    video = torch.from_numpy(rs.randint(0, 256, (t, h, w) if gray else (t, h, w, 3)).astype(np.uint8)).cuda()
    views = ds.test_view_params(_cfg(), t, h, w)[:v]
    views = [(f, p._replace(flip=True) if i in flipped else p) for i, (f, p) in enumerate(views)]
    mean, std = ([0.45], [0.225]) if gray else (MEAN3, STD3)
    return ds, video, views, mean, std, alpha, reverse, pad, (CROP + 2 * pad[1] if wp is None else wp), (1 if gray else 4)


def _guarded(shape):
    """A NaN-filled buffer of `shape` between two sentinel margins -> (whole allocation, the buffer's view)."""
    n = int(np.prod(shape))
    whole = torch.full((MARGIN + n + MARGIN,), SENTINEL, dtype=torch.float32, device="cuda")
    whole[MARGIN:MARGIN + n] = float("nan")
    return whole, whole[MARGIN:MARGIN + n].view(shape)


def _margins_intact(whole):
    return bool((whole[:MARGIN] == SENTINEL).all()) and bool((whole[-MARGIN:] == SENTINEL).all())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_view_sampler_equals_per_clip_path_bitwise(name):
    import sfhip
    ds, video, views, mean, std, alpha, reverse, (ph, pw), wp, cpad = _setup(name)
    V = len(views)
    slow_idx = ds.slow_frame_indices(N_FAST, alpha) if alpha is not None else torch.zeros(0, dtype=torch.long)
    n_slow = slow_idx.numel()
    hp = CROP + 2 * ph
    fast_all, fast = _guarded((V, N_FAST, hp, wp, cpad))
    slow_all, slow = _guarded((V, n_slow, hp, wp, cpad)) if n_slow else (None, None)
    table_host = ds.view_table(views, slow_idx)
    sfhip.clip_views(video, table_host, table_host.cuda(), n_slow, CROP, mean, std, fast, slow, reverse=reverse,
                     ph=ph, pw=pw)
    torch.cuda.synchronize()
    assert _margins_intact(fast_all) and (slow_all is None or _margins_intact(slow_all))
    assert not bool(torch.isnan(fast).any()) and (slow is None or not bool(torch.isnan(slow).any()))  # all written
    # the per-clip path: one gathered clip per view, one launch per pathway
    si = slow_idx.to(device="cuda", dtype=torch.int32)
    for v, (frames, p) in enumerate(views):
        clip = video.index_select(0, frames.cuda()).contiguous()
        want = torch.full((N_FAST, hp, wp, cpad), float("nan"), device="cuda")
        sfhip.clip_prologue(clip, want, (p.new_h, p.new_w), (p.y, p.x), CROP, p.flip, mean, std, reverse=reverse,
                            ph=ph, pw=pw)
        assert _same_bits(fast[v], want), (name, v, "fast")
        if n_slow:
            want = torch.full((n_slow, hp, wp, cpad), float("nan"), device="cuda")
            sfhip.clip_prologue(clip, want, (p.new_h, p.new_w), (p.y, p.x), CROP, p.flip, mean, std, frame_idx=si,
                                reverse=reverse, ph=ph, pw=pw)
            assert _same_bits(slow[v], want), (name, v, "slow")
    # gpu_test_views is the same launch behind the dataset-level interface
    packed = ds.gpu_test_views(video, views, mean, std, alpha, reverse_input_channel=reverse, pad=(ph, pw), wp=wp)
    assert len(packed) == (2 if n_slow else 1) and _same_bits(packed[-1].buf, fast)
    assert packed[-1].shape == (V, cpad if cpad == 1 else 3, N_FAST, CROP, CROP)
    if n_slow:
        assert _same_bits(packed[0].buf, slow) and packed[0].buf.shape[1] == n_slow


def test_clamped_indices_repeat_the_last_frame():
    """T_total = 10 under a 16-frame span: frames 5..7 of every view are the video's last frame."""
    ds, video, views, mean, std, alpha, reverse, pad, wp, _ = _setup("rgb_clamped_frames")
    assert views[0][0].tolist() == [0, 2, 4, 6, 8, 9, 9, 9]
    slow, fast = ds.gpu_test_views(video, views, mean, std, alpha, pad=pad, wp=wp)
    assert _same_bits(fast.buf[:, 5], fast.buf[:, 6]) and _same_bits(fast.buf[:, 6], fast.buf[:, 7])
    assert not _same_bits(fast.buf[:, 4], fast.buf[:, 5])
    assert _same_bits(slow.buf[:, 1], fast.buf[:, 7])  # slow_frame_indices(8, 4) = [0, 7]


def test_view_sampler_argument_errors_leave_the_output_untouched():
    import sfhip
    ds, video, views, mean, std, alpha, reverse, (ph, pw), wp, cpad = _setup("rgb_landscape_a4_flip")
    L = sfhip.lib()
    slow_idx = ds.slow_frame_indices(N_FAST, alpha)
    tab = ds.view_table(views, slow_idx)
    tab_dev = tab.cuda()
    fast = torch.full((9, N_FAST, CROP + 2 * ph, wp, 4), SENTINEL, device="cuda")
    slow = torch.full((9, 2, CROP + 2 * ph, wp, 4), SENTINEL, device="cuda")
    m3 = ctypes.cast((ctypes.c_float * 3)(*MEAN3), ctypes.c_void_p)
    s3 = ctypes.cast((ctypes.c_float * 3)(*STD3), ctypes.c_void_p)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(video_p=p(video), host=tab, dev=p(tab_dev), fast_p=p(fast), slow_p=p(slow), V=9, n_slow=2):
        return L.sf_clip_views(video_p, 40, 20, 28, p(host), dev, V, N_FAST, n_slow, CROP, 0, m3, s3, fast_p, slow_p, ph,
                               pw, wp, stream)

    outside = tab.clone()
    outside[5 * 2 + 3] = 7  # view 2: x0 + crop = 23 > new_w = 22
    for kw in (dict(video_p=None), dict(dev=None), dict(fast_p=None), dict(V=0), dict(host=outside), dict(n_slow=9)):
        assert call(**kw) == sfhip.SF_EINVAL, kw
    torch.cuda.synchronize()
    assert bool((fast == SENTINEL).all()) and bool((slow == SENTINEL).all())
    assert call() == 0  # the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert not bool((fast == SENTINEL).any()) and not bool((slow == SENTINEL).any())
    gfast = torch.full((9, N_FAST, CROP, CROP, 1), SENTINEL, device="cuda")
    gvideo = video[..., 0].contiguous()
    for V, host in ((0, tab), (9, outside)):
        assert L.sf_clip_views_gray(p(gvideo), 40, 20, 28, p(host), p(tab_dev), V, N_FAST, 2, CROP, 0.45, 0.225, p(gfast),
                                    p(slow), 0, 0, CROP, stream) == sfhip.SF_EINVAL
    torch.cuda.synchronize()
    assert bool((gfast == SENTINEL).all())


# video of each clip in two consecutive batches (B = 5, Nv = 4) and each video's label
_VIDS = ([2, 0, 2, 3, 2], [1, 1, 3, 0, 2])
_LABEL_OF = [5, 1, 6, 2]


def _host_meter(method, K, batches):
    from slowfast.utils.meters import TestMeter
    m = TestMeter(4, 3, K, 2, ensemble_method=method)
    for preds, labels, clip_ids in batches:
        m.update_stats(preds, labels, clip_ids)
    return m


def _batches(K, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n, vids in enumerate(_VIDS):
        preds = torch.randn(5, K, generator=g) * 3.0
        labels = torch.tensor([_LABEL_OF[v] % max(K, 1) for v in vids])
        clip_ids = torch.tensor([3 * v + (i + n) % 3 for i, v in enumerate(vids)])  # video = clip id // 3
        out.append((preds, labels, clip_ids))
    return out


@pytest.mark.parametrize("K", [7, 1])
@pytest.mark.parametrize("method", ["sum", "max"])
def test_ensemble_update_equals_host_meter(method, K):
    import sfhip
    from slowfast.utils.meters import DeviceTestMeter
    batches = _batches(K, 11 + K)
    host = _host_meter(method, K, batches)
    # the kernel on raw accumulators, between sentinel margins
    vp_all, vp = _guarded((4, K))
    vp.zero_()
    vl = torch.zeros(4, dtype=torch.int32, device="cuda")
    cc = torch.zeros(4, dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    dev_meter = DeviceTestMeter(4, 3, K, 2, ensemble_method=method)
    for preds, labels, clip_ids in batches:
        vid = (clip_ids // 3).to(torch.int32).cuda()
        sfhip.ensemble_update(preds.cuda(), vid, labels.to(torch.int32).cuda(), vp, vl, cc, bad,
                              0 if method == "sum" else 1)
        dev_meter.update_stats(preds.cuda(), labels.cuda(), clip_ids.cuda())
    torch.cuda.synchronize()
    assert _margins_intact(vp_all) and int(bad) == 0
    for got_p, got_l, got_c in ((vp, vl, cc), (dev_meter.video_preds, dev_meter.video_labels, dev_meter.clip_count)):
        assert _same_bits(got_p.cpu(), host.video_preds)  # sum: the host loop's order; max: exact by nature
        assert got_l.cpu().long().tolist() == host.video_labels.tolist()
        assert got_c.cpu().long().tolist() == host.clip_count.tolist() == [2, 2, 4, 2]
    ks = (1, 5) if K >= 5 else (1,)
    assert dev_meter.finalize_metrics(ks) == host.finalize_metrics(ks)
    dev_meter.reset()
    assert float(dev_meter.video_preds.abs().max()) == 0.0 and int(dev_meter.clip_count.sum()) == 0


def test_ensemble_update_skips_and_reports_an_index_out_of_range():
    import sfhip
    from slowfast.utils.meters import DeviceTestMeter
    K = 7
    preds = torch.randn(4, K, generator=torch.Generator().manual_seed(3))
    vid = torch.tensor([2, 4, -1, 0], dtype=torch.int32)  # Nv = 4: 4 and -1 are outside
    vp_all, vp = _guarded((4, K))
    vp.zero_()
    vl = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    cc = torch.zeros(4, dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    labels = torch.tensor([3, 9, 9, 1], dtype=torch.int32)
    for _ in range(2):
        sfhip.ensemble_update(preds.cuda(), vid.cuda(), labels.cuda(), vp, vl, cc, bad, 0)
    torch.cuda.synchronize()
    assert _margins_intact(vp_all) and int(bad) == 4  # two per call
    want = torch.zeros(4, K)
    want[2] = (want[2] + preds[0]) + preds[0]
    want[0] = (want[0] + preds[3]) + preds[3]
    assert _same_bits(vp.cpu(), want) and cc.tolist() == [2, 0, 2, 0] and vl.tolist() == [1, -7, 3, -7]
    m = DeviceTestMeter(4, 1, K, 1)
    m.update_stats(preds.cuda(), labels.cuda(), vid.cuda())  # one clip per video: clip id = video
    with pytest.raises(IndexError, match="2 clip"):
        m.finalize_metrics()
