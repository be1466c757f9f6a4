"""The streaming demo, model level: StreamingDemo over S + 2 frames against the reference's frame list restated — the
window's clip through gpu_input_step, the model on those clips, torch.nonzero on its output.  The same kernels run on
the same bits, so every comparison is exact."""
import contextlib
import io

import pytest
import torch

import _stream_ref as ref

pytestmark = pytest.mark.gpu

H = W = 48  # a square source, resampled to TEST_CROP_SIZE x TEST_CROP_SIZE


def _build(name):
    from _util import load_case, seeded_state_dict
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta = load_case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.DATA.TEST_CROP_SIZE = meta["t"], 2, meta["size"]
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    model.load_state_dict(seeded_state_dict(z["sd_keys"], z["sd_shapes"], meta["param_seed"]))
    return cfg, model.eval()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _restated_clips(cfg, model, frames, window):
    """The window's clip as the reference composes it (the S frames, BGR -> RGB, the fast linspace), through the
    per-clip input step: [slow, fast] ([clip] for a single pathway)."""
    from slowfast.datasets import utils as ds
    crop = cfg.DATA.TEST_CROP_SIZE
    single = cfg.MODEL.ARCH in cfg.MODEL.SINGLE_PATHWAY_ARCH
    fast_pos, _ = ref.window_positions(cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, None)
    clip = torch.stack([frames[window[int(i)]] for i in fast_pos]).flip(-1).contiguous().cuda()
    ph, pw, wp = ds.stem_input_geometry(model, crop)
    return ds.gpu_input_step([clip], [ds.SpatialParams(crop, crop, 0, 0, False, crop)], cfg.DATA.MEAN, cfg.DATA.STD,
                             None if single else cfg.SLOWFAST.ALPHA, pad=(ph, pw), wp=wp)


def _want_ids(preds):
    return [torch.nonzero(row > 0.1).reshape(-1).tolist() for row in preds.reshape(preds.shape[0], -1)]


@pytest.mark.parametrize("name", ["slowfast_r50_s64", "slow_r18_s64"])  # two pathways, one pathway
def test_streaming_classification(name):
    from slowfast.utils import stream
    cfg, model = _build(name)
    S = cfg.DATA.NUM_FRAMES * cfg.DATA.SAMPLING_RATE
    frames = ref.frames_u8(S + 2, H, W, seed=31)
    windows = dict(ref.reference_loop(len(frames), S, 1))
    assert sorted(windows) == [S - 1, S, S + 1]
    demo = stream.StreamingDemo(cfg, model)
    names = ["class%d" % i for i in range(cfg.MODEL.NUM_CLASSES)]
    for n, frame in enumerate(frames):
        got = demo.push(frame.numpy())
        if n not in windows:
            assert got is None
            continue
        want_in = _restated_clips(cfg, model, frames, windows[n])
        assert len(demo.last_inputs) == len(want_in)
        for a, b in zip(demo.last_inputs, want_in):
            assert a.shape == b.shape and (a.ph, a.pw, a.Wp) == (b.ph, b.pw, b.Wp)
            assert _same_bits(a.buf, b.buf), n
        with torch.no_grad():
            want = model(list(want_in))
        assert tuple(want.shape) == (1, cfg.MODEL.NUM_CLASSES)
        assert _same_bits(demo.last_preds, want), n  # tolerance 0
        ids = _want_ids(want)
        assert got.ids == ids and got.argmax == [int(torch.argmax(want[0]))]
        assert stream.labels_for(got.ids[0], names) == ([names[i] for i in ids[0]] or ["Unknown"])


def test_streaming_hop_empties_the_buffer():
    """hop = S (the reference's commented `frames = []`): windows fire on pushes S and 2 S only."""
    from slowfast.utils import stream
    cfg, model = _build("slow_r18_s64")
    S = cfg.DATA.NUM_FRAMES * cfg.DATA.SAMPLING_RATE
    frames = ref.frames_u8(2 * S, H, W, seed=37)
    windows = dict(ref.reference_loop(len(frames), S, S))
    demo = stream.StreamingDemo(cfg, model, hop=S)
    fired = []
    for n, frame in enumerate(frames):
        got = demo.push(frame)
        if got is not None:
            fired.append(n)
            want_in = _restated_clips(cfg, model, frames, windows[n])
            assert _same_bits(demo.last_inputs[0].buf, want_in[0].buf)
    assert fired == sorted(windows) == [S - 1, 2 * S - 1]


def test_streaming_detection_with_and_without_boxes():
    import sfhip
    from slowfast.utils import stream
    cfg, model = _build("slowfast_r50_ava_s64")
    assert cfg.DETECTION.ENABLE
    S = cfg.DATA.NUM_FRAMES * cfg.DATA.SAMPLING_RATE
    frames = ref.frames_u8(S + 1, H, W, seed=41)
    windows = dict(ref.reference_loop(len(frames), S, 1))
    demo = stream.StreamingDemo(cfg, model)
    for n in range(S - 1):
        assert demo.push(frames[n]) is None  # no boxes needed while the ring fills
    boxes = [[4.0, 6.0, 30.0, 40.0], [10.5, 2.0, 44.0, 47.0]]  # display coordinates of the 48 x 48 frame
    got = demo.push(frames[S - 1], boxes=boxes)
    want_in = _restated_clips(cfg, model, frames, windows[S - 1])
    for a, b in zip(demo.last_inputs, want_in):
        assert _same_bits(a.buf, b.buf)
    bboxes = ref.ref_scale_boxes(cfg.DATA.TEST_CROP_SIZE, boxes, H, W).cuda()
    with torch.no_grad():
        want = model(list(want_in), bboxes)
    assert tuple(want.shape) == (2, cfg.MODEL.NUM_CLASSES)
    assert _same_bits(demo.last_preds, want)
    assert got.ids == _want_ids(want) and len(got.ids) == 2
    assert got.argmax == [int(i) for i in torch.argmax(want, dim=1)]
    # nothing in the scene: an empty result, and only the frame's push reaches the library
    calls = sfhip.CALLS
    none = demo.push(frames[S], boxes=torch.zeros(0, 4))
    assert none == stream.DemoLabels([], []) and none is not None
    assert sfhip.CALLS == calls + 1 and demo.last_preds is None
    with pytest.raises(ValueError, match="person boxes"):
        demo.push(frames[S])  # a firing window needs to be told about the scene
