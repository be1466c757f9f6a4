"""Multi-view testing on the GPU, model level: test_view_params -> gpu_test_views -> model -> DeviceTestMeter against
the per-clip path (gpu_input_step on the gathered clips -> model -> TestMeter).  The inputs are bitwise equal
(tests/test_views_ops_gpu.py), so the model's outputs must be too: a difference means the batch layout is wrong."""
import contextlib
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_views_through_the_model_and_the_device_meter():
    from _util import load_case, seeded_state_dict
    from slowfast.config.defaults import get_cfg
    from slowfast.datasets import utils as ds
    from slowfast.models import build_model
    from slowfast.utils.meters import DeviceTestMeter, TestMeter
    z, meta = load_case("slowfast_r50_s64")
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    crop, t = meta["size"], meta["t"]
    cfg.DATA.NUM_FRAMES, cfg.DATA.SAMPLING_RATE, cfg.DATA.TEST_CROP_SIZE = t, 2, crop
    cfg.TEST.NUM_ENSEMBLE_VIEWS, cfg.TEST.NUM_SPATIAL_CROPS = 3, 3
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    model.load_state_dict(seeded_state_dict(z["sd_keys"], z["sd_shapes"], meta["param_seed"]))
    model.eval()
    ph, pw, wp = ds.stem_input_geometry(model, crop)
    alpha, n_views, n_videos = cfg.SLOWFAST.ALPHA, 9, 2
    num_cls = cfg.MODEL.NUM_CLASSES
    rs = np.random.RandomState(21)
    host = TestMeter(n_videos, n_views, num_cls, n_videos)
    dev = DeviceTestMeter(n_videos, n_views, num_cls, n_videos)
    labels = [3 % num_cls, 5 % num_cls]
    for vid, (h, w) in enumerate(((crop + 16, crop + 40), (crop + 30, crop + 8))):  # landscape, portrait
        video = torch.from_numpy(rs.randint(0, 256, (40, h, w, 3)).astype(np.uint8)).cuda()
        views = ds.test_view_params(cfg, 40, h, w)
        assert len(views) == n_views
        packed = ds.gpu_test_views(video, views, cfg.DATA.MEAN, cfg.DATA.STD, alpha, pad=(ph, pw), wp=wp)
        clips = [video.index_select(0, f.cuda()).contiguous() for f, _ in views]
        per_clip = ds.gpu_input_step(clips, [p for _, p in views], cfg.DATA.MEAN, cfg.DATA.STD, alpha, pad=(ph, pw),
                                     wp=wp)
        for a, b in zip(packed, per_clip):
            assert a.shape == b.shape and torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32))
        with torch.no_grad():
            out_views = model(list(packed))
            out_clips = model(list(per_clip))
        assert out_views.shape == (n_views, num_cls)
        assert torch.equal(out_views.view(torch.int32), out_clips.view(torch.int32))  # view for view
        lab = torch.full((n_views,), labels[vid], dtype=torch.long)
        clip_ids = torch.arange(n_views) + vid * n_views
        dev.update_stats(out_views, lab.cuda(), clip_ids.cuda())
        host.update_stats(out_clips.cpu(), lab, clip_ids)
    torch.cuda.synchronize()
    assert torch.equal(dev.video_preds.cpu().view(torch.int32), host.video_preds.view(torch.int32))
    assert dev.video_labels.cpu().long().tolist() == host.video_labels.tolist() == labels
    assert dev.clip_count.cpu().long().tolist() == host.clip_count.tolist() == [n_views] * n_videos
    ks = (1, min(5, num_cls))
    stats = dev.finalize_metrics(ks)
    assert stats == host.finalize_metrics(ks) and stats["complete"] is True
