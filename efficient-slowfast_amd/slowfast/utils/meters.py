"""Head-side test-time ensemble (reference utils/meters.py:214-373 TestMeter, utils/metrics.py:9-42).

The reference copies every batch of predictions to the host and adds them to per-video rows one clip at a time in a
Python loop.  Here the accumulators live on the model's device and one `index_add_` / `scatter_reduce_` per batch
performs the ensemble, so the test loop never synchronises with the GPU until `finalize_metrics`."""
from slowfast._overlay import chain_module as _chain_module

_chain_module(globals())  # the reference's namesake (when importable) supplies every name not defined below
import datetime
import json
import logging
import time

import torch

_LOG = logging.getLogger(__name__)


def topks_correct(preds, labels, ks):
    """Number of samples whose label is within the top-k predictions, for each k (utils/metrics.py:9-42)."""
    assert preds.size(0) == labels.size(0), "Batch dim of predictions and labels must match"
    _, inds = torch.topk(preds, max(ks), dim=1, largest=True, sorted=True)
    correct = inds.t().eq(labels.view(1, -1).expand(max(ks), -1))
    return [correct[:k, :].reshape(-1).float().sum() for k in ks]


class TestMeter(object):
    """Sum / max ensemble of `num_clips` clip predictions per video and the final top-k accuracies."""

    __test__ = False  # not a pytest class

    def __init__(self, num_videos, num_clips, num_cls, overall_iters, multi_label=False, ensemble_method="sum",
                 device="cpu"):
        if ensemble_method not in ("sum", "max"):
            raise NotImplementedError("Ensemble Method {} is not supported".format(ensemble_method))
        self.num_clips = num_clips
        self.overall_iters = overall_iters
        self._tic, self._lap = time.perf_counter(), 0.0
        self.multi_label = multi_label
        self.ensemble_method = ensemble_method
        self.video_preds = torch.zeros((num_videos, num_cls), device=device)
        self.video_labels = (torch.zeros((num_videos, num_cls), device=device) if multi_label
                             else torch.zeros((num_videos,), dtype=torch.long, device=device))
        self.clip_count = torch.zeros((num_videos,), dtype=torch.long, device=device)
        self.reset()

    def reset(self):
        self.clip_count.zero_()
        self.video_preds.zero_()
        if self.multi_label:
            self.video_preds -= 1e10
        self.video_labels.zero_()

    def update_stats(self, preds, labels, clip_ids):
        """preds [N, C], labels [N] (or [N, C] multi-label), clip_ids [N]: video = clip_id // num_clips."""
        dev = self.video_preds.device
        preds, labels = preds.detach().to(dev), labels.to(dev)
        vid = torch.div(clip_ids.to(dev).long(), self.num_clips, rounding_mode="floor")
        self.video_labels[vid] = labels.to(self.video_labels.dtype)
        if self.ensemble_method == "sum":
            self.video_preds.index_add_(0, vid, preds.to(self.video_preds.dtype))
        else:
            self.video_preds.scatter_reduce_(0, vid.view(-1, 1).expand_as(preds), preds.to(self.video_preds.dtype),
                                             reduce="amax", include_self=True)
        self.clip_count.index_add_(0, vid, torch.ones_like(vid))

    def iter_tic(self):
        """Start timing one test iteration (utils/meters.py:337-338)."""
        self._tic = time.perf_counter()

    def iter_toc(self):
        """Stop timing; the lap feeds `log_iter_stats` (utils/meters.py:340-341)."""
        self._lap = time.perf_counter() - self._tic

    def log_iter_stats(self, cur_iter):
        """One `json_stats:` line per iteration with the remaining-time estimate (utils/meters.py:319-335)."""
        eta = str(datetime.timedelta(seconds=int(self._lap * (self.overall_iters - cur_iter))))
        stats = {"split": "test_iter", "cur_iter": "{}".format(cur_iter + 1), "eta": eta, "time_diff": self._lap}
        _LOG.info("json_stats: {}".format(json.dumps(stats, sort_keys=True)))
        return stats

    def finalize_metrics(self, ks=(1, 5)):
        """Returns {"split": "test_final", "top{k}_acc": "xx.xx", ...} (multi-label mAP is not on this path)."""
        if self.multi_label:
            raise NotImplementedError("multi-label mAP (AVA/Charades) is outside the hot-path scope")
        stats = {"split": "test_final", "complete": bool((self.clip_count == self.num_clips).all())}
        correct = topks_correct(self.video_preds, self.video_labels, ks)
        for k, c in zip(ks, correct):
            stats["top{}_acc".format(k)] = "{:.{prec}f}".format(float(c) / self.video_preds.size(0) * 100.0, prec=2)
        return stats


class DeviceTestMeter(TestMeter):
    """TestMeter whose ensemble is one `sf_ensemble_update` launch per batch: predictions, labels and clip ids stay on
    the GPU, the per-video rows are folded in the host loop's order (the sum is TestMeter's bit for bit) and nothing
    is copied to the host before `finalize_metrics`."""

    def __init__(self, num_videos, num_clips, num_cls, overall_iters, multi_label=False, ensemble_method="sum",
                 device="cuda"):
        if ensemble_method not in ("sum", "max"):
            raise NotImplementedError("Ensemble Method {} is not supported".format(ensemble_method))
        self.num_clips = num_clips
        self.overall_iters = overall_iters
        self._tic, self._lap = time.perf_counter(), 0.0
        self.multi_label = multi_label
        self.ensemble_method = ensemble_method
        self.device = torch.device(device)
        self._shape = (num_videos, num_cls)
        self.video_preds = self.video_labels = self.clip_count = self.bad_count = None  # allocated on first use

    def _allocate(self):
        n, k = self._shape
        self.video_preds = torch.zeros((n, k), device=self.device)
        self.video_labels = torch.zeros((n,), dtype=torch.int32, device=self.device)
        self.clip_count = torch.zeros((n,), dtype=torch.int32, device=self.device)
        self.bad_count = torch.zeros((1,), dtype=torch.int32, device=self.device)

    def reset(self):
        if self.video_preds is not None:
            for t in (self.video_preds, self.video_labels, self.clip_count, self.bad_count):
                t.zero_()

    def update_stats(self, preds, labels, clip_ids):
        """preds [N, C], labels [N], clip_ids [N], all on the device: video = clip_id // num_clips."""
        if self.multi_label:
            raise NotImplementedError("multi-label mAP (AVA/Charades) is outside the hot-path scope")
        import sfhip
        if self.video_preds is None:
            self._allocate()
        vid = torch.div(clip_ids, self.num_clips, rounding_mode="floor").to(torch.int32).contiguous()
        sfhip.ensemble_update(preds.detach().float().contiguous(), vid, labels.to(torch.int32).contiguous(),
                              self.video_preds, self.video_labels, self.clip_count, self.bad_count,
                              0 if self.ensemble_method == "sum" else 1)

    def finalize_metrics(self, ks=(1, 5)):
        """One copy of the accumulators to the host, then TestMeter's statistics (through `topks_correct`)."""
        if self.multi_label:
            raise NotImplementedError("multi-label mAP (AVA/Charades) is outside the hot-path scope")
        if self.video_preds is None:
            self._allocate()
        n, k = self._shape
        packed = torch.cat([self.video_preds.flatten().view(torch.int32), self.video_labels, self.clip_count,
                            self.bad_count]).cpu()  # the one device-to-host copy
        video_preds = packed[:n * k].view(torch.float32).view(n, k)
        video_labels, clip_count = packed[n * k:n * k + n].long(), packed[n * k + n:n * k + 2 * n].long()
        bad = int(packed[-1])
        if bad:
            raise IndexError("{} clip(s) named a video outside [0, {}) and were skipped".format(bad, n))
        stats = {"split": "test_final", "complete": bool((clip_count == self.num_clips).all())}
        correct = topks_correct(video_preds, video_labels, ks)
        for kk, c in zip(ks, correct):
            stats["top{}_acc".format(kk)] = "{:.{prec}f}".format(float(c) / video_preds.size(0) * 100.0, prec=2)
        return stats
