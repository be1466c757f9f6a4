"""Head-side test-time ensemble (reference utils/meters.py:214-373 TestMeter, utils/metrics.py:9-42).

The reference copies every batch of predictions to the host and adds them to per-video rows one clip at a time in a
Python loop.  Here the accumulators live on the model's device and one `index_add_` / `scatter_reduce_` per batch
performs the ensemble, so the test loop never synchronises with the GPU until `finalize_metrics`.

The multi-label side (reference :623-632, :671-675, :690-714) is here too: `get_map` (numpy, no scikit-learn) for host
tensors, `device_map` / `DeviceMultiLabelTestMeter` / `DeviceValMeter` on the `sf_map`, `sf_ensemble_update_ml`,
`sf_topk_errors` and `sf_rows_append` kernels.

Class by class (no counterpart in the reference): `DevicePerClassMeter` keeps a confusion matrix and per-class top-k
hits on the device (`sf_confusion_update`) and reads precision / recall / F1 per class once per epoch
(`sf_class_report`); `DeviceValMeter` and `DeviceTestMeter` take one as `per_class=`.

Detection (reference :28-213 get_ava_mini_groundtruth, AVAMeter): `DeviceAVAMeter` keeps predictions, boxes and metadata
on the device and computes the AVA frame-mAP with `sf_ava_match` / `sf_ava_ap` (utils/ava_eval_helper.py)."""
from slowfast._overlay import chain_module as _chain_module

_chain_module(globals())  # the reference's namesake (when importable) supplies every name not defined below
import collections
import datetime
import json
import logging
import math
import time

import numpy as np
import torch

_LOG = logging.getLogger(__name__)


def topks_correct(preds, labels, ks):
    """Number of samples whose label is within the top-k predictions, for each k (utils/metrics.py:9-42)."""
    assert preds.size(0) == labels.size(0), "Batch dim of predictions and labels must match"
    _, inds = torch.topk(preds, max(ks), dim=1, largest=True, sorted=True)
    correct = inds.t().eq(labels.view(1, -1).expand(max(ks), -1))
    return [correct[:k, :].reshape(-1).float().sum() for k in ks]


def _check_map_inputs(preds, labels):
    preds, labels = np.asarray(preds), np.asarray(labels)
    if preds.ndim != 2 or preds.shape != labels.shape:
        raise ValueError("get_map: preds [N, C] and labels [N, C], got {} and {}".format(preds.shape, labels.shape))
    bad = int((~np.isfinite(preds)).sum() + ((labels != 0) & (labels != 1)).sum())
    if bad:
        raise ValueError("get_map: {} element(s) with a NaN or infinite score or a label other than 0 or 1".format(bad))
    return preds, labels == 1


def average_precisions(preds, labels):
    """Per-class average precision, float64 [C], -1 for a class without a positive: what
    sklearn.metrics.average_precision_score(labels, preds, average=None) returns for the other classes, as

        AP = (1/P) sum_{i : y_i = 1} TP(s_i) / CNT(s_i),  TP(t) = #{j : s_j >= t, y_j = 1},  CNT(t) = #{j : s_j >= t}

    (scikit-learn walks the distinct thresholds of the sorted scores; tied scores form one threshold and every positive
    of the tie group contributes the group's precision — the same sum).  Scores compare as floats: -0.0 ties +0.0."""
    preds, pos = _check_map_inputs(preds, labels)
    n, c = preds.shape
    aps = np.full((c,), -1.0, dtype=np.float64)
    for k in range(c):
        s, y = preds[:, k], pos[:, k]
        p = int(y.sum())
        if p == 0:
            continue
        sp = s[y]
        cnt = n - np.searchsorted(np.sort(s), sp, side="left")
        tp = p - np.searchsorted(np.sort(sp), sp, side="left")
        aps[k] = float(np.sum(tp.astype(np.float64) / cnt.astype(np.float64))) / p
    return aps


def get_map(preds, labels):
    """utils/meters.py:690-714 for host arrays [N, C] without scikit-learn: the mean of `average_precisions` over the
    classes with a positive, 0.0 when there is none (the reference prints scikit-learn's error and returns 0.0).  A NaN
    or infinite score or a label other than 0 or 1 raises ValueError (the reference swallows scikit-learn's error and
    reports 0.0 there)."""
    _LOG.info("Getting mAP for {} examples".format(np.asarray(preds).shape[0]))
    aps = average_precisions(preds, labels)
    aps = aps[aps >= 0]
    return float(np.mean(aps)) if aps.size else 0.0


def _checked_map(out3, who):
    """(mAP, classes, refused) as read from `sf_map`'s out -> the mAP, or ValueError for refused elements."""
    if out3[2] != 0:
        raise ValueError("{}: {} element(s) with a NaN or infinite score or a label other than 0 or 1".format(
            who, int(out3[2])))
    return float(out3[0])


def device_map(preds, labels):
    """`get_map` of GPU tensors [N, C]: one `sf_map` call and ONE device-to-host copy (its three-number result)."""
    import sfhip
    out = sfhip.mean_ap(preds.detach().float(), labels if labels.dtype == torch.float32 else labels.float())
    return _checked_map(out.cpu().tolist(), "device_map")


# ---------------------------------------------------------------------------------------------- per-class meter
PER_CLASS_COLUMNS = ("support", "precision", "recall", "f1", "top1_acc", "topk_acc")
SUMMARY_FIELDS = ("samples", "accuracy", "mean_class_accuracy", "macro_precision", "macro_recall", "macro_f1",
                  "classes_with_support", "classes_never_predicted")
_PER_CLASS_ML_REFUSAL = ("per-class reports are single-label (confusion matrix, precision / recall per class) — for "
                         "multi-label evaluation sf_map already returns the per-class AP")
_REPORT_KMAX = 1024  # sf_class_report: one workgroup


def format_json_stats(stats):
    """The line utils/logging.py:84-96 log_json_stats writes: floats with six decimals, keys sorted."""
    items = []
    for k in sorted(stats):
        v = stats[k]
        items.append("%s: %s" % (json.dumps(k), "{:.6f}".format(v) if isinstance(v, float) else json.dumps(v)))
    return "json_stats: {" + ", ".join(items) + "}"


class DevicePerClassMeter(object):
    """Which class is taken for which, and every class's precision / recall / F1, without a prediction on the host.
    The state is ONE int64 buffer on `device`: `conf` [K, K] ([true, predicted]), `hits` [K, 2] (label within the top 1 /
    top `k_hi`, per true class) and `refused` [2] (rows with a label outside [0, K); rows holding a NaN or an infinity),
    followed by the fp64 report `sf_class_report` writes.  `update(preds, labels)` is one `sf_confusion_update` launch —
    no sync, capturable; `all_reduce()` is one collective on the int64 part; `finalize()` is one `sf_class_report`
    launch and the ONE host read of the epoch.  The tie rule is `sf_topk_errors`' (include/sfhip.h): of equal scores
    the lower class index is predicted."""

    def __init__(self, num_classes, k_hi, device="cuda"):
        K, k_hi = int(num_classes), int(k_hi)
        if K < 1 or K > _REPORT_KMAX:
            raise ValueError("DevicePerClassMeter: num_classes must be in [1, {}], got {}".format(_REPORT_KMAX, K))
        if k_hi < 1 or k_hi > K:
            raise ValueError("DevicePerClassMeter: k_hi must be in [1, num_classes = {}], got {}".format(K, k_hi))
        self.num_classes, self.k_hi = K, k_hi
        self.device = torch.device(device)
        n_int = K * K + 2 * K + 2
        self._buf = torch.zeros((n_int + len(SUMMARY_FIELDS) + len(PER_CLASS_COLUMNS) * K,), dtype=torch.int64,
                                device=self.device)
        self.state = self._buf[:n_int]  # what all_reduce sums
        self.conf = self.state[:K * K].view(K, K)
        self.hits = self.state[K * K:K * K + 2 * K].view(K, 2)
        self.refused = self.state[K * K + 2 * K:]
        report = self._buf[n_int:].view(torch.float64)
        self.summary = report[:len(SUMMARY_FIELDS)]
        self.per_class = report[len(SUMMARY_FIELDS):].view(K, len(PER_CLASS_COLUMNS))

    def reset(self):
        self._buf.zero_()

    def update(self, preds, labels):
        """preds [N, K] and labels [N] on the device: one launch, nothing read."""
        import sfhip
        if preds.dim() != 2 or preds.shape[1] != self.num_classes:
            raise ValueError("DevicePerClassMeter: preds [N, {}], got {}".format(self.num_classes, tuple(preds.shape)))
        preds = preds.detach()
        sfhip.confusion_update(preds if preds.dtype == torch.float32 else preds.float(),
                               labels if labels.dtype == torch.int64 else labels.long(), self.k_hi, self.conf,
                               self.hits, self.refused)

    def all_reduce(self):
        """Sum the counters over the ranks: one collective on the flat int64 state; nothing at world size 1."""
        import slowfast.utils.distributed as du
        du.all_reduce([self.state], average=False)

    def class_weights(self, scheme="balanced", beta=None, out=None):
        """fp32 [K] class weights from the counters added since reset(), for `HipCrossEntropy(weight=)` / `HipBCE(weight=)`:
        one `sf_class_weights` launch, nothing read — capturable; `out` (fp32 [K] on the meter's device) is written in
        place, so a loss that holds it sees the new weights.  "balanced": scikit-learn's compute_class_weight("balanced")
        over the classes with support, samples / (classes with support * support[c]); "effective": the class-balanced
        (1 - beta) / (1 - beta^support[c]), rescaled to sum to the number of classes with support, `beta` in (0, 1).  A
        class without support gets 0.  Across ranks call it AFTER `all_reduce()` has summed the counters: there is no
        collective in here, and weights made from one rank's counters differ from rank to rank."""
        import sfhip
        return sfhip.class_weights(self.conf, scheme=scheme, beta=beta, out=out)

    def finalize(self, allow_refused=False):
        """The report of everything added since reset(): one launch, then the one host read.  Returns {"confusion": int64
        [K, K], "hits": int64 [K, 2], "per_class": fp64 [K, 6] (PER_CLASS_COLUMNS), "summary": {SUMMARY_FIELDS},
        "refused": {"bad_label", "non_finite"}, "k_hi"} on the host.  Refused rows raise ValueError unless
        `allow_refused`."""
        import sfhip
        K = self.num_classes
        sfhip.class_report(self.conf, self.hits, self.summary, self.per_class)
        host = self._buf.cpu()  # the one device-to-host copy
        n_int = K * K + 2 * K + 2
        bad_label, non_finite = int(host[n_int - 2]), int(host[n_int - 1])
        if (bad_label or non_finite) and not allow_refused:
            raise ValueError("DevicePerClassMeter: {} row(s) with a label outside [0, {}) and {} row(s) with a NaN or "
                             "infinite prediction were left out".format(bad_label, K, non_finite))
        report = host[n_int:].view(torch.float64)
        summary = dict(zip(SUMMARY_FIELDS, report[:len(SUMMARY_FIELDS)].tolist()))
        for name in ("samples", "classes_with_support", "classes_never_predicted"):
            summary[name] = int(summary[name])
        return {"confusion": host[:K * K].view(K, K).clone(), "hits": host[K * K:K * K + 2 * K].view(K, 2).clone(),
                "per_class": report[len(SUMMARY_FIELDS):].view(K, len(PER_CLASS_COLUMNS)).clone(),
                "summary": summary, "refused": {"bad_label": bad_label, "non_finite": non_finite}, "k_hi": self.k_hi}

    def log_report(self, class_names=None, report=None, allow_refused=False):
        """One `json_stats:` line for the summary and one per class (`class_names[c]`, or the index).  Formats `report`
        (a finalize() result) when given, so that logging costs no second host read; returns the logged records."""
        K = self.num_classes
        if class_names is not None and len(class_names) != K:
            raise ValueError("DevicePerClassMeter: {} class names for {} classes".format(len(class_names), K))
        if report is None:
            report = self.finalize(allow_refused=allow_refused)
        records = [dict({"_type": "class_report", "k_hi": report["k_hi"],
                         "refused_bad_label": report["refused"]["bad_label"],
                         "refused_non_finite": report["refused"]["non_finite"]}, **report["summary"])]
        table, conf = report["per_class"].tolist(), report["confusion"].tolist()
        for c in range(K):
            rec = {"_type": "class_report_class", "class": str(class_names[c]) if class_names is not None else c,
                   "confused_as": conf[c]}
            for name, v in zip(PER_CLASS_COLUMNS, table[c]):
                rec[name] = int(v) if name == "support" else v
            records.append(rec)
        for rec in records:
            _LOG.info(format_json_stats(rec))
        return records


def _checked_per_class(per_class, multi_label, who):
    if per_class is None:
        return None
    if not isinstance(per_class, DevicePerClassMeter):
        raise TypeError("{}: per_class must be a DevicePerClassMeter, got {}".format(who, type(per_class).__name__))
    if multi_label:
        raise ValueError("{}: {}".format(who, _PER_CLASS_ML_REFUSAL))
    return per_class


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
        """Returns {"split": "test_final", "top{k}_acc": "xx.xx", ...}, or {..., "map": mAP} under multi_label
        (utils/meters.py:353-358, through `get_map`)."""
        stats = {"split": "test_final", "complete": bool((self.clip_count == self.num_clips).all())}
        if self.multi_label:
            stats["map"] = get_map(self.video_preds.cpu().numpy(), self.video_labels.cpu().numpy())
            return stats
        correct = topks_correct(self.video_preds, self.video_labels, ks)
        for k, c in zip(ks, correct):
            stats["top{}_acc".format(k)] = "{:.{prec}f}".format(float(c) / self.video_preds.size(0) * 100.0, prec=2)
        return stats


_ML_REFUSAL = ("multi-label mAP (AVA/Charades) is outside the hot-path scope of DeviceTestMeter — use "
               "DeviceMultiLabelTestMeter")


class DeviceTestMeter(TestMeter):
    """TestMeter whose ensemble is one `sf_ensemble_update` launch per batch: predictions, labels and clip ids stay on
    the GPU, the per-video rows are folded in the host loop's order (the sum is TestMeter's bit for bit) and nothing
    is copied to the host before `finalize_metrics`."""

    def __init__(self, num_videos, num_clips, num_cls, overall_iters, multi_label=False, ensemble_method="sum",
                 device="cuda", per_class=None):
        if ensemble_method not in ("sum", "max"):
            raise NotImplementedError("Ensemble Method {} is not supported".format(ensemble_method))
        self.per_class = _checked_per_class(per_class, multi_label, "DeviceTestMeter")
        if self.per_class is not None and self.per_class.num_classes != num_cls:
            raise ValueError("DeviceTestMeter: per_class counts {} classes, the meter {}".format(
                self.per_class.num_classes, num_cls))
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
            raise NotImplementedError(_ML_REFUSAL)
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
            raise NotImplementedError(_ML_REFUSAL)
        if self.video_preds is None:
            self._allocate()
        n, k = self._shape
        if self.per_class is not None:  # the ensemble's rows, once: the report is the videos', whatever it held
            self.per_class.reset()
            self.per_class.update(self.video_preds, self.video_labels.long())
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


class DeviceMultiLabelTestMeter(TestMeter):
    """The multi-label TestMeter (rows reset to -1e10, label rows, mAP) on the device: one `sf_ensemble_update_ml` launch
    per batch, `sf_map` and ONE copy to the host in `finalize_metrics`.  A clip whose label row differs from the row its
    video already holds (the reference's `assert torch.equal`, :292-296) is counted on the device and raises ValueError
    at the end; a clip of a video outside [0, num_videos) raises IndexError."""

    def __init__(self, num_videos, num_clips, num_cls, overall_iters, multi_label=True, ensemble_method="sum",
                 device="cuda", per_class=None):
        if ensemble_method not in ("sum", "max"):
            raise NotImplementedError("Ensemble Method {} is not supported".format(ensemble_method))
        _checked_per_class(per_class, True, "DeviceMultiLabelTestMeter")
        if not multi_label:
            raise ValueError("DeviceMultiLabelTestMeter is the multi-label meter — use DeviceTestMeter")
        self.num_clips = num_clips
        self.overall_iters = overall_iters
        self._tic, self._lap = time.perf_counter(), 0.0
        self.multi_label = True
        self.ensemble_method = ensemble_method
        self.device = torch.device(device)
        self._shape = (num_videos, num_cls)
        self.video_preds = self.video_labels = self.clip_count = self.bad_count = None  # allocated on first use

    def _allocate(self):
        n, k = self._shape
        self.video_preds = torch.full((n, k), -1e10, dtype=torch.float32, device=self.device)
        self.video_labels = torch.zeros((n, k), dtype=torch.float32, device=self.device)
        self.clip_count = torch.zeros((n,), dtype=torch.int32, device=self.device)
        self.bad_count = torch.zeros((2,), dtype=torch.int32, device=self.device)

    def reset(self):
        if self.video_preds is not None:
            self.video_preds.fill_(-1e10)
            for t in (self.video_labels, self.clip_count, self.bad_count):
                t.zero_()

    def update_stats(self, preds, labels, clip_ids):
        """preds [N, C], labels [N, C] (any real dtype), clip_ids [N], all on the device."""
        import sfhip
        if self.video_preds is None:
            self._allocate()
        vid = torch.div(clip_ids, self.num_clips, rounding_mode="floor").to(torch.int32).contiguous()
        labels = labels if labels.dtype == torch.float32 else labels.float()
        sfhip.ensemble_update_ml(preds.detach().float().contiguous(), vid, labels, self.video_preds, self.video_labels,
                                 self.clip_count, self.bad_count, 0 if self.ensemble_method == "sum" else 1)

    def finalize_metrics(self, ks=(1, 5)):
        """`sf_map` over the rows, then one copy: {"split": "test_final", "complete": ..., "map": ...}."""
        import sfhip
        if self.video_preds is None:
            self._allocate()
        n, _ = self._shape
        out = sfhip.mean_ap(self.video_preds, self.video_labels)
        packed = torch.cat([out, self.clip_count.double(), self.bad_count.double()]).cpu()  # the one copy
        clip_count = packed[3:3 + n]
        bad, mismatched = int(packed[3 + n]), int(packed[4 + n])
        if bad:
            raise IndexError("{} clip(s) named a video outside [0, {}) and were skipped".format(bad, n))
        if mismatched:
            raise ValueError("{} clip(s) carried a label row that differs from the one their video already "
                             "held".format(mismatched))
        return {"split": "test_final", "complete": bool((clip_count == self.num_clips).all()),
                "map": _checked_map(packed[:3].tolist(), "DeviceMultiLabelTestMeter")}


# ---------------------------------------------------------------------------------------------- training meter
class _ScalarWindow(object):
    """utils/meters.py:375-423 ScalarMeter: a window of the last `window_size` values plus the running total."""

    def __init__(self, window_size):
        self.deque = collections.deque(maxlen=window_size)
        self.total = 0.0
        self.count = 0

    def reset(self):
        self.deque.clear()
        self.total = 0.0
        self.count = 0

    def add_value(self, value):
        self.deque.append(value)
        self.count += 1
        self.total += value

    def get_win_median(self):
        return np.median(self.deque)

    def get_win_avg(self):
        return np.mean(self.deque)

    def get_global_avg(self):
        return self.total / self.count


def _drain_ring(ring, drained, world, who, cols=7):
    """The rows written to `ring` since step `drained`, oldest first, as lists of seven floats {loss, top-1 err, top-k
    err, non-finite flag, N, bad count, kind} (cols=8: and the gradient norm `HipGradClip` left in column 7): one
    all-reduce (mean) of the block when world > 1 (train_net.py:128-131, :233-234), ONE device-to-host copy."""
    import slowfast.utils.distributed as du
    # the counter rides in the block (exact in float32 far beyond any epoch: the difference below is what is used)
    block = torch.cat([ring.rows.flatten(), ring.counter.to(torch.float64).sub_(drained).float()])
    if world > 1:
        du.all_reduce([block])
    host = block.cpu()  # the one device-to-host copy (the only synchronisation of the logging period)
    fresh = int(round(float(host[-1])))
    rows = host[:-1].view(ring.cap, -1)
    if fresh < 0 or fresh > ring.cap:
        raise RuntimeError("{}: {} steps since the last drain but the ring holds {} — drain at least "
                           "every LOG_PERIOD steps".format(who, fresh, ring.cap))
    return [[float(v) for v in rows[i % ring.cap, :cols]] for i in range(drained, drained + fresh)]


class DeviceTrainMeter(object):
    """TrainMeter (utils/meters.py:426-554) for a loop that never reads the loss on the host: the loss kernel
    (`models.step_tail.HipCrossEntropy`) leaves one row {loss, top-1 err, top-k err, non-finite flag, N, bad labels}
    per step in a device ring of LOG_PERIOD rows, `update_stats(lr)` only records the host learning rate, and
    `log_iter_stats` (on a LOG_PERIOD boundary) / `log_epoch_stats` drain the ring: one all-reduce of the block when
    NUM_GPUS > 1 (train_net.py:128-131), ONE device-to-host copy, then TrainMeter.update_stats' arithmetic row by row —
    the logged medians and averages are the reference's for the same values.  A drained row with the non-finite flag
    raises misc.check_nan_losses' RuntimeWarning (late by at most LOG_PERIOD steps; `HipSGD.step(guard=...)` keeps
    such a step from touching the parameters), a bad-label count raises ValueError.  The BCE losses (`HipBCE`,
    `HipBCEWithLogits`) write the same rows with field 6 = 1 and no top-k errors; with `cfg.DATA.MULTI_LABEL` the meter
    folds the loss and the sample count only and logs what the reference's TrainMeter logs then (utils/meters.py:492,
    523, 547): no top1_err / top5_err per iteration, and neither those nor the loss per epoch.
    `grad_norm=True` (opt-in; the default changes nothing): the drain also folds column 7 of every row — the step's
    total gradient norm, left there by `models.step_tail.HipGradClip(..., ring=meter.ring)` — into a window, and
    `log_iter_stats` adds its median as "grad_norm"; a row whose norm is not finite raises the same RuntimeWarning."""

    def __init__(self, epoch_iters, cfg, ring=None, device="cuda", grad_norm=False):
        from slowfast.models.step_tail import StatsRing
        self._cfg = cfg
        self._multi_label = bool(cfg.DATA.MULTI_LABEL)
        self._grad_norm = bool(grad_norm)
        self.grad_norm = _ScalarWindow(cfg.LOG_PERIOD)
        self.epoch_iters = epoch_iters
        self.MAX_EPOCH = cfg.SOLVER.MAX_EPOCH * epoch_iters
        self._tic, self._lap = time.perf_counter(), 0.0
        self.ring = ring if ring is not None else StatsRing(cfg.LOG_PERIOD, device)
        self._drained = 0  # ring.counter at the last drain
        self.loss = _ScalarWindow(cfg.LOG_PERIOD)
        self.mb_top1_err = _ScalarWindow(cfg.LOG_PERIOD)
        self.mb_top5_err = _ScalarWindow(cfg.LOG_PERIOD)
        self.reset()

    def reset(self):
        self.loss.reset()
        self.loss_total = 0.0
        self.lr = None
        self.mb_top1_err.reset()
        self.mb_top5_err.reset()
        self.grad_norm.reset()
        self.num_top1_mis = 0
        self.num_top5_mis = 0
        self.num_samples = 0

    def iter_tic(self):
        self._tic = time.perf_counter()

    def iter_toc(self):
        self._lap = time.perf_counter() - self._tic

    def update_stats(self, lr):
        self.lr = lr

    def _fold(self, top1_err, top5_err, loss, mb_size):
        """TrainMeter.update_stats (utils/meters.py:477-498) for one step's values."""
        self.loss.add_value(loss)
        self.loss_total += loss * mb_size
        self.num_samples += mb_size
        if self._multi_label:
            return
        self.mb_top1_err.add_value(top1_err)
        self.mb_top5_err.add_value(top5_err)
        self.num_top1_mis += top1_err * mb_size
        self.num_top5_mis += top5_err * mb_size

    def drain(self):
        """Fold the rows written since the last drain; returns how many there were."""
        world = max(int(self._cfg.NUM_GPUS), 1)
        rows = _drain_ring(self.ring, self._drained, world, "DeviceTrainMeter", cols=8 if self._grad_norm else 7)
        for i, (loss, top1, top5, flag, n, bad, kind, *norm) in enumerate(rows, self._drained):
            if bad != 0:
                what = "label(s) outside [0, classes)" if kind == 0 else "target or probability outside [0, 1]"
                raise ValueError("DeviceTrainMeter: step {} had {} ({:g} per rank on average)".format(i, what, bad))
            if flag != 0 or math.isnan(loss) or (norm and not math.isfinite(norm[0])):
                raise RuntimeWarning("ERROR: Got NaN losses {}".format(datetime.datetime.now()))
            self._fold(top1, top5, loss, int(round(n)) * world)
            if norm:
                self.grad_norm.add_value(norm[0])
        self._drained += len(rows)
        return len(rows)

    def _eta(self, iters_left):
        return str(datetime.timedelta(seconds=int(self._lap * iters_left)))

    @staticmethod
    def _gpu_mem():
        return (torch.cuda.max_memory_allocated() if torch.cuda.is_available() else 0) / 1024 ** 2

    def log_iter_stats(self, cur_epoch, cur_iter):
        if (cur_iter + 1) % self._cfg.LOG_PERIOD != 0:
            return None
        self.drain()
        stats = {
            "_type": "train_iter",
            "epoch": "{}/{}".format(cur_epoch + 1, self._cfg.SOLVER.MAX_EPOCH),
            "iter": "{}/{}".format(cur_iter + 1, self.epoch_iters),
            "time_diff": self._lap,
            "eta": self._eta(self.MAX_EPOCH - (cur_epoch * self.epoch_iters + cur_iter + 1)),
            "loss": self.loss.get_win_median(),
            "lr": self.lr,
            "gpu_mem": "{:.2f} GB".format(self._gpu_mem()),
        }
        if not self._multi_label:
            stats["top1_err"] = self.mb_top1_err.get_win_median()
            stats["top5_err"] = self.mb_top5_err.get_win_median()
        if self._grad_norm:
            stats["grad_norm"] = self.grad_norm.get_win_median()
        _LOG.info(format_json_stats(stats))
        return stats

    def log_epoch_stats(self, cur_epoch):
        self.drain()
        stats = {
            "_type": "train_epoch",
            "epoch": "{}/{}".format(cur_epoch + 1, self._cfg.SOLVER.MAX_EPOCH),
            "time_diff": self._lap,
            "eta": self._eta(self.MAX_EPOCH - (cur_epoch + 1) * self.epoch_iters),
            "lr": self.lr,
            "gpu_mem": "{:.2f} GB".format(self._gpu_mem()),
        }
        _ram_field(stats)
        if not self._multi_label:
            stats["top1_err"] = self.num_top1_mis / self.num_samples
            stats["top5_err"] = self.num_top5_mis / self.num_samples
            stats["loss"] = self.loss_total / self.num_samples
        _LOG.info(format_json_stats(stats))
        return stats


# ---------------------------------------------------------------------------------------------- validation meter
def _ram_field(stats):
    try:
        import psutil
        vram = psutil.virtual_memory()
        stats["RAM"] = "{:.2f}/{:.2f} GB".format((vram.total - vram.available) / 1024 ** 3, vram.total / 1024 ** 3)
    except ImportError:  # the reference needs psutil for this one field
        pass


class DeviceValMeter(object):
    """ValMeter (utils/meters.py:557-687) for an eval_epoch (train_net.py:166-251) that never reads a prediction on the
    host.  Single-label: `update_stats(preds, labels)` is one `sf_topk_errors` launch that leaves the batch's top-1 /
    top-k errors as a ring row; `log_iter_stats` (on a LOG_PERIOD boundary) and `log_epoch_stats` drain the ring as
    DeviceTrainMeter does — one all-reduce when NUM_GPUS > 1, ONE copy — and fold the rows with ValMeter.update_stats'
    arithmetic.  With `cfg.DATA.MULTI_LABEL`: `update_predictions(preds, labels)` is one `sf_rows_append` launch into a
    device store of `max_iter` batches (sized on first use), and `log_epoch_stats` gathers every rank's filled rows
    once, runs `sf_map` and makes ONE copy.  The logged records are the reference's."""

    def __init__(self, max_iter, cfg, ring=None, device="cuda", per_class=None):
        from slowfast.models.step_tail import StatsRing
        self._cfg = cfg
        self._multi_label = bool(cfg.DATA.MULTI_LABEL)
        self.per_class = _checked_per_class(per_class, self._multi_label, "DeviceValMeter")
        self.max_iter = max_iter
        self.device = torch.device(device)
        self._tic, self._lap = time.perf_counter(), 0.0
        self.ring = ring if ring is not None else StatsRing(cfg.LOG_PERIOD, device)
        self._drained = 0  # ring.counter at the last drain
        self.mb_top1_err = _ScalarWindow(cfg.LOG_PERIOD)
        self.mb_top5_err = _ScalarWindow(cfg.LOG_PERIOD)
        self.min_top1_err = 100.0
        self.min_top5_err = 100.0
        self.all_preds = self.all_labels = self._cursor = None  # [cap, K] stores and {rows filled, rows refused}
        self.cap = 0
        self.reset()

    def reset(self):
        self.mb_top1_err.reset()
        self.mb_top5_err.reset()
        self.num_top1_mis = 0
        self.num_top5_mis = 0
        self.num_samples = 0
        self._appended = 0  # rows handed to update_predictions this epoch (the host's count of the cursor)
        if self._cursor is not None:
            self._cursor.zero_()
        if self.per_class is not None:
            self.per_class.reset()

    def iter_tic(self):
        self._tic = time.perf_counter()

    def iter_toc(self):
        self._lap = time.perf_counter() - self._tic

    def update_stats(self, preds, labels):
        """Single-label: the batch's errors, one launch, no host read (train_net.py:227-243).  Multi-label: nothing, as
        eval_epoch computes no errors then."""
        if self._multi_label:
            return
        from slowfast.models.step_tail import topk_errors
        preds = preds.detach().float()
        topk_errors(preds, labels, self._cfg.TRAIN.TOPK, self.ring)
        if self.per_class is not None:  # the same batch, one more launch, still nothing read
            self.per_class.update(preds, labels)

    def update_predictions(self, preds, labels):
        """Multi-label: append the batch to the device store (utils/meters.py:623-632).  Single-label: nothing — the
        reference's list is never read then."""
        if not self._multi_label:
            return
        import sfhip
        preds = preds.detach().float()  # fp16 / bf16 predictions of an autocast forward are converted, as the labels are
        if self._cursor is None:
            self.cap = int(self.max_iter) * int(preds.shape[0])
            self.all_preds = torch.empty((self.cap, preds.shape[1]), dtype=torch.float32, device=preds.device)
            self.all_labels = torch.empty_like(self.all_preds)
            self._cursor = torch.zeros((2,), dtype=torch.int32, device=preds.device)
        sfhip.rows_append(preds, labels if labels.dtype == torch.float32 else labels.float(), self.all_preds,
                          self.all_labels, self._cursor)
        self._appended += int(preds.shape[0])

    def _fold(self, top1_err, top5_err, mb_size):
        """ValMeter.update_stats (utils/meters.py:609-621) for one batch's values."""
        self.mb_top1_err.add_value(top1_err)
        self.mb_top5_err.add_value(top5_err)
        self.num_top1_mis += top1_err * mb_size
        self.num_top5_mis += top5_err * mb_size
        self.num_samples += mb_size

    def drain(self):
        """Fold the rows written since the last drain; returns how many there were."""
        from slowfast.models.step_tail import KIND_EVAL
        world = max(int(self._cfg.NUM_GPUS), 1)
        rows = _drain_ring(self.ring, self._drained, world, "DeviceValMeter")
        for i, (_, top1, top5, flag, n, bad, kind) in enumerate(rows, self._drained):
            if kind != KIND_EVAL:
                raise RuntimeError("DeviceValMeter: ring row {} was not written by sf_topk_errors (kind {:g}) — give the "
                                   "validation meter a ring of its own".format(i, kind))
            if bad != 0:
                raise ValueError("DeviceValMeter: batch {} had label(s) outside [0, classes) ({:g} per rank on "
                                 "average)".format(i, bad))
            if flag != 0:
                _LOG.warning("DeviceValMeter: batch {} had NaN or infinite predictions; those rows count as "
                             "wrong".format(i))
            self._fold(top1, top5, int(round(n)) * world)
        self._drained += len(rows)
        return len(rows)

    def log_iter_stats(self, cur_epoch, cur_iter):
        if (cur_iter + 1) % self._cfg.LOG_PERIOD != 0:
            return None
        stats = {
            "_type": "val_iter",
            "epoch": "{}/{}".format(cur_epoch + 1, self._cfg.SOLVER.MAX_EPOCH),
            "iter": "{}/{}".format(cur_iter + 1, self.max_iter),
            "time_diff": self._lap,
            "eta": str(datetime.timedelta(seconds=int(self._lap * (self.max_iter - cur_iter - 1)))),
            "gpu_mem": "{:.2f} GB".format(DeviceTrainMeter._gpu_mem()),
        }
        if not self._multi_label:
            self.drain()
            stats["top1_err"] = self.mb_top1_err.get_win_median()
            stats["top5_err"] = self.mb_top5_err.get_win_median()
        _LOG.info(format_json_stats(stats))
        return stats

    def _epoch_map(self):
        """mAP of the epoch's rows: every rank's filled rows gathered once, `sf_map`, one copy."""
        import sfhip
        import slowfast.utils.distributed as du
        if self._cursor is None or self._appended == 0:
            raise RuntimeError("DeviceValMeter: no predictions were recorded this epoch")
        n = min(self._appended, self.cap)
        preds, labels, cursor = self.all_preds[:n], self.all_labels[:n], self._cursor
        if int(self._cfg.NUM_GPUS) > 1:
            preds, labels, cursor = du.all_gather([preds, labels, cursor])
        out = sfhip.mean_ap(preds, labels)
        host = torch.cat([out, cursor.double()]).cpu().tolist()  # the one device-to-host copy of the epoch
        cursors = host[3:]
        if any(v != 0 for v in cursors[1::2]):
            raise RuntimeError("DeviceValMeter: {} row(s) did not fit the prediction store (cap = {} rows = max_iter {} "
                               "x the first batch's rows)".format(int(sum(cursors[1::2])), self.cap, self.max_iter))
        if any(v != n for v in cursors[0::2]):
            raise RuntimeError("DeviceValMeter: the ranks stored {} rows, {} were expected on each".format(
                [int(v) for v in cursors[0::2]], n))
        return _checked_map(host[:3], "DeviceValMeter")

    def log_epoch_stats(self, cur_epoch):
        stats = {
            "_type": "val_epoch",
            "epoch": "{}/{}".format(cur_epoch + 1, self._cfg.SOLVER.MAX_EPOCH),
            "time_diff": self._lap,
            "gpu_mem": "{:.2f} GB".format(DeviceTrainMeter._gpu_mem()),
        }
        _ram_field(stats)
        if self._multi_label:
            stats["map"] = self._epoch_map()
        else:
            self.drain()
            top1_err = self.num_top1_mis / self.num_samples
            top5_err = self.num_top5_mis / self.num_samples
            self.min_top1_err = min(self.min_top1_err, top1_err)
            self.min_top5_err = min(self.min_top5_err, top5_err)
            stats["top1_err"] = top1_err
            stats["top5_err"] = top5_err
            stats["min_top1_err"] = self.min_top1_err
            stats["min_top5_err"] = self.min_top5_err
        _LOG.info(format_json_stats(stats))
        return stats


# ---------------------------------------------------------------------------------------------- detection (AVA) meter
def get_ava_mini_groundtruth(full_groundtruth):
    """The ground truth of the "subset" of the AVA validation set, the frames with second % 4 == 0
    (utils/meters.py:28-43): faster evaluation while training."""
    ret = [collections.defaultdict(list), collections.defaultdict(list), collections.defaultdict(list)]
    for i in range(3):
        for key in full_groundtruth[i].keys():
            if int(key.split(",")[1]) % 4 == 0:
                ret[i][key] = full_groundtruth[i][key]
    return ret


class DeviceAVAMeter(object):
    """AVAMeter (utils/meters.py:46-213) for a detection eval_epoch / test that never reads a prediction on the host.
    `update_stats(preds, ori_boxes, metadata)` copies the batch into three device stores (row counts are host-known
    shapes: plain copies into preallocated, doubling stores — no kernel, no sync); `finalize_metrics` runs
    `sf_ava_match` + `sf_ava_ap` over the stored rows against ground-truth tables built on the host ONCE (in
    `__init__`) and makes ONE device-to-host copy: the mAP, two refusal counters and the per-class AP.  The reference
    keeps a Python list of batches, pickles every batch across ranks (train_net.py:209-213) and walks every (image,
    class) pair in numpy; with several processes `all_gather()` here is one collective per store per epoch.

    mode: "val" or "test" ("train" raises: the training side of AVAMeter is loss and lr only — DeviceTrainMeter).
    The full ground truth is used in test mode or with AVA.FULL_TEST_ON_VAL, the mini one (second % 4 == 0) otherwise.
    `full_map` is the mAP at IoU 0.5, `per_class_ap` maps category names to AP (the evaluator's
    PascalBoxes_PerformanceByCategory/AP@0.5IOU/<name> entries)."""

    def __init__(self, overall_iters, cfg, mode, video_idx_to_name=None):
        import os
        from slowfast.utils import ava_eval_helper as H
        if mode == "train":
            raise ValueError("DeviceAVAMeter evaluates detections (mode 'val' or 'test'); the training loop's loss / lr "
                             "statistics are DeviceTrainMeter's")
        if mode not in ("val", "test"):
            raise ValueError("DeviceAVAMeter: unknown mode {!r} (expected 'val' or 'test')".format(mode))
        self.cfg = cfg
        self.mode = mode
        self.lr = None
        self.loss = _ScalarWindow(cfg.LOG_PERIOD)
        self.full_ava_test = bool(cfg.AVA.FULL_TEST_ON_VAL)
        self.overall_iters = overall_iters
        self._tic, self._lap = time.perf_counter(), 0.0
        self.excluded_keys = H.read_exclusions(os.path.join(cfg.AVA.ANNOTATION_DIR, cfg.AVA.EXCLUSION_FILE))
        self.categories, self.class_whitelist = H.read_labelmap(
            os.path.join(cfg.AVA.ANNOTATION_DIR, cfg.AVA.LABEL_MAP_FILE))
        self.full_groundtruth = H.read_csv(os.path.join(cfg.AVA.ANNOTATION_DIR, cfg.AVA.GROUNDTRUTH_FILE),
                                           self.class_whitelist)
        self.mini_groundtruth = get_ava_mini_groundtruth(self.full_groundtruth)
        self.video_idx_to_name = list(video_idx_to_name) if video_idx_to_name is not None else \
            H.load_video_names(cfg, False)
        self.uses_full_groundtruth = mode == "test" or self.full_ava_test
        self._tables = None  # built on the first finalize_metrics: the number of classes is the predictions'
        self.all_preds = self.all_ori_boxes = self.all_metadata = None  # device stores [cap, C], [cap, 5], [cap, 2]
        self.rows = 0
        self.full_map = None
        self.per_class_ap = {}

    # ------------------------------------------------------------------ the loop's side
    def iter_tic(self):
        self._tic = time.perf_counter()

    def iter_toc(self):
        self._lap = time.perf_counter() - self._tic

    def reset(self):
        self.loss.reset()
        self.rows = 0  # the stores keep their memory

    @property
    def cap(self):
        return 0 if self.all_preds is None else int(self.all_preds.shape[0])

    def _reserve(self, n, preds):
        """Room for n more rows: the first batch sizes the stores for overall_iters batches like it, later ones double."""
        need = self.rows + n
        if need <= self.cap:
            return
        cap = max(need, 2 * self.cap, int(self.overall_iters) * n)
        stores = []
        for old, width in ((self.all_preds, preds.shape[1]), (self.all_ori_boxes, 5), (self.all_metadata, 2)):
            new = torch.empty((cap, width), dtype=torch.float32, device=preds.device)
            if old is not None and self.rows:
                new[:self.rows].copy_(old[:self.rows])
            stores.append(new)
        self.all_preds, self.all_ori_boxes, self.all_metadata = stores

    def update_stats(self, preds, ori_boxes, metadata, loss=None, lr=None):
        """AVAMeter.update_stats (utils/meters.py:151-168): preds [n, C], ori_boxes [n, 5], metadata [n, 2] of any
        float / integer type, on the GPU."""
        if not (preds.is_cuda and ori_boxes.is_cuda and metadata.is_cuda):
            raise ValueError("DeviceAVAMeter.update_stats: preds, ori_boxes and metadata are GPU tensors (the "
                             "evaluation runs on the device; there is no host route)")
        n = int(preds.shape[0])
        if preds.dim() != 2 or tuple(ori_boxes.shape) != (n, 5) or tuple(metadata.shape) != (n, 2):
            raise ValueError("DeviceAVAMeter.update_stats: preds [n, C], ori_boxes [n, 5] and metadata [n, 2], got {}, "
                             "{} and {}".format(tuple(preds.shape), tuple(ori_boxes.shape), tuple(metadata.shape)))
        if self.all_preds is not None and preds.shape[1] != self.all_preds.shape[1]:
            raise ValueError("DeviceAVAMeter.update_stats: {} classes, the earlier batches had {}".format(
                preds.shape[1], self.all_preds.shape[1]))
        if n:
            self._reserve(n, preds)
            lo, hi = self.rows, self.rows + n
            self.all_preds[lo:hi].copy_(preds.detach())  # converts fp16 / bf16 / int64 on the way
            self.all_ori_boxes[lo:hi].copy_(ori_boxes.detach())
            self.all_metadata[lo:hi].copy_(metadata.detach())
            self.rows = hi
        if loss is not None:
            self.loss.add_value(loss)
        if lr is not None:
            self.lr = lr

    def log_iter_stats(self, cur_epoch, cur_iter):
        """AVAMeter.log_iter_stats (utils/meters.py:83-127) for the val / test records."""
        if (cur_iter + 1) % self.cfg.LOG_PERIOD != 0:
            return None
        eta = str(datetime.timedelta(seconds=int(self._lap * (self.overall_iters - cur_iter))))
        stats = {"_type": "{}_iter".format(self.mode), "cur_iter": "{}".format(cur_iter + 1), "eta": eta,
                 "time_diff": self._lap, "mode": self.mode}
        if self.mode == "val":
            stats["cur_epoch"] = "{}".format(cur_epoch + 1)
        _LOG.info(format_json_stats(stats))
        return stats

    # ------------------------------------------------------------------ the epoch's end
    def groundtruth_tables(self, num_classes, device):
        """The device tables of the ground truth this meter evaluates against (built and uploaded once)."""
        from slowfast.utils.ava_eval_helper import GroundTruthTables
        if self._tables is None or self._tables.num_classes != num_classes:
            gt = self.full_groundtruth if self.uses_full_groundtruth else self.mini_groundtruth
            self._tables = GroundTruthTables(gt, self.excluded_keys, self.class_whitelist, self.video_idx_to_name,
                                             num_classes, device=device)
        return self._tables

    def all_gather(self):
        """Every rank's rows: (preds, ori_boxes, metadata), or None when no rank recorded a row.  One process: the
        stores' filled part, nothing else.  Several (the size of the default process group): the ranks exchange their
        row counts and class counts — read on the host once (16 bytes per rank), because the padded height is a shape
        — then every store is padded to the largest count, gathered ONCE and compacted: three collectives per epoch in
        place of the reference's pickled gather per batch (train_net.py:209-213).  A rank without rows (or without a
        store: it never saw a batch) takes part with empty stores, so no rank waits in a collective for another."""
        import slowfast.utils.distributed as du
        world = du.get_world_size()
        if world <= 1:
            if self.all_preds is None or self.rows == 0:
                return None
            return tuple(t[:self.rows] for t in (self.all_preds, self.all_ori_boxes, self.all_metadata))
        have = self.all_preds is not None
        dev = self.all_preds.device if have else torch.device("cuda", torch.cuda.current_device())
        mine = torch.tensor([[self.rows if have else 0, self.all_preds.shape[1] if have else 0]], dtype=torch.int64,
                            device=dev)
        sizes = du.all_gather([mine])[0].cpu().tolist()  # [world][2]
        counts = [int(n) for n, _ in sizes]
        widths = {int(c) for n, c in sizes if n}
        if not widths:
            return None
        if len(widths) != 1:
            raise ValueError("DeviceAVAMeter: the ranks recorded predictions of {} classes".format(sorted(widths)))
        pad = max(counts)
        out = []
        for store, width in ((self.all_preds, widths.pop()), (self.all_ori_boxes, 5), (self.all_metadata, 2)):
            padded = torch.zeros((pad, width), dtype=torch.float32, device=dev)
            if have and self.rows:
                padded[:self.rows].copy_(store[:self.rows])
            whole = du.all_gather([padded])[0]
            out.append(torch.cat([whole[r * pad:r * pad + n] for r, n in enumerate(counts)], dim=0))
        return tuple(out)

    def finalize_metrics(self, log=True):
        """AVAMeter.finalize_metrics (utils/meters.py:170-195): five launches and ONE device-to-host copy (with
        several ranks, also the row counts in `all_gather`)."""
        from slowfast.utils import ava_eval_helper as H
        gathered = self.all_gather()  # first: every rank enters the collectives, whatever it recorded
        if gathered is None:
            raise RuntimeError("DeviceAVAMeter: no predictions were recorded this epoch")
        preds, boxes, meta = gathered
        tables = self.groundtruth_tables(int(preds.shape[1]), preds.device)
        self.full_map, ap = H.device_frame_map(preds, boxes, meta, tables, who="DeviceAVAMeter")
        results = H.per_category_results(self.categories, self.full_map, ap)
        self.per_class_ap = {k[len(H.CATEGORY_KEY):]: v for k, v in results.items() if k.startswith(H.CATEGORY_KEY)}
        if log:
            _LOG.info(format_json_stats({"mode": self.mode, "map": self.full_map}))
        return self.full_map

    def log_epoch_stats(self, cur_epoch):
        """AVAMeter.log_epoch_stats (utils/meters.py:197-213)."""
        self.finalize_metrics(log=False)
        stats = {"_type": "{}_epoch".format(self.mode), "cur_epoch": "{}".format(cur_epoch + 1), "mode": self.mode,
                 "map": self.full_map, "gpu_mem": "{:.2f} GB".format(DeviceTrainMeter._gpu_mem())}
        _ram_field(stats)
        _LOG.info(format_json_stats(stats))
        return stats
