#!/usr/bin/env python3
"""DevicePerClassMeter.update against the host route it replaces.

  update     one `sf_confusion_update` launch on a batch (nothing read back: the meter is read once per epoch)
  host       `preds.cpu()` + `labels.cpu()` and the numpy loop a user writes today: arg-max per row, `np.add.at` into the
             confusion matrix, the label's rank for the top-k hits
Sizes: 64 rows x 3 classes (the fork's classifiers: thread per row, LDS counters) and 64 x 400 (Kinetics: wavefront per
row).  Also the epoch's end: `finalize()` (one `sf_class_report` launch + the one copy) at both sizes.
Method: every arm warmed up, then ROUNDS rounds in which the arms of a pair alternate; an arm's round is REPS calls
between two device synchronisations, host clock, per call; the figure is the median round, the spread its min .. max.
The kernel's device time alone: REPS calls back to back between two HIP events, per call.  Clocks not pinned.
usage: tools/microbench/per_class_bench.py [out.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from slowfast.utils.meters import DevicePerClassMeter  # noqa: E402

ROUNDS, REPS = 9, 20


def alternate(arms):
    for _, fn in arms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    total = {n: [] for n, _ in arms}
    for _ in range(ROUNDS):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                fn()
            torch.cuda.synchronize()
            total[name].append((time.perf_counter() - t0) / REPS)
    return total


def report(lines, title, total):
    lines.append(title)
    for name, v in total.items():
        lines.append("  %-50s %9.1f us per call  (%.1f .. %.1f)" % (name, statistics.median(v) * 1e6, min(v) * 1e6,
                                                                   max(v) * 1e6))


def host_update(preds, labels, conf, hits, k_hi):
    """The host route: two copies, then numpy (untied scores: np.argmax is the kernels' prediction)."""
    p, lab = preds.cpu().numpy(), labels.cpu().numpy()
    np.add.at(conf, (lab, p.argmax(1)), 1)
    rank = (p > p[np.arange(len(lab)), lab][:, None]).sum(1)
    np.add.at(hits[:, 0], lab[rank < 1], 1)
    np.add.at(hits[:, 1], lab[rank < k_hi], 1)


def main():
    assert torch.cuda.is_available(), "per_class_bench needs an MI355X"
    lines = ["per_class_bench on %s, %d rounds x %d calls" % (torch.cuda.get_device_name(0), ROUNDS, REPS)]
    g = torch.Generator().manual_seed(0)
    for n, k, k_hi in ((64, 3, 2), (64, 400, 5)):
        preds = torch.rand(n, k, generator=g).cuda()
        labels = torch.randint(0, k, (n,), generator=g).cuda()
        m = DevicePerClassMeter(k, k_hi)
        conf, hits = np.zeros((k, k), np.int64), np.zeros((k, 2), np.int64)
        # the two routes count the same before anything is timed
        m.update(preds, labels)
        host_update(preds, labels, conf, hits, k_hi)
        rep = m.finalize()
        assert np.array_equal(rep["confusion"].numpy(), conf) and np.array_equal(rep["hits"].numpy(), hits)
        report(lines, "update [%d, %d]" % (n, k), alternate([
            ("preds.cpu() + labels.cpu() + numpy", lambda: host_update(preds, labels, conf, hits, k_hi)),
            ("DevicePerClassMeter.update (one launch, nothing read)", lambda: m.update(preds, labels))]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(REPS):
            m.update(preds, labels)
        e1.record()
        torch.cuda.synchronize()
        lines.append("  %-50s %9.1f us per call" % ("sf_confusion_update back to back (HIP events)",
                                                   e0.elapsed_time(e1) * 1e3 / REPS))
        report(lines, "epoch end, K = %d" % k, alternate([
            ("finalize (sf_class_report + the one copy)", lambda: m.finalize())]))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
