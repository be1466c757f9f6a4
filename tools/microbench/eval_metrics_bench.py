#!/usr/bin/env python3
"""The evaluation metrics against the host routes they replace.

  mAP        `device_map` at 1863 x 157 (Charades' validation set): one sf_map call and its 24-byte copy, against a
             copy of both matrices to the host plus the numpy `get_map`
  top-k      one `sf_topk_errors` launch at [8, 400] (nothing read back: the meter drains once per LOG_PERIOD), against
             `topks_correct` plus the two `.item()` of train_net.py:227-237
Method: every arm warmed up, then ROUNDS rounds in which the arms of a pair alternate; an arm's round is REPS calls
between two device synchronisations, host clock, per call; the figure is the median round, the spread its min .. max.
sf_map's device time alone: REPS calls back to back between two HIP events, per call.  Clocks not pinned.
usage: tools/microbench/eval_metrics_bench.py [out.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import torch  # noqa: E402
import sfhip  # noqa: E402
from slowfast.models.step_tail import StatsRing, topk_errors  # noqa: E402
from slowfast.utils.meters import device_map, get_map, topks_correct  # noqa: E402

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
        lines.append("  %-46s %9.1f us per call  (%.1f .. %.1f)" % (name, statistics.median(v) * 1e6, min(v) * 1e6,
                                                                   max(v) * 1e6))


def main():
    assert torch.cuda.is_available(), "eval_metrics_bench needs an MI355X"
    lines = ["eval_metrics_bench on %s, %d rounds x %d calls" % (torch.cuda.get_device_name(0), ROUNDS, REPS)]
    g = torch.Generator().manual_seed(0)
    n, c = 1863, 157
    preds = torch.rand(n, c, generator=g).cuda()
    labels = (torch.rand(n, c, generator=g) < 0.05).float().cuda()
    host = lambda: get_map(preds.cpu().numpy(), labels.cpu().numpy())  # noqa: E731
    dev = lambda: device_map(preds, labels)  # noqa: E731
    lines.append("mAP %d x %d: device %.17g, host %.17g" % (n, c, dev(), host()))
    report(lines, "mAP %d x %d" % (n, c), alternate([("copy to the host + numpy get_map", host),
                                                   ("device_map (sf_map + one 24-byte copy)", dev)]))
    out = torch.empty(3, dtype=torch.float64, device="cuda")
    for _ in range(3):
        sfhip.mean_ap(preds, labels, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(REPS):
        sfhip.mean_ap(preds, labels, out=out)
    e1.record()
    torch.cuda.synchronize()
    lines.append("  sf_map alone (both launches, HIP events)         %9.1f us per call" % (e0.elapsed_time(e1) * 1e3 / REPS))

    p8 = torch.rand(8, 400, generator=g).cuda()
    l8 = torch.randint(0, 400, (8,), generator=g).cuda()
    ring = StatsRing(10)

    def ref():
        a, b = [(1.0 - x / 8) * 100.0 for x in topks_correct(p8, l8, (1, 5))]
        return a.item(), b.item()
    report(lines, "top-k errors [8, 400]", alternate([("topks_correct + two .item()", ref),
                                                      ("sf_topk_errors (one launch, nothing read)",
                                                       lambda: topk_errors(p8, l8, 5, ring))]))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
