#!/usr/bin/env python3
"""One `sf_ce_topk_w` launch against one `sf_ce_topk` launch (csrc/step_tail.hip) at 64 x 3 (the driver-monitoring
configs) and 64 x 400 (Kinetics), resident logits, labels and weights.
Method: both arms warmed up, then ROUNDS rounds in which the arms alternate; an arm's round is REPS launches back to
back between two HIP events (the host issues a launch in far less than it runs), per launch; the figure is the median
round, the spread its min .. max.  Clocks not pinned.
usage: tools/microbench/weighted_loss_bench.py [out.txt]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import torch  # noqa: E402
from slowfast.models.step_tail import StatsRing, ce_topk, ce_topk_w  # noqa: E402

ROUNDS, REPS = 9, 200


def main():
    lines = ["weighted cross-entropy launch, %s, %d rounds of %d launches (HIP events), us per launch: median (min .. max)"
             % (torch.cuda.get_device_name(0), ROUNDS, REPS)]
    g = torch.Generator().manual_seed(0)
    for N, K in ((64, 3), (64, 400)):
        x = torch.randn(N, K, generator=g).cuda()
        y = torch.randint(0, K, (N,), generator=g).cuda()
        w = (torch.rand(K, generator=g) * 3.75 + 0.25).cuda()
        ring, out = StatsRing(8), torch.zeros(2, device="cuda")
        d = torch.empty((N, K), device="cuda")
        k_hi = min(5, K)
        arms = [("sf_ce_topk", lambda: ce_topk(x, y, k_hi, ring, out, dlogits=d)),
                ("sf_ce_topk_w", lambda: ce_topk_w(x, y, w, k_hi, ring, out, dlogits=d))]
        for _, fn in arms:
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n, _ in arms}
        for _ in range(ROUNDS):
            for name, fn in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / REPS)
        for name, _ in arms:
            t = times[name]
            lines.append("  %3d x %-4d %-14s %7.2f  (%.2f .. %.2f)" % (N, K, name, statistics.median(t), min(t), max(t)))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
