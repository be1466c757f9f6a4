#!/usr/bin/env python3
"""Time of slowfast.models.gradcam.class_gradients on the `dual` workload of bench.py (SlowFastDualAttention R50,
T = 32, 224^2) at ONE clip, targets s2 and s5, against the train-mode backward of the same model at the same clip —
before the eval-mode tape, the only way to get any gradient out of it (forward in train mode, cross-entropy,
loss.backward(): every weight gradient included).  Also timed: the plain eval forward (what class_gradients adds to
is its backward from the target on) and GradVideoCam.generate_cam_videos (class_gradients + the two CAM kernels per
pathway).  Wall time per call between device synchronisations, GRADCAM_ITERS calls after 3 warm ones.
usage: tools/microbench/gradcam_bench.py [--targets s2,s5]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import torch  # noqa: E402

ITERS = int(os.environ.get("GRADCAM_ITERS", "10"))


def timeit(fn, iters=ITERS):
    """milliseconds per call."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", default="s2,s5")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gradcam_bench needs an MI355X"
    import bench
    from slowfast.models import gradcam
    dev = torch.device("cuda:0")
    with contextlib.redirect_stdout(io.StringIO()):
        cfg, model, _, _ = bench.build("dual", dev)
    clips = bench.synthetic_clips(cfg, 1, dev, 1)
    label = torch.zeros(1, dtype=torch.long, device=dev)
    res = {"workload": "dual", "clips": 1, "iters": ITERS}

    def train_backward():
        model.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(model([c.clone() for c in clips]), label).backward()

    model.train()
    res["train_forward_backward_ms"] = timeit(train_backward)
    model.zero_grad(set_to_none=True)
    model.eval()

    def eval_forward():
        with torch.no_grad():
            model([c.clone() for c in clips])

    res["eval_forward_ms"] = timeit(eval_forward)
    for target in a.targets.split(","):
        res["class_gradients_%s_ms" % target] = timeit(
            lambda: gradcam.class_gradients(model, [c.clone() for c in clips], target))
        cam = gradcam.GradVideoCam(model, target)
        res["generate_cam_videos_%s_ms" % target] = timeit(lambda: cam.generate_cam_videos([c.clone() for c in clips]))
        res["class_gradients_%s_over_train_backward" % target] = (
            res["class_gradients_%s_ms" % target] / res["train_forward_backward_ms"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
