#!/usr/bin/env python3
"""Golden vectors of the grayscale models at the driver-monitoring YAMLs' own spatial strides, produced by running the
REFERENCE itself (CPU, fp32).

configs/TIRED/*_112*.yaml set RESNET.SPATIAL_STRIDES [[1,1],[1,1],[2,2],[2,2]] ([[1],[1],[2],[2]] for one pathway): res5
is crop/16 wide while the head's AvgPool3d window stays crop//32, stride 1, so the head is fully convolutional — pooled
extent 3 x 3 at crop 64 — and the TRAINING logits are [N, 1*3*3*classes] (head_helper.py:198-223).  The cases are
make_golden_gray.py's with that one override; fields, clips and seeds are the same (`run_case` is make_golden.py's):
  fast_r18_gray_tired_s64   fast_r18_gray_s64 + RESNET.SPATIAL_STRIDES [[1],[1],[2],[2]]
  dual_r18_gray_tired_s64   dual_r18_gray_s64 + RESNET.SPATIAL_STRIDES [[1,1],[1,1],[2,2],[2,2]]

`python tests/golden/make_golden_tired.py` writes the fixtures; `... check` prints the reference's fp32-against-fp64
floor in the measures of tests/test_tired_strides_gpu.py (make_golden_gray.fp32_floor)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_gray as gray  # noqa: E402
from _refimport import import_reference  # noqa: E402

STRIDES = {"fast_r18_gray_s64": [[1], [1], [2], [2]], "dual_r18_gray_s64": [[1, 1], [1, 1], [2, 2], [2, 2]]}

CASES = [dict(c, name=c["name"].replace("_s64", "_tired_s64"),
              over=c["over"] + ["RESNET.SPATIAL_STRIDES", STRIDES[c["name"]]]) for c in gray.CASES]


if __name__ == "__main__":
    torch.set_num_threads(8)
    get_cfg, build_model = import_reference()
    which = [a for a in sys.argv[1:] if a != "check"]
    mg.make_clip = gray.gray_clip  # run_case's clips: one channel
    for c in CASES:
        if which and c["name"] not in which:
            continue
        if "check" in sys.argv[1:]:
            gray.fp32_floor(c, get_cfg, build_model)
        else:
            mg.run_case(c, get_cfg, build_model)
