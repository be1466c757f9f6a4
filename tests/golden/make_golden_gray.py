#!/usr/bin/env python3
"""Golden vectors of the grayscale (one input channel) models, produced by running the REFERENCE itself (CPU, fp32).

Same fields as make_golden.py's model fixtures — `run_case` is that file's, imported — for the driver-monitoring family
of the fork (configs/TIRED/*, configs/WHEEL/*: DATA.INPUT_CHANNEL_NUM [1] / [1, 1], MEAN [0.45], STD [0.225],
ResNet-18 bottleneck pathways), at the default SPATIAL_STRIDES so that the head pools to 1 x 1 x 1 in training:
  fast_r18_gray_s64   ResNet, MODEL.ARCH fast (the fork's Fast-only single pathway, video_model_builder.py:73-79, :89),
                      WIDTH_PER_GROUP 16 (TIRED_FAST_NLN_8x8_R50_112.yaml)
  dual_r18_gray_s64   SlowFastDualAttention, ALPHA 8, BETA_INV 8 (DUAL_TIRED_SLOWFAST_8x8_R18_HALF_112_GRAY.yaml)
The clips are paramgen.make_clip(..., channels=1): the tests regenerate them with the same call when the fixture's
cfg_dump has DATA.INPUT_CHANNEL_NUM[0] == 1.

`python tests/golden/make_golden_gray.py` writes the fixtures; `... check` instead runs every case in fp32 AND fp64 on
the reference and prints the measures of tests/test_gray_models_gpu.py between the two: the floor of fp32 itself, which
has to sit inside the tests' bounds for a fixture to be worth committing."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import paramgen  # noqa: E402
from _refimport import import_reference  # noqa: E402

GRAY = ["DATA.MEAN", [0.45], "DATA.STD", [0.225], "MODEL.NUM_CLASSES", 3]
R18 = ["RESNET.DEPTH", 18]

CASES = [
    dict(name="fast_r18_gray_s64", yaml="SLOW_8x8_R50.yaml", model="ResNet", batch=2, t=16, alpha=1, size=64,
         single=True,
         over=GRAY + R18 + ["DATA.INPUT_CHANNEL_NUM", [1], "MODEL.ARCH", "fast", "RESNET.WIDTH_PER_GROUP", 16,
                            "RESNET.NUM_BLOCK_TEMP_KERNEL", [[2], [2], [2], [2]]] + mg.small(64, 16)),
    dict(name="dual_r18_gray_s64", yaml=mg.DUAL_YAML, model="SlowFastDualAttention", batch=2, t=16, alpha=8, size=64,
         over=GRAY + R18 + ["DATA.INPUT_CHANNEL_NUM", [1, 1], "SLOWFAST.ALPHA", 8, "SLOWFAST.BETA_INV", 8,
                            "RESNET.NUM_BLOCK_TEMP_KERNEL", [[2, 2], [2, 2], [2, 2], [2, 2]]] + mg.small(64, 16),
         grad_keys=["s1.pathway0_stem.conv.weight"] + mg.GRAD_KEYS["SlowFastDualAttention"]),
]


def gray_clip(seed, batch, t_fast, alpha, size):
    return paramgen.make_clip(seed, batch, t_fast, alpha, size, channels=1)


def fp32_floor(case, get_cfg, build_model):
    """The reference in fp32 against itself in fp64, in the measures of the GPU tests."""
    res = {}
    for dt in (torch.float32, torch.float64):
        cfg = get_cfg()
        cfg.merge_from_file(mg.ref_yaml(case["yaml"]))
        cfg.merge_from_list(mg.COMMON + ["MODEL.MODEL_NAME", case["model"]] + case["over"])
        torch.manual_seed(0)
        model = build_model(cfg)
        paramgen.fill_state_dict(model.state_dict(), mg.PARAM_SEED)
        model = model.to(dt)
        slow, fast = gray_clip(mg.CLIP_SEED, case["batch"], case["t"], case["alpha"], case["size"])
        arrs = [fast] if case.get("single") else [slow, fast]
        model.eval()
        with torch.no_grad():
            ev = model([torch.from_numpy(a).to(dt) for a in arrs])
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        model.train()
        logits = model([torch.from_numpy(a).to(dt) for a in arrs])
        labels = torch.from_numpy(np.random.RandomState(11).randint(0, cfg.MODEL.NUM_CLASSES, case["batch"]))
        loss = torch.nn.functional.cross_entropy(logits, labels)
        loss.backward()
        params = dict(model.named_parameters())
        keys = case.get("grad_keys") or mg.GRAD_KEYS[case["model"]]
        res[dt] = (ev.double().numpy(), logits.detach().double().numpy(), float(loss),
                   {k: params[k].grad.double().numpy() for k in keys})

    def rel(a, b):
        return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))

    a, b = res[torch.float32], res[torch.float64]
    print("%-20s fp32 vs fp64 of the reference: eval out %.2e  train logits %.2e  |loss diff| %.2e" % (
        case["name"], rel(a[0], b[0]), rel(a[1], b[1]), abs(a[2] - b[2])))
    for k in a[3]:
        g, r = a[3][k], b[3][k]
        print("    grad %-52s L2rel %.3e  |g| %.4e vs %.4e" % (
            k, np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-30), np.linalg.norm(g), np.linalg.norm(r)))


if __name__ == "__main__":
    torch.set_num_threads(8)
    get_cfg, build_model = import_reference()
    which = [a for a in sys.argv[1:] if a != "check"]
    mg.make_clip = gray_clip  # run_case's clips: one channel
    for c in CASES:
        if which and c["name"] not in which:
            continue
        if "check" in sys.argv[1:]:
            fp32_floor(c, get_cfg, build_model)
        else:
            mg.run_case(c, get_cfg, build_model)
