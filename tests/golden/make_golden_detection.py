#!/usr/bin/env python3
"""Generate the committed detection fixtures by running the REFERENCE itself (CPU, fp32), AVA configs with
DETECTION.ENABLE: ResNetRoIHead over boxes.

Runs only in the build container (needs the reference tree); the GPU box and the test-suite only read the resulting
``tests/golden/*_ava_*.npz``.  Re-run: ``python tests/golden/make_golden_detection.py``.

detectron2's compiled ROIAlign does not exist here.  The reference binds ``ROIAlign`` as a module global of its
head_helper at import and ResNetRoIHead.__init__ looks it up at construction, so setting that attribute swaps in the
project's float64 restatement (tests/_roi_align_ref.py), which the CPU tests pin against analytic cases.

Every fixture holds data only: the resolved cfg (JSON), the seeds, the state_dict's key / shape list, the children,
the boxes and multi-hot labels, the eval probabilities, the train-mode probabilities (dropout off), the BCE loss and
sampled parameter gradients.
"""
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from _refimport import REF_ROOT, import_reference  # noqa: E402
from _roi_align_ref import ROIAlign as ROIAlignRef  # noqa: E402
from make_golden import CLIP_SEED, COMMON, PARAM_SEED, hparams_from_cfg, plain_cfg, small  # noqa: E402
from paramgen import fill_state_dict, make_clip, sample_activation  # noqa: E402

LABEL_SEED = 13

# 5 boxes over 2 clips at S = 64 (input pixels, res5 stride 16 -> a 4 x 4 map): an ordinary box, one partly outside
# the frame, one smaller than a feature cell, a full-frame box, and one more
BOXES = [[0, 8.0, 4.0, 40.0, 56.0],
         [0, -12.0, 20.0, 30.0, 80.0],
         [1, 30.5, 22.25, 36.75, 27.5],
         [1, 0.0, 0.0, 64.0, 64.0],
         [1, 12.0, 16.0, 52.0, 44.0]]

AVA = REF_ROOT + "/SlowFast/configs/AVA/"
CASES = [
    dict(name="slowfast_r50_ava_s64", yaml="SLOWFAST_32x2_R50_SHORT.yaml", model="SlowFast", batch=2, t=16,
         alpha=4, size=64, over=small(64, 16)),
    # the Slow 8x8 AVA YAML at its own NUM_FRAMES 4 (the ResNet class, single pathway)
    dict(name="slow_r50_ava_s64", yaml="SLOW_8x8_R50_SHORT.yaml", model="ResNet", batch=2, t=4, alpha=1, size=64,
         over=small(64, 4), single=True),
    # the fork's SlowFastDualAttention (CMDA laterals) on the AVA SlowFast YAML: dilated res5 + ResNetRoIHead
    dict(name="dual_r50_ava_s64", yaml="SLOWFAST_32x2_R50_SHORT.yaml", model="SlowFastDualAttention", batch=2, t=16,
         alpha=4, size=64, over=small(64, 16)),
]

GRAD_KEYS = {
    "SlowFast": ["s1.pathway0_stem.conv.weight", "s4.pathway0_res0.branch2.a.weight",
                 "s5.pathway0_res1.branch2.b.weight", "s5.pathway1_res2.branch2.b.weight",
                 "s5.pathway0_res2.branch2.c_bn.weight", "head.projection.weight", "head.projection.bias"],
    "ResNet": ["s1.pathway0_stem.conv.weight", "s3.pathway0_res0.branch1.weight", "s5.pathway0_res0.branch2.b.weight",
               "s5.pathway0_res1.branch2.b_bn.weight", "head.projection.weight", "head.projection.bias"],
    "SlowFastDualAttention": ["s1.pathway1_stem.conv.weight", "s3_fuse.attention_channel_f2s.conv.weight",
                              "s5.pathway0_res1.branch2.b.weight", "s5.pathway1_res0.branch2.b.weight",
                              "head.projection.weight", "head.projection.bias"],
}


def run_case(case, get_cfg, build_model):
    t0 = time.time()
    cfg = get_cfg()
    cfg.merge_from_file(AVA + case["yaml"])
    over = COMMON + ["MODEL.MODEL_NAME", case["model"]] + case["over"]
    cfg.merge_from_list(over)
    assert cfg.DETECTION.ENABLE and cfg.MODEL.HEAD_ACT == "sigmoid"
    torch.manual_seed(0)
    model = build_model(cfg)
    assert isinstance(model.head.s0_roi, ROIAlignRef)
    sd = model.state_dict()
    fill_state_dict(sd, PARAM_SEED)
    model.load_state_dict(sd)
    slow, fast = make_clip(CLIP_SEED, case["batch"], case["t"], case["alpha"], case["size"])
    single = bool(case.get("single"))
    boxes = torch.tensor(BOXES, dtype=torch.float32)
    labels = (np.random.RandomState(LABEL_SEED).rand(len(BOXES), cfg.MODEL.NUM_CLASSES) < 0.1).astype(np.float32)

    def clips(grad=False):
        arrs = [fast] if single else [slow, fast]
        return [torch.from_numpy(a.copy()).requires_grad_(grad) for a in arrs]

    head = model.head
    out = {
        "meta": json.dumps(dict(name=case["name"], model=case["model"], yaml="AVA/" + case["yaml"],
                                overrides=[str(o) if not isinstance(o, (int, float, bool)) else o for o in over],
                                cfg_dump=plain_cfg(cfg), hparams=hparams_from_cfg(cfg), param_seed=PARAM_SEED,
                                clip_seed=CLIP_SEED, label_seed=LABEL_SEED, batch=case["batch"], t=case["t"],
                                alpha=case["alpha"], size=case["size"], single=single, torch=torch.__version__)),
        "sd_keys": np.array(list(sd.keys())),
        "sd_shapes": np.array([json.dumps(list(v.shape)) for v in sd.values()]),
        "children": np.array([n for n, _ in model.named_children()]),
        "head_children": np.array([n for n, _ in head.named_children()]),
        "head_children_types": np.array([type(m).__name__ for _, m in head.named_children()]),
        "boxes": boxes.numpy(),
        "labels": labels,
    }

    # ---- eval (test_net.py: preds = model(inputs, meta["boxes"]))
    model.eval()
    with torch.no_grad():
        probs = model(clips(), boxes)
    out["eval/out"] = probs.numpy()

    # ---- train forward + backward (train_net.py:71-96), dropout off so it is deterministic; BCE as LOSS_FUNC bce
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.train()
    p = model(clips(grad=True), boxes)
    loss = torch.nn.BCELoss(reduction="mean")(p, torch.from_numpy(labels))
    loss.backward()
    out["train/out"] = p.detach().numpy()
    out["train/loss"] = np.array([loss.item()], np.float64)
    params = dict(model.named_parameters())
    for k in GRAD_KEYS[case["model"]]:
        g = params[k].grad
        s, amax, mean = sample_activation(g.numpy(), 4096)
        out["grad/" + k] = s
        out["grad/" + k + "/stats"] = np.array([amax, float(g.norm())], np.float64)
    path = os.path.join(HERE, case["name"] + ".npz")
    np.savez_compressed(path, **out)
    print("%-22s %5.1fs  %6.1f KB  loss=%.5f  max-prob=%.4f" % (
        case["name"], time.time() - t0, os.path.getsize(path) / 1024, loss.item(), float(probs.max())))


if __name__ == "__main__":
    torch.set_num_threads(8)
    get_cfg, build_model = import_reference()
    import slowfast.models.head_helper as ref_head_helper
    ref_head_helper.ROIAlign = ROIAlignRef  # detectron2's op, restated (module docstring)
    which = sys.argv[1:]
    for c in CASES:
        if not which or c["name"] in which:
            run_case(c, get_cfg, build_model)
