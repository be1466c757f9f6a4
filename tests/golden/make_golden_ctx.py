"""Fixture of the two attention blocks of wdf_attention_helper.py that no model instantiates: the reference's own
ChannelAttention (:97-124) and ContextBlock3D (:289-379) classes, run in train mode on the CPU with seeded non-zero
parameters (paramgen.fill_state_dict — a fresh ContextBlock3D is the identity), a seeded input and a seeded upstream
gradient.  Per case: state_dict keys and shapes, the output, dL/dx and every parameter gradient.  Inputs and upstream
gradients are regenerated from their seeds by the tests (a float64 checksum of the input is recorded).

    python tests/golden/make_golden_ctx.py        (build container only: needs the reference tree)
writes tests/golden/ctx_blocks.npz."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _refimport import import_reference  # noqa: E402
from paramgen import fill_state_dict, make_upstream  # noqa: E402

PARAM_SEED = 4242
THW = (3, 7, 9)  # 189 positions: two workgroups' partials per sample in the pooling kernels
CASES = [
    dict(name="ca_c8_r16", kind="ChannelAttention", C=8, reduction=16),        # inner = 2 (8 // 16 == 0)
    dict(name="ca_c64_r16", kind="ChannelAttention", C=64, reduction=16),
    dict(name="gc_att_c32_r1", kind="ContextBlock3D", C=32, ratio=1.0, pooling_type="att"),
    dict(name="gc_att_c32_r025", kind="ContextBlock3D", C=32, ratio=0.25, pooling_type="att"),
    dict(name="gc_avg_c30_r05", kind="ContextBlock3D", C=30, ratio=0.5, pooling_type="avg"),
]


def main():
    import_reference()
    from slowfast.models.wdf_attention_helper import ChannelAttention, ContextBlock3D
    out = {}
    metas = []
    for i, case in enumerate(CASES):
        torch.manual_seed(0)
        if case["kind"] == "ChannelAttention":
            m = ChannelAttention(case["C"], reduction=case["reduction"])
        else:
            m = ContextBlock3D(case["C"], ratio=case["ratio"], pooling_type=case["pooling_type"])
        m.train()
        sd = m.state_dict()
        fill_state_dict(sd, PARAM_SEED)
        shape = (2, case["C"]) + THW
        meta = dict(case, shape=list(shape), input_seed=7000 + i, upstream_seed=8000 + i, param_seed=PARAM_SEED,
                    sd_keys=list(sd.keys()), sd_shapes=[list(v.shape) for v in sd.values()])
        x = torch.from_numpy(np.random.RandomState(meta["input_seed"]).standard_normal(shape).astype(np.float32))
        g = torch.from_numpy(make_upstream(meta["upstream_seed"], shape))
        meta["input_sum"] = float(x.double().sum())
        x.requires_grad_(True)
        y = m(x)
        y.backward(g)
        pre = case["name"] + "/"
        out[pre + "out"] = y.detach().numpy()
        out[pre + "dx"] = x.grad.numpy()
        for k, p in m.named_parameters():
            out[pre + "grad/" + k] = p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
        metas.append(meta)
    out["meta"] = np.array(json.dumps(metas))
    path = os.path.join(HERE, "ctx_blocks.npz")
    np.savez(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
