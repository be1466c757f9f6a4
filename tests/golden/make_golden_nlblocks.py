"""Fixture of the two non-local blocks of wdf_attention_helper.py that no model instantiates: the reference's own
NonLocalBlock (:129-195) and Stripe_NonLocalBlock (:198-273) classes, run in train mode on the CPU with seeded non-zero
parameters and running statistics (paramgen.fill_state_dict — a fresh block is the identity), a seeded input and a seeded
upstream gradient.  Per case: state_dict keys and shapes, the output, dL/dx, every parameter gradient, the BN's running
statistics after the step, and the eval-mode output computed with them.  Inputs and upstream gradients are regenerated
from their seeds by the tests (a float64 checksum of the input is recorded).  Activation-sized tensors of more than
_nlblock_ref.SAMPLE_ABOVE elements are stored as a strided sample (_nlblock_ref.stored), which keeps the file at about
0.5 MB.

    python tests/golden/make_golden_nlblocks.py        (build container only: needs the reference tree)
writes tests/golden/nl_blocks.npz."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _refimport import import_reference  # noqa: E402
from paramgen import make_upstream  # noqa: E402
from _nlblock_ref import build_kwargs, fill_case, is_param, stored  # noqa: E402

PARAM_SEED = 5151
# inter_channels = C // 2 must be a width the attention kernels take (a multiple of 4): 73 // 2 = 36 — an odd C above a
# wavefront's 64 lanes, so the scalar kernels run more than one channel chunk
CASES = [
    dict(name="st_mean_soft_s3", kind="Stripe_NonLocalBlock", C=32, thw=(3, 6, 5), stripe=3, pool_type="mean",
         instance="soft"),                                             # 9 positions, not a multiple of 16
    dict(name="st_meanmax_dot_s2", kind="Stripe_NonLocalBlock", C=32, thw=(3, 6, 5), stripe=2, pool_type="meanmax",
         instance="dot"),
    dict(name="st_max_soft_s1_c73", kind="Stripe_NonLocalBlock", C=73, thw=(2, 4, 70), stripe=1, pool_type="max",
         instance="soft", qk_scale=0.3),                             # hs*W = 280 positions per stripe
    dict(name="st_max_dot_s6", kind="Stripe_NonLocalBlock", C=32, thw=(3, 6, 5), stripe=6, pool_type="max",
         instance="dot"),                                              # S = H: one row per stripe
    dict(name="nl_soft", kind="NonLocalBlock", C=32, thw=(3, 6, 5), sub_sample=False, bn_layer=True, instance="soft"),
    dict(name="nl_dot_sub", kind="NonLocalBlock", C=32, thw=(2, 6, 7), sub_sample=True, bn_layer=True,
         instance="dot"),                                              # odd W is floored; N_q = 4 N_k
    dict(name="nl_soft_sub_nobn", kind="NonLocalBlock", C=32, thw=(2, 6, 7), sub_sample=True, bn_layer=False,
         instance="soft"),
]


def main():
    import_reference()
    from slowfast.models import wdf_attention_helper as ref
    if not hasattr(ref, "F"):
        # the reference file calls F.softmax (:187, :262) without importing torch.nn.functional: its 'soft' blocks raise
        # NameError as shipped.  The name is supplied here, in this process only — STE-NVAN's original imports it.
        ref.F = torch.nn.functional
    out = {}
    metas = []
    for i, case in enumerate(CASES):
        torch.manual_seed(0)
        m = getattr(ref, case["kind"])(**build_kwargs(case))
        m.train()
        case = dict(case, param_seed=PARAM_SEED)
        fill_case(m, case)
        sd = m.state_dict()
        shape = (2, case["C"]) + tuple(case["thw"])
        meta = dict(case, thw=list(case["thw"]), shape=list(shape), input_seed=7100 + i, upstream_seed=8100 + i,
                    sd_keys=list(sd.keys()), sd_shapes=[list(v.shape) for v in sd.values()],
                    inter_channels=int(m.inter_channels))
        x = torch.from_numpy(np.random.RandomState(meta["input_seed"]).standard_normal(shape).astype(np.float32))
        g = torch.from_numpy(make_upstream(meta["upstream_seed"], shape))
        meta["input_sum"] = float(x.double().sum())
        x.requires_grad_(True)
        y = m(x)
        y.backward(g)
        pre = case["name"] + "/"
        out[pre + "out"] = stored(y.detach()).numpy()
        out[pre + "dx"] = stored(x.grad).numpy()
        for k, p in m.named_parameters():
            assert is_param(k)
            out[pre + "grad/" + k] = p.grad.numpy()
        for k, v in m.state_dict().items():
            if k.endswith(("running_mean", "running_var")):
                out[pre + "after/" + k] = v.detach().numpy().copy()
        m.eval()
        with torch.no_grad():
            out[pre + "eval_out"] = stored(m(x.detach())).numpy()
        metas.append(meta)
    out["meta"] = np.array(json.dumps(metas))
    path = os.path.join(HERE, "nl_blocks.npz")
    np.savez(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
