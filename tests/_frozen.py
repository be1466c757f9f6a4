"""Shared by the frozen-BN tests: the oracle's eval forward with the parameters as autograd leaves — the reference for a
training step through eval-mode BatchNorm layers (utils.misc.frozen_bn_stats; torch.nn.BatchNorm3d eval semantics: the
running statistics are constants, gamma and beta still receive gradients).  Computed once per (fixture, dtype)."""
import torch

from _util import case_inputs, load_case, seeded_state_dict

FIXTURES = ["slow_r18_s64", "dual_r50_s64", "dual_r50_subbn_s64", "shufflenet_w2_g3_s64", "ghostnet_w2_s64",
            "shufflenetv2_cfg1", "mobilenetv2_w1_s64"]
TINY = 1e-6  # a parameter whose fp64 gradient norm is below this fraction of the largest is bounded absolutely
_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")

_CASES = {}
_GRADS = {}


def case(name):
    """(z, meta, state_dict, clips) of a fixture, loaded once."""
    if name not in _CASES:
        z, meta = load_case(name)
        sd = seeded_state_dict(z["sd_keys"], z["sd_shapes"], meta["param_seed"])
        _CASES[name] = (z, meta, sd, case_inputs(meta))
    return _CASES[name]


def oracle_grads(name, dtype):
    """{parameter name: dL/dp (float64 tensor)} and the logits [N, classes] of
    cross_entropy(oracle eval forward logits, train/labels), parameters as leaves of dtype `dtype`."""
    key = (name, dtype)
    if key not in _GRADS:
        from oracle import slowfast_oracle as oracle
        z, meta, sd, xs = case(name)
        leaves, sdr = {}, {}
        for k, v in sd.items():
            if not v.is_floating_point():
                sdr[k] = v
            elif k.rsplit(".", 1)[-1] in _BUFFERS:
                sdr[k] = v.to(dtype)
            else:
                sdr[k] = leaves[k] = v.to(dtype).clone().requires_grad_(True)
        n = xs[0].shape[0]
        logits = oracle.FORWARDS[meta["model"]](sdr, [x.to(dtype) for x in xs], meta["hparams"],
                                                training=False)["logits"].reshape(n, -1)
        labels = torch.from_numpy(z["train/labels"]).long()
        torch.nn.functional.cross_entropy(logits, labels).backward()
        _GRADS[key] = ({k: (v.grad.detach().double() if v.grad is not None else None) for k, v in leaves.items()},
                       logits.detach().double())
    return _GRADS[key]


def tiny_parameters(name):
    """Names whose fp64 oracle gradient norm is below TINY of the largest parameter-gradient norm."""
    g64, _ = oracle_grads(name, torch.float64)
    top = max(float(g.norm()) for g in g64.values())
    return sorted(k for k, g in g64.items() if float(g.norm()) < TINY * top)
