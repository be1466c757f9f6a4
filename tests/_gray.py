"""Shared helpers of the grayscale (one input channel) tests: the fixtures' clips and model construction."""
import contextlib
import io

import torch

from _util import load_case, make_clip, seeded_state_dict

GRAY_CASES = ["fast_r18_gray_s64", "dual_r18_gray_s64"]


def gray_inputs(meta):
    """The clips make_golden_gray.py fed the reference: paramgen.make_clip(..., channels=1)."""
    assert meta["cfg_dump"]["DATA"]["INPUT_CHANNEL_NUM"][0] == 1
    slow, fast = make_clip(meta["clip_seed"], meta["batch"], meta["t"], meta["alpha"], meta["size"], channels=1)
    arrs = [fast] if meta.get("single") else [slow, fast]
    return [torch.from_numpy(a) for a in arrs]


def build_gray(name, load=True):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta = load_case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1 if torch.cuda.is_available() else 0
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    sd = seeded_state_dict(z["sd_keys"], z["sd_shapes"], meta["param_seed"])
    if load:
        missing = model.load_state_dict(sd, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
    return model, sd, z, meta, cfg
