"""The oracle (oracle/slowfast_oracle.py) against the reference's golden vectors at the driver-monitoring YAMLs' spatial
strides (tests/golden/make_golden_tired.py): res5 is crop/16 wide under a crop//32 head window, so the head is fully
convolutional and the training logits are [N, 3*3*classes].  Bound: the 1e-4 of tests/test_oracle_golden.py.

Only the dual-pathway fixture: the oracle takes its strides from the fixture's hyper-parameters and reproduces it as
it stands, but it has no MODEL.ARCH fast (the Fast-only fixture is held to the reference by the GPU tests alone, as
fast_r18_gray_s64 is)."""
import pytest
import torch

from _gray import gray_inputs
from _util import load_case, rel_err, sample_activation, seeded_state_dict
from oracle import slowfast_oracle as oracle

TOL = 1e-4
ORACLE_CASES = ["dual_r18_gray_tired_s64"]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_tired_forward_matches_reference(name):
    z, meta = load_case(name)
    assert meta["hparams"]["spatial_strides"] == [1, 1, 2, 2]
    sd = seeded_state_dict(z["sd_keys"], z["sd_shapes"], meta["param_seed"])
    acts = oracle.forward(meta["model"], sd, gray_inputs(meta), meta["hparams"], training=False)
    checked = 0
    for child in z["children"]:
        child = str(child)
        if child not in acts:
            continue
        for i, a in enumerate(acts[child]):
            tag = "eval/%s/%d" % (child, i)
            if tag + "/shape" not in z.files:
                tag = "eval/%s" % child
            assert tuple(a.shape) == tuple(z[tag + "/shape"]), tag
            s, amax, mean = sample_activation(a.numpy())
            assert rel_err(s, z[tag]) < TOL, tag
            checked += 1
    assert checked >= (5 if meta.get("single") else 16)
    assert tuple(z["eval/logits_full"].shape) == (meta["batch"], 27)
    assert rel_err(acts["logits"].reshape(meta["batch"], -1).numpy(), z["eval/logits_full"]) < TOL
    assert rel_err(acts["out"].numpy(), z["eval/out"]) < TOL


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_tired_train_mode_logits(name):
    z, meta = load_case(name)
    sd = seeded_state_dict(z["sd_keys"], z["sd_shapes"], meta["param_seed"])
    acts = oracle.forward(meta["model"], sd, gray_inputs(meta), meta["hparams"], training=True)
    assert tuple(acts["out"].shape) == (meta["batch"], 27)
    assert rel_err(acts["out"].numpy(), z["train/logits"]) < TOL
    loss = torch.nn.functional.cross_entropy(acts["out"], torch.from_numpy(z["train/labels"]))
    assert abs(loss.item() - float(z["train/loss"][0])) < TOL
