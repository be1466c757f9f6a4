"""End-to-end GPU parity of the grayscale models against golden vectors produced by the REFERENCE itself
(tests/golden/make_golden_gray.py): the Fast-only ResNet-18 (MODEL.ARCH fast, one input channel) and
SlowFastDualAttention R18 with DATA.INPUT_CHANNEL_NUM [1, 1].

Measures and bounds are those of tests/test_models_gpu.py: max-norm relative error < 1e-3 at every recorded child
boundary, the pre-activation logits and the output (:47-92); the train step's loss within 1e-3 absolute, every recorded
gradient's sampled relative L2 error < 8e-2 (< 0.3 for a parameter of fewer than 16 elements) and its norm within 5 %
(:206-249 — the floor there is the reference's own fp32-against-fp64 difference on ReLU / max-pool networks; for these
two fixtures that difference is at most 5.3e-2, on the scalar s2_fuse...gamma, and 2.5e-2 on the others:
`make_golden_gray.py check`)."""
import numpy as np
import pytest
import torch

from _gray import GRAY_CASES, build_gray, gray_inputs
from _util import rel_err, sample_activation

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.mark.parametrize("name", GRAY_CASES)
def test_gray_eval_forward_matches_reference_golden(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sfhip
    from slowfast.models import head_helper
    model, sd, z, meta, cfg = build_gray(name)
    model.eval()
    acts, tap = {}, {}

    def hook(child):
        def f(m, i, o):
            if isinstance(o, (list, tuple)):
                acts[child] = [sfhip.to_ncthw(a).cpu().numpy() if isinstance(a, sfhip.Act) else a.cpu().numpy()
                               for a in o]
        return f

    for n, m in model.named_children():
        m.register_forward_hook(hook(n))
    head_helper.LOGITS_TAP = lambda t: tap.__setitem__("logits", t.detach().cpu().numpy())
    try:
        with torch.no_grad():
            out = model([x.cuda() for x in gray_inputs(meta)])
        torch.cuda.synchronize()
    finally:
        head_helper.LOGITS_TAP = None
    checked = 0
    for child in z["children"]:
        child = str(child)
        if child not in acts:
            continue
        for i, a in enumerate(acts[child]):
            tag = "eval/%s/%d" % (child, i)
            assert tuple(a.shape) == tuple(z[tag + "/shape"]), tag
            s, amax, mean = sample_activation(a)
            e = rel_err(s, z[tag])
            print("%-20s %-10s p%d %.3e" % (name, child, i, e))
            assert e < TOL, (tag, e)
            checked += 1
    assert checked >= (5 if meta.get("single") else 16)
    e_log = rel_err(tap["logits"].reshape(meta["batch"], -1), z["eval/logits_full"])
    e_out = rel_err(out.cpu().numpy(), z["eval/out"])
    print("%-20s logits %.3e out %.3e" % (name, e_log, e_out))
    assert e_log < TOL and e_out < TOL


@pytest.mark.parametrize("name", GRAY_CASES)
def test_gray_train_step_matches_reference_golden(name):
    """logits = model(x); loss = CE(logits, labels); loss.backward() (train_net.py:78-96), dropout off."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    model, sd, z, meta, cfg = build_gray(name)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.train()
    logits = model([x.cuda() for x in gray_inputs(meta)])
    labels = torch.from_numpy(z["train/labels"]).cuda()
    loss = torch.nn.functional.cross_entropy(logits, labels)
    loss.backward()
    torch.cuda.synchronize()
    e = rel_err(logits.detach().cpu().numpy(), z["train/logits"])
    print("%-20s train logits %.3e  loss %.6f vs %.6f" % (name, e, loss.item(), float(z["train/loss"][0])))
    assert e < TOL
    assert abs(loss.item() - float(z["train/loss"][0])) < 1e-3
    params = dict(model.named_parameters())
    keys = [k[5:] for k in z.files if k.startswith("grad/") and not k.endswith("/stats")]
    assert len(keys) >= 4 and "s1.pathway0_stem.conv.weight" in keys
    assert meta.get("single") or "s1.pathway1_stem.conv.weight" in keys
    for k in keys:
        g = params[k].grad
        assert g is not None, k
        s, amax, _ = sample_activation(g.cpu().numpy(), 4096)
        ref = z["grad/" + k].astype(np.float64)
        e = float(np.linalg.norm(s.astype(np.float64) - ref) / max(np.linalg.norm(ref), 1e-30))
        norm, rnorm = float(g.norm()), float(z["grad/" + k + "/stats"][1])
        print("%-20s grad %-50s L2rel %.3e  |g| %.4e vs %.4e" % (name, k, e, norm, rnorm))
        assert e < (0.3 if g.numel() < 16 else 8e-2), (k, e)
        if g.numel() >= 16:
            assert abs(norm - rnorm) < 5e-2 * rnorm + 1e-9, (k, norm, rnorm)
    missing = [k for k, p in params.items() if p.grad is None]
    assert not missing, missing[:5]
