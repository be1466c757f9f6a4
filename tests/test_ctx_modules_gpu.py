"""ChannelAttention and ContextBlock3D (slowfast/models/wdf_attention_helper.py) against the reference's own classes:
tests/golden/ctx_blocks.npz (make_golden_ctx.py) holds, per case, the train-mode output, dL/dx and every parameter
gradient the reference computed on the CPU for seeded non-zero parameters, a seeded input and a seeded upstream gradient.

Bound, per tensor as relative L2 against the float64 restatement of tests/_ctx_ref.py (which is first held to the
fixture):  err(HIP, fp64) <= max(1e-3, 4 x err(fp32 PyTorch restatement, fp64)) — the rule of
test_gradcam_efficient_models_gpu.py.  conv_mask.bias has the gradient 0 (the softmax is shift invariant): the HIP path
must give exactly 0 there.  Every run appends its values to models_report.txt through test_models_gpu._report.
Observed on an MI355X over the five cases (output, dL/dx and every parameter gradient): HIP vs fp64 at most 4.9e-7, the
fp32 PyTorch restatement vs fp64 at most 5.4e-7; conv_mask.bias exactly 0.

Also: tensor in / tensor out and Act in / Act out give the same bits; the eval forward equals the train forward (no BN
in these blocks); a step under the gradient sink equals the step without it; the eval-mode tape yields the training
tape's dL/dx and no parameter gradient; and a block inserted behind s2 of the dual_r18_gray_s64 model trains with finite
gradients and leaves the model's own step bit-identical once it is removed."""
import json
import os

import numpy as np
import pytest
import torch

import _ctx_ref
from test_models_gpu import _report

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["ca_c8_r16", "ca_c64_r16", "gc_att_c32_r1", "gc_att_c32_r025", "gc_avg_c30_r05"]
_FIX = {}


def _fixture():
    if not _FIX:
        z = np.load(os.path.join(HERE, "golden", "ctx_blocks.npz"))
        _FIX["z"] = z
        _FIX["cases"] = {c["name"]: c for c in json.loads(str(z["meta"]))}
    return _FIX["z"], _FIX["cases"]


def _block(case):
    m = _ctx_ref.seeded_fill(_ctx_ref.build_block(case), case["param_seed"])
    return m.cuda().train()


def _step(m, x, g, sink=False, as_act=True, eval_tape=False):
    """One taped forward + backward of the block alone.  -> (out NCTHW, dL/dx NCTHW, {name: grad}) on the CPU."""
    import sfhip
    from slowfast.models import engine
    xa = sfhip.from_ncthw(x)
    t = engine.EvalTape("x") if eval_tape else engine.Tape()
    t.armed = True
    if sink:
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
        t.sink = {p: p.grad for p in m.parameters()}
    with torch.no_grad(), engine.taping(t):
        y = m(xa) if as_act else m(x)
    ya = y if as_act else None
    assert isinstance(y, sfhip.Act) == as_act
    out = sfhip.to_ncthw(y) if as_act else y
    if not as_act:
        return out.cpu(), None, None
    gbuf = t.gbuf
    with torch.no_grad(), engine.taping(None):
        gy = t.grad_of(ya)
        gy.buf.copy_(g.permute(0, 2, 3, 4, 1).reshape(gy.buf.shape))
        if eval_tape:
            t.target_acts, t.out = [xa], out
            dx = sfhip.to_ncthw(t.backward(torch.zeros(1, device="cuda"))[0])
        else:
            t.backward()
            dx = gbuf[xa.buf.data_ptr()].view(xa.buf.shape).permute(0, 4, 1, 2, 3).contiguous()
    torch.cuda.synchronize()
    if sink:
        pg = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
        for p in m.parameters():
            p.grad = None
    else:
        pg = {k: t.pgrads[p].detach().cpu().reshape(p.shape) for k, p in m.named_parameters() if p in t.pgrads}
    return out.cpu(), dx.cpu(), pg


@pytest.mark.parametrize("name", NAMES)
def test_block_against_the_reference_fixture(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    z, cases = _fixture()
    case = cases[name]
    x, g = _ctx_ref.case_tensors(case)
    assert abs(float(x.double().sum()) - case["input_sum"]) < 1e-6
    m = _block(case)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert list(sd) == case["sd_keys"]
    pool = case.get("pooling_type")
    o64, dx64, pg64 = _ctx_ref.module_ref(case["kind"], pool, sd, x, g, torch.float64)
    o32, dx32, pg32 = _ctx_ref.module_ref(case["kind"], pool, sd, x, g, torch.float32)
    # the restatement is the reference: its float64 form against the fixture the reference's own classes wrote (fp32)
    assert _ctx_ref.rel_l2(torch.from_numpy(z[name + "/out"]), o64) < 1e-5
    assert _ctx_ref.rel_l2(torch.from_numpy(z[name + "/dx"]), dx64) < 1e-4
    for k in sd:
        ref = torch.from_numpy(z[name + "/grad/" + k])
        if float(pg64[k].norm()) > 1e-9:
            assert _ctx_ref.rel_l2(ref, pg64[k]) < 1e-3, k
    out, dx, pg = _step(m, x.cuda(), g.cuda())
    assert sorted(pg) == sorted(sd), "a parameter has no gradient"
    rows = [("out", out, o64, o32), ("dx", dx, dx64, dx32)] + [(k, pg[k], pg64[k], pg32[k]) for k in sd]
    for label, got, r64, r32 in rows:
        assert bool(torch.isfinite(got).all()), label
        if label == "conv_mask.bias":
            _report("%-18s %-28s HIP %s (exact 0 expected)" % (name, label, got.reshape(-1).tolist()))
            assert not bool(got.any()) and float(r64.abs().max()) < 1e-12
            continue
        e_hip, e_ref = _ctx_ref.rel_l2(got, r64), _ctx_ref.rel_l2(r32, r64)
        _report("%-18s %-28s vs fp64: HIP %.3e, torch fp32 %.3e" % (name, label, e_hip, e_ref))
        print("%s %s: HIP %.3e torch-fp32 %.3e" % (name, label, e_hip, e_ref))
        assert e_hip <= max(1e-3, 4.0 * e_ref), (name, label, e_hip, e_ref)


@pytest.mark.parametrize("name", ["ca_c8_r16", "gc_att_c32_r025", "gc_avg_c30_r05"])
def test_kinds_modes_sink_and_eval_tape_agree(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sfhip
    _, cases = _fixture()
    case = cases[name]
    x, g = _ctx_ref.case_tensors(case)
    x, g = x.cuda(), g.cuda()
    m = _block(case)
    out, dx, pg = _step(m, x, g)
    # tensor in / tensor out == Act in / Act out, train and eval, taped or not
    for mode in (m.train, m.eval):
        mode()
        with torch.no_grad():
            y_t = m(x)
            y_a = m(sfhip.from_ncthw(x))
        assert isinstance(y_t, torch.Tensor) and isinstance(y_a, sfhip.Act)
        assert torch.equal(y_t.cpu(), out) and torch.equal(sfhip.to_ncthw(y_a).cpu(), out)
    m.train()
    assert torch.equal(_step(m, x, g, as_act=False)[0], out)
    wide = m(sfhip.from_ncthw(x), reserve=(4, 8))  # room for an in-place concat behind the block
    assert (wide.coff, wide.cs, wide.C) == (4, case["C"] + 12, case["C"])
    assert torch.equal(sfhip.to_ncthw(wide).cpu(), out)
    # the gradient sink: the same bits in .grad as the tape hands to autograd
    out_s, dx_s, pg_s = _step(m, x, g, sink=True)
    assert torch.equal(out_s, out) and torch.equal(dx_s, dx)
    for k in pg:
        assert torch.equal(pg_s[k], pg[k]), k
    # the eval-mode tape: activation gradients only
    m.eval()
    out_e, dx_e, pg_e = _step(m, x, g, eval_tape=True)
    # (the eval tape masks the bare conv + ReLU through sf_epilogue_bwd, the training tape through sf_act_bwd: the same
    # products, so fp32 rounding of the following GEMMs is all that may differ)
    assert torch.equal(out_e, out) and _ctx_ref.rel_l2(dx_e, dx) < 1e-6 and pg_e == {}
    assert all(p.grad is None for p in m.parameters())


class _Behind(torch.nn.Module):
    """A stage with `block` applied to pathway 0 of its outputs (the test's insertion: the model is not changed)."""

    def __init__(self, stage, block):
        super(_Behind, self).__init__()
        self.stage, self.block = stage, block

    def forward(self, x, reserve=None):
        room = reserve[0] if reserve else (0, 0)
        ys = list(self.stage(x, reserve=[(0, 0)] + list(reserve[1:]) if reserve else None))
        ys[0] = self.block(ys[0], reserve=room)
        return ys


@pytest.mark.parametrize("kind", ["ContextBlock3D", "ChannelAttention"])
def test_block_behind_s2_of_the_dual_model(kind):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from _gray import build_gray, gray_inputs
    from slowfast.models.wdf_attention_helper import ChannelAttention, ContextBlock3D
    model, sd, z, meta, cfg = build_gray("dual_r18_gray_s64")
    model = model.cuda().train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    xs = [t.cuda() for t in gray_inputs(meta)]
    labels = torch.from_numpy(z["train/labels"]).cuda()

    def step():
        for p in model.parameters():
            p.grad = None
        loss = torch.nn.functional.cross_entropy(model(xs), labels)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    loss0, g0 = step()
    stage = model.s2
    c = model.s2_fuse.downsample_c_of_slow.in_channels  # the Slow pathway's width behind s2
    block = ContextBlock3D(c, ratio=0.25) if kind == "ContextBlock3D" else ChannelAttention(c)
    _ctx_ref.seeded_fill(block, 77)
    model.s2 = _Behind(stage, block.cuda().train())
    loss1, g1 = step()
    assert np.isfinite(loss1) and loss1 != loss0, "the block changed nothing"
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())
    mine = [k for k in g1 if k.startswith("s2.block.")]
    assert len(mine) == len(list(block.parameters()))
    assert all(float(g1[k].abs().max()) > 0 for k in mine if not k.endswith("conv_mask.bias")), "a dead gradient"
    model.s2 = stage
    loss2, g2 = step()
    assert loss2 == loss0 and sorted(g2) == sorted(g0)
    for k in g0:
        assert torch.equal(g2[k], g0[k]), k
