"""NonLocalBlock and Stripe_NonLocalBlock (slowfast/models/wdf_attention_helper.py) against the reference's own classes:
tests/golden/nl_blocks.npz (make_golden_nlblocks.py) holds, per case, what the reference computed on the CPU in fp32 for
seeded non-zero parameters, a seeded input and a seeded upstream gradient — the train-mode output, dL/dx, every
parameter gradient, the BN's running statistics after the step and the eval-mode output computed with them.

Bound, per tensor, against the float64 restatement of tests/_nlblock_ref.py (held to the fixture by
test_nlblock_args_cpu.py):  err(HIP, fp64) <= max(floor, 4 x err(reference fp32, fp64)), floors 1e-5 (outputs, running
statistics), 1e-4 (dL/dx) and 1e-3 (parameter gradients) — test_ctx_modules_gpu.py's; err is the relative L2 distance
(_nlblock_ref.err: where the float64 gradient of a bias is an analytical zero, relative to its weight's gradient); the
reference-fp32 error is taken from the fixture, for activation-sized tensors at the fixture's stored elements.  Every run appends its values to
models_report.txt through test_models_gpu._report.
Observed on an MI355X over the seven cases, HIP vs fp64 / reference fp32 vs fp64 at most: outputs (train and eval)
3.2e-6 / 4.4e-6, running statistics 4.4e-7 / 2.5e-7, dL/dx 6.7e-5 / 6.4e-5, parameter gradients 1.0e-4 / 8.0e-5 — the
largest of each in st_max_soft_s1_c73, whose BN sees four rows; every other case stays below 5.0e-6.  The attention
term of nl_dot_sub: 1.6e-7 from the 1 / N_q rule, 0.79 from 1 / N_k.

Also: tensor in / tensor out and Act in / Act out (with reserve) give the same bits; 'dot' with sub_sample is far from
the 1 / N_k scaling; the eval-mode tape raises NotImplementedError; a key width no attention kernel takes raises."""
import json
import os

import numpy as np
import pytest
import torch

import _nlblock_ref as R
from test_models_gpu import _report

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["st_mean_soft_s3", "st_meanmax_dot_s2", "st_max_soft_s1_c73", "st_max_dot_s6", "nl_soft", "nl_dot_sub",
         "nl_soft_sub_nobn"]
FLOOR = {"out": 1e-5, "eval_out": 1e-5, "running": 1e-5, "dx": 1e-4, "grad": 1e-3}
_FIX = {}


def _fixture():
    if not _FIX:
        z = np.load(os.path.join(HERE, "golden", "nl_blocks.npz"))
        _FIX["z"] = z
        _FIX["cases"] = {c["name"]: c for c in json.loads(str(z["meta"]))}
    return _FIX["z"], _FIX["cases"]


def _block(case):
    return R.fill_case(R.build_block(case), case).cuda().train()


def _step(m, x, g, tape=None, reserve=(0, 0)):
    """One taped forward + backward of the block alone.  -> (out NCTHW, dL/dx NCTHW, {name: grad}) on the CPU."""
    import sfhip
    from slowfast.models import engine
    xa = sfhip.from_ncthw(x)
    t = tape if tape is not None else engine.Tape()
    t.armed = True
    with torch.no_grad(), engine.taping(t):
        ya = m(xa, reserve=reserve)
    assert isinstance(ya, sfhip.Act)
    out = sfhip.to_ncthw(ya)
    gbuf = t.gbuf
    with torch.no_grad(), engine.taping(None):
        gy = t.grad_of(ya)
        gy.buf[..., gy.coff:gy.coff + gy.C] = g.permute(0, 2, 3, 4, 1)
        t.backward()
        dx = gbuf[xa.buf.data_ptr()].view(xa.buf.shape).permute(0, 4, 1, 2, 3).contiguous()
    torch.cuda.synchronize()
    pg = {k: t.pgrads[p].detach().cpu().reshape(p.shape) for k, p in m.named_parameters() if p in t.pgrads}
    return out.cpu(), dx.cpu(), pg


@pytest.mark.parametrize("name", NAMES)
def test_block_against_the_reference_fixture(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    z, cases = _fixture()
    case = cases[name]
    x, g = R.case_tensors(case)
    assert abs(float(x.double().sum()) - case["input_sum"]) < 1e-6
    m = _block(case)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert list(sd) == case["sd_keys"]
    r = R.module_ref(case, sd, x, g, torch.float64)
    out, dx, pg = _step(m, x.cuda(), g.cuda())
    params = [k for k in sd if R.is_param(k)]
    assert sorted(pg) == sorted(params), "a parameter has no gradient"
    fix = lambda key: torch.from_numpy(z[name + "/" + key])  # noqa: E731
    rows = [("out", "out", R.stored(out), R.stored(r["out"]), fix("out")),
            ("dx", "dx", R.stored(dx), R.stored(r["dx"]), fix("dx"))]
    rows += [("grad", k, pg[k], r["grads"][k], fix("grad/" + k)) for k in params]
    if r["running_mean"] is not None:
        after = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        assert int(after["W.1.num_batches_tracked"]) == int(sd["W.1.num_batches_tracked"]) + 1
        rows += [("running", k, after[k], r[k[4:]], fix("after/" + k)) for k in ("W.1.running_mean", "W.1.running_var")]
    m.eval()
    with torch.no_grad():
        ev = m(x.cuda()).cpu()
    rows.append(("eval_out", "eval_out", R.stored(ev), R.stored(r["eval_out"]), fix("eval_out")))
    bad = []
    for kind, label, got, r64, r32 in rows:
        assert bool(torch.isfinite(got).all()), label
        if kind == "grad":
            e_hip, e_ref = R.grad_err(got, r["grads"], label), R.grad_err(r32, r["grads"], label)
        else:
            e_hip, e_ref = R.rel_l2(got, r64), R.rel_l2(r32, r64)
        line = "%-20s %-18s vs fp64: HIP %.3e, reference fp32 %.3e" % (name, label, e_hip, e_ref)
        _report(line)
        print(line)
        if not e_hip <= max(FLOOR[kind], 4.0 * e_ref):
            bad.append(line)
    assert not bad, bad


@pytest.mark.parametrize("name", ["st_meanmax_dot_s2", "st_max_soft_s1_c73", "nl_dot_sub", "nl_soft_sub_nobn"])
def test_tensor_and_act_forms_agree_and_reserve_is_kept(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sfhip
    _, cases = _fixture()
    case = cases[name]
    x, g = R.case_tensors(case)
    x, g = x.cuda(), g.cuda()
    m = _block(case)
    out, dx, pg = _step(m, x, g)  # (a train forward moves the running statistics, which no train output reads)
    for mode in (m.train, m.eval):
        mode()
        with torch.no_grad():
            y_t = m(x)
            y_a = m(sfhip.from_ncthw(x))
            wide = m(sfhip.from_ncthw(x), reserve=(4, 8))  # room for an in-place concat behind the block
        assert isinstance(y_t, torch.Tensor) and isinstance(y_a, sfhip.Act)
        assert (wide.coff, wide.cs, wide.C) == (4, case["C"] + 12, case["C"])
        assert torch.equal(sfhip.to_ncthw(y_a).cpu(), y_t.cpu()) and torch.equal(sfhip.to_ncthw(wide).cpu(), y_t.cpu())
        if mode == m.train:
            assert torch.equal(y_t.cpu(), out)
    m.train()
    out_w, dx_w, pg_w = _step(m, x, g, reserve=(4, 8))  # the taped step into a reserved slice: the same bits
    assert torch.equal(out_w, out) and torch.equal(dx_w, dx)
    for k in pg:
        assert torch.equal(pg_w[k], pg[k]), k


def test_dot_with_sub_sample_divides_by_the_query_count():
    """N_q = 84 queries against N_k = 18 max-pooled keys: f / f.shape[1] is f / 84.  The output's attention term under
    the 1 / N_k rule of Nonlocal's dot_product would be about 4.7 x as large — the HIP output must be the fixture's,
    and far from that.  The term out - x is compared: it is a fraction of out, so fp32's 6e-8 grows by |out| / |term|
    (below 100 for these parameters, and the chain of four GEMMs adds a few units): 1e-4 is wide for the right rule,
    while the wrong one is off by (84 / 18 - 1) / (84 / 18) = 0.79 of the wrong term's norm, up to the biases."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    z, cases = _fixture()
    case = cases["nl_dot_sub"]
    x, g = R.case_tensors(case)
    m = _block(case)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        out = m.eval()(x.cuda()).cpu()   # eval: the BN does not renormalise the scale away
    # (in train mode the BN behind W renormalises a scale away: the eval forward, with the seeded running statistics)
    stats = [sd["W.1.running_mean"].double(), sd["W.1.running_var"].double()]
    sdd = {k: v.double() for k, v in sd.items()}
    e_right = R.rel_l2(out - x, R.nonlocal_block_ref(sdd, x.double(), case, stats, False) - x.double())
    e_wrong = R.rel_l2(out - x, R.nonlocal_block_ref(sdd, x.double(), case, stats, False, scale_by_keys=True) - x.double())
    print("attention term: vs 1/N_q %.3e, vs 1/N_k %.3e" % (e_right, e_wrong))
    assert e_right < 1e-4 and e_wrong > 0.5, (e_right, e_wrong)


def test_eval_tape_and_unserved_widths_raise():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sfhip
    from slowfast.models import engine
    from slowfast.models.wdf_attention_helper import NonLocalBlock, Stripe_NonLocalBlock
    x = torch.randn(1, 32, 2, 4, 6, device="cuda")
    for m in (NonLocalBlock(32), Stripe_NonLocalBlock(2, 32)):
        m = m.cuda().eval()
        t = engine.EvalTape("x")
        t.armed = True
        with torch.no_grad(), engine.taping(t):
            with pytest.raises(NotImplementedError, match="eval-mode tape"):
                m(sfhip.from_ncthw(x))
    for m in (NonLocalBlock(32, inter_channels=6), Stripe_NonLocalBlock(2, 32, inter_channels=6, instance="dot")):
        with torch.no_grad(), pytest.raises(NotImplementedError, match="key width of 6"):
            m.cuda().eval()(x)
    with torch.no_grad(), pytest.raises(AssertionError, match="does not divide"):
        Stripe_NonLocalBlock(3, 32).cuda().eval()(x)
