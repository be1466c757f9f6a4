"""sf_adamw_step, sf_lars_ratios and sf_lars_sgd_step on the GPU (csrc/step_tail.hip, csrc/lars.hip) through
slowfast/models/step_tail.py, on the eight-tensor problem of the Adam tests (tests/test_multilabel_tail_ops_gpu.py).

Parity is against float64 on the CPU; the bound is the project's rule: what torch's own float32 GPU path (foreach AdamW;
the tests/_lars_ref.py wrapper around foreach SGD) misses the same float64 values by, on the same inputs, times 2.  Every
case prints both errors; the figures measured on an MI355X are in profiles/lars_step.txt.

The ratios are compared with the float64 wrapper's value rounded to float32, equal or the adjacent float32: the kernel
evaluates the same formula in float64 from float64 sums of the same squares in another order (relative difference
~1e-15), so the two float64 values round to the same float32 unless a rounding boundary lies between them.  The
hyper-parameters of those cases are exact in float32 (the kernel reads float32 ones from device memory): both sides get
the same numbers."""
import numpy as np
import pytest
import torch

from _lars_ref import LarsRef

pytestmark = pytest.mark.gpu
MARGIN, SENTINEL = 256, -777.0
LRS = (0.1, 0.05, 0.2)
SKIP = 3  # this parameter has grad None throughout
ADAMW = dict(lr=0.1, betas=(0.9, 0.999), eps=1e-8)
SGD = dict(lr=0.1, momentum=0.9, nesterov=True)
LARS = dict(trust_coefficient=0.02, clip=True, eps=1e-8)
_REF = {}


def _mods():
    from slowfast.models import step_tail
    return step_tail


def _chunk():
    import sfhip
    return sfhip.lib().sf_sgd_chunk_elems()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _guarded(n):
    """A NaN-filled float32 buffer of n elements between two sentinel margins -> (whole allocation, the buffer)."""
    whole = torch.full((MARGIN + n + MARGIN,), SENTINEL, dtype=torch.float32, device="cuda")
    whole[MARGIN:MARGIN + n] = float("nan")
    return whole, whole[MARGIN:MARGIN + n]


def _margins_intact(whole):
    return bool((whole[:MARGIN] == SENTINEL).all()) and bool((whole[-MARGIN:] == SENTINEL).all())


def _problem(seed=0):
    """The eight tensors of the SGD / Adam tests (the chunk path's edge sizes); the gradients are packed tightly into one
    flat buffer: behind the one-element tensor some views are 4-byte- but not 16-byte-aligned."""
    C = _chunk()
    numels = [C, 1, 3, 4, 5, C - 1, C + 1, 2 * C + 1]
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g) for n in numels]
    grads = [[torch.randn(n, generator=g) for n in numels] for _ in range(4)]
    return numels, params, grads


def _bind(params, flat, skip):
    off = 0
    for i, p in enumerate(params):
        p.grad = None if i == skip else flat[off:off + p.numel()].view_as(p)
        off += p.numel()


def _load(flat, grads, dtype):
    flat.copy_(torch.cat(grads).to(dtype))


def _groups(params, wd=(0.0, 5e-2), **extra):
    return [dict({"params": params[0::2], "weight_decay": wd[0]}, **{k: v[0] for k, v in extra.items()}),
            dict({"params": params[1::2], "weight_decay": wd[1]}, **{k: v[1] for k, v in extra.items()})]


def _steps(make_opt, device, dtype, steps=3, wd=(0.0, 5e-2), groups_extra=None, **step_kw):
    numels, p0, grads = _problem()
    params = [torch.nn.Parameter(p.to(device=device, dtype=dtype)) for p in p0]
    flat = torch.zeros(sum(numels), device=device, dtype=dtype)
    _bind(params, flat, SKIP)
    opt = make_opt(_groups(params, wd, **(groups_extra or {})))
    for s in range(steps):
        for gr in opt.param_groups:
            gr["lr"] = LRS[s]
        _load(flat, grads[s], dtype)
        opt.step(**step_kw)
    return params, opt, flat


def _err(params, opt, ref_params, ref_opt, keys):
    out = []
    for key in (None,) + tuple(keys):
        e = 0.0
        for a, b in zip(params, ref_params):
            if key is None:
                e = max(e, float((a.detach().double().cpu() - b.detach()).abs().max()))
            elif key in ref_opt.state.get(b, {}):
                e = max(e, float((opt.state[a][key].double().cpu() - ref_opt.state[b][key]).abs().max()))
        out.append(e)
    return out


def _within(e, t):
    return all(a <= 2 * b for a, b in zip(e, t))


# ------------------------------------------------------------------------------------------------ AdamW
ADAM_KEYS = ("exp_avg", "exp_avg_sq")


def _adamw_reference(steps):
    """torch.optim.AdamW in float64 on the CPU and torch's own float32 foreach run on the GPU: computed once."""
    if ("adamw", steps) not in _REF:
        _REF[("adamw", steps)] = (_steps(lambda g: torch.optim.AdamW(g, **ADAMW), "cpu", torch.float64, steps),
                                  _steps(lambda g: torch.optim.AdamW(g, foreach=True, **ADAMW), "cuda", torch.float32,
                                         steps))
    return _REF[("adamw", steps)]


def test_adamw_matches_float64_within_twice_torchs_own_error():
    st = _mods()
    (ref_p, ref_o, _), (t_p, t_o, _) = _adamw_reference(3)
    h_p, h_o, flat = _steps(lambda g: st.HipAdamW(g, **ADAMW), "cuda", torch.float32)
    torch.cuda.synchronize()
    al = [p.grad.data_ptr() % 16 for i, p in enumerate(h_p) if i != SKIP]
    assert 0 in al and any(a in (4, 8, 12) for a in al)  # 16-byte aligned and merely 4-byte aligned gradient views
    e, t = _err(h_p, h_o, ref_p, ref_o, ADAM_KEYS), _err(t_p, t_o, ref_p, ref_o, ADAM_KEYS)
    print("adamw: param err %.3e (torch %.3e)  exp_avg err %.3e (torch %.3e)  exp_avg_sq err %.3e (torch %.3e)" % (
        e[0], t[0], e[1], t[1], e[2], t[2]))
    assert _within(e, t)
    _, p0, _ = _problem()
    assert torch.equal(h_p[SKIP].detach().cpu(), p0[SKIP])  # grad None: untouched, no state
    assert len(h_o.state.get(h_p[SKIP], {})) == 0
    for i, p in enumerate(h_p):
        if i == SKIP:
            continue
        s = h_o.state[p]
        assert set(s) == {"step", "exp_avg", "exp_avg_sq"} == set(ref_o.state[ref_p[i]])
        assert s["step"].is_cuda and s["step"].dtype == torch.float32 and float(s["step"]) == 3.0
        assert all(v.data_ptr() % 16 == 0 for v in s.values())
    # the decay really is decoupled: Adam with the same weight decay ends somewhere else
    a_p, _, _ = _steps(lambda g: st.HipAdam(g, **ADAMW), "cuda", torch.float32)
    assert not _same_bits(a_p[1].detach(), h_p[1].detach())


def test_adamw_without_weight_decay_equals_adam_bit_for_bit():
    st = _mods()
    w_p, w_o, _ = _steps(lambda g: st.HipAdamW(g, **ADAMW), "cuda", torch.float32, wd=(0.0, 0.0))
    a_p, a_o, _ = _steps(lambda g: st.HipAdam(g, **ADAMW), "cuda", torch.float32, wd=(0.0, 0.0))
    torch.cuda.synchronize()
    moved = 0
    _, p0, _ = _problem()
    for i, (a, b) in enumerate(zip(w_p, a_p)):
        assert _same_bits(a.detach(), b.detach())
        moved += int(not torch.equal(a.detach().cpu(), p0[i]))
        if i != SKIP:
            for k in ("exp_avg", "exp_avg_sq", "step"):
                assert _same_bits(w_o.state[a][k], a_o.state[b][k])
    assert moved == len(w_p) - 1


def test_adamw_zero_grad_and_guard():
    st = _mods()
    base_p, base_o, base_flat = _steps(lambda g: st.HipAdamW(g, **ADAMW), "cuda", torch.float32)
    z_p, z_o, z_flat = _steps(lambda g: st.HipAdamW(g, **ADAMW), "cuda", torch.float32, zero_grad=True)
    torch.cuda.synchronize()
    for a, b in zip(base_p, z_p):
        assert _same_bits(a.detach(), b.detach())
    off = 0
    for i, p in enumerate(z_p):
        seg = z_flat[off:off + p.numel()]
        if i == SKIP:  # not in the table: its span of the buffer is nobody's to zero
            assert bool((seg != 0).any())
        else:
            assert bool((seg.view(torch.int32) == 0).all())  # +0.0 exactly
        off += p.numel()
    assert bool((base_flat != 0).all())
    # a guard that reads non-zero: nothing moves — parameters, both moments, the step counts, the gradients
    live = [p for i, p in enumerate(base_p) if i != SKIP]
    before = [p.detach().clone() for p in base_p]
    state = [base_o.state[p][k].clone() for p in live for k in ("exp_avg", "exp_avg_sq", "step")]
    gflat = base_flat.clone()
    for bad in (1.0, float("nan")):
        base_o.step(guard=torch.tensor([bad], device="cuda"), zero_grad=True)
    torch.cuda.synchronize()
    for a, b in zip(base_p, before):
        assert _same_bits(a.detach(), b)
    for a, b in zip([base_o.state[p][k] for p in live for k in ("exp_avg", "exp_avg_sq", "step")], state):
        assert _same_bits(a, b)
    assert all(float(base_o.state[p]["step"]) == 3.0 for p in live)
    assert _same_bits(base_flat, gflat)
    base_o.step(guard=torch.tensor([0.0], device="cuda"))
    assert not _same_bits(base_p[0].detach(), before[0]) and float(base_o.state[live[0]]["step"]) == 4.0


def test_checkpoint_round_trip_with_torch_adamw():
    st = _mods()
    numels, _, grads = _problem()
    (ref_p, ref_o, _), (t_p, t_o, _) = _adamw_reference(3)
    h_p, h_o, h_flat = _steps(lambda g: st.HipAdamW(g, **ADAMW), "cuda", torch.float32, steps=2)
    u_p, u_o, u_flat = _steps(lambda g: torch.optim.AdamW(g, foreach=True, **ADAMW), "cuda", torch.float32, steps=2)
    torch.cuda.synchronize()
    a_p = [torch.nn.Parameter(p.detach().clone()) for p in h_p]
    a_flat = torch.zeros_like(h_flat)
    _bind(a_p, a_flat, SKIP)
    a_o = torch.optim.AdamW(_groups(a_p), foreach=True, **ADAMW)
    a_o.load_state_dict(h_o.state_dict())
    b_p = [torch.nn.Parameter(p.detach().clone()) for p in u_p]
    b_flat = torch.zeros_like(u_flat)
    _bind(b_p, b_flat, SKIP)
    b_o = st.HipAdamW(_groups(b_p), **ADAMW)
    b_o.load_state_dict(u_o.state_dict())
    for i, p in enumerate(b_p):  # loaded state lives in the optimizer's own allocation
        if i != SKIP:
            for k, v in b_o.state[p].items():
                assert v.data_ptr() == b_o._slots[p][k].data_ptr() and v.data_ptr() % 16 == 0
            assert float(b_o.state[p]["step"]) == 2.0
    for opt, flat in ((a_o, a_flat), (b_o, b_flat)):
        for gr in opt.param_groups:
            gr["lr"] = LRS[2]
        _load(flat, grads[2], torch.float32)
        opt.step()
    torch.cuda.synchronize()
    t = _err(t_p, t_o, ref_p, ref_o, ADAM_KEYS)
    a = _err(a_p, a_o, ref_p, ref_o, ADAM_KEYS)          # two HipAdamW steps, then torch
    b = _err(b_p, b_o, ref_p, ref_o, ADAM_KEYS)          # two torch steps, then HipAdamW
    print("adamw round trip (param / exp_avg / exp_avg_sq): torch %.3e %.3e %.3e  hip->torch %.3e %.3e %.3e  "
          "torch->hip %.3e %.3e %.3e" % tuple(t + a + b))
    assert _within(a, t) and _within(b, t)
    assert float(b_o.state[b_p[0]]["step"]) == 3.0 and float(a_o.state[a_p[0]]["step"]) == 3.0


# ------------------------------------------------------------------------------------------------ ratios
def _ratio_problem(device, dtype, zero_grad_at=6, zero_param_at=5):
    """The eight tensors with a mix of shapes (some [1, n]: not one-dimensional), one all-zero gradient and one all-zero
    parameter; the gradients packed tight as above, no parameter skipped."""
    numels, p0, grads = _problem(seed=1)
    two_d = (0, 3, 5, 6, 7)
    params = []
    for i, p in enumerate(p0):
        v = torch.zeros_like(p) if i == zero_param_at else p
        params.append(torch.nn.Parameter(v.to(device=device, dtype=dtype).view((1, -1) if i in two_d else (-1,))))
    flat = torch.zeros(sum(numels), device=device, dtype=dtype)
    _bind(params, flat, None)
    g = [torch.zeros_like(x) if i == zero_grad_at else x for i, x in enumerate(grads[0])]
    _load(flat, g, dtype)
    return params


def _adjacent(a, b):
    """float32 tensors: equal, or neighbours in float32."""
    return bool(((a.view(torch.int32).long() - b.view(torch.int32).long()).abs() <= 1).all())


# every number is exact in float32: lr = trust = 2^-6 puts r / lr on both sides of 1 when clipping
@pytest.mark.parametrize("clip,apply0,ignore_1d", [(True, True, False), (False, True, False), (False, False, True)],
                         ids=["clip", "noclip", "noclip_group0_off_ignore_1d"])
def test_ratios_match_the_float64_wrapper(clip, apply0, ignore_1d):
    st = _mods()
    lr, wd, kw = 2.0 ** -6, (0.0, 2.0 ** -4), dict(trust_coefficient=2.0 ** -6, clip=clip, eps=2.0 ** -27,
                                                  ignore_1d_param=ignore_1d)
    extra = {"apply_LARS": (apply0, True)}
    r_p = _ratio_problem("cpu", torch.float64)
    ref = LarsRef(torch.optim.SGD(_groups(r_p, wd, **extra), lr=lr), **kw)
    want = torch.tensor(ref.ratios(), dtype=torch.float64)
    h_p = _ratio_problem("cuda", torch.float32)
    opt = st.HipLARS(_groups(h_p, wd, **extra), lr=lr, **kw)
    opt.step()
    torch.cuda.synchronize()
    got = opt.ratios.cpu()
    w32 = want.float()
    order = [0, 2, 4, 6, 1, 3, 5, 7]  # table order: group by group
    for row, i in enumerate(order):
        print("tensor %d (%s): r %.9g (float64 %.17g)  wd_t %.9g" % (i, tuple(h_p[i].shape), float(got[row, 0]),
                                                                   float(want[row, 0]), float(got[row, 1])))
    assert tuple(got.shape) == (8, 2) and _adjacent(got, w32)
    assert torch.equal(got[:, 1], w32[:, 1])  # wd_t is one of two exact values
    row = {i: r for r, i in enumerate(order)}
    assert got[row[6]].tolist() == [1.0, 0.0] and got[row[5]].tolist() == [1.0, 0.0]  # zero gradient; zero parameter
    if clip:
        # the two zero-norm tensors read 1; the three-chunk tensor (pn ~ gn, wd = 1 / 16) stays below it
        assert bool((got[:, 0] <= 1.0).all()) and int((got[:, 0] == 1.0).sum()) >= 2 and float(got[row[7], 0]) < 1.0
    if not apply0:
        assert all(got[row[i]].tolist() == [1.0, wd[0]] for i in (0, 2, 4))
        assert int(((got[:, 0] != 1.0)).sum()) >= 1  # group 1 still applies LARS
    if ignore_1d:
        assert got[row[1]].tolist() == [1.0, wd[1]] and got[row[3], 0] != 1.0  # [1] is 1-D, [1, 4] is not
    assert float(opt.guard) == 0.0 and float(opt.nonfinite) == 0.0


def _raw_ratios(p, g, lr=0.125, wd=0.0625, guard=None):
    """One tensor through the raw entry: (ratios [1, 2], partials, state)."""
    st = _mods()
    table, chunks = st.build_lars_tables([(p.data_ptr(), g.data_ptr(), p.numel(), 0, 0)], _chunk())
    hyper = torch.tensor([[lr, wd, 1.0], [2.0 ** -6, 2.0 ** -27, 0.0]], dtype=torch.float32)
    partials = torch.zeros(2 * chunks.shape[0], dtype=torch.float64, device="cuda")
    ratios = torch.zeros((1, 2), dtype=torch.float32, device="cuda")
    state = torch.zeros(8, dtype=torch.float32, device="cuda")
    st.lars_ratios(table, table.cuda(), chunks, chunks.cuda(), hyper, hyper.cuda(), partials, ratios, state, guard=guard)
    torch.cuda.synchronize()
    return ratios, partials, state


def test_ratios_repeat_their_bits_whatever_the_alignment():
    n = 2 * _chunk() + 7
    gen = torch.Generator().manual_seed(5)
    pv, gv = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    bufs = [torch.zeros(n + 8, device="cuda") for _ in range(2)]
    runs = []
    for po, go in ((0, 0), (0, 0), (0, 1), (3, 0), (1, 2)):  # offsets in floats: 16-byte aligned or merely 4
        p, g = bufs[0][po:po + n], bufs[1][go:go + n]
        p.copy_(pv)
        g.copy_(gv)
        assert p.data_ptr() % 16 == 4 * po and g.data_ptr() % 16 == 4 * go
        runs.append(_raw_ratios(p, g))
    for r in runs[1:]:
        assert _same_bits(r[0], runs[0][0]) and torch.equal(r[1].view(torch.int64), runs[0][1].view(torch.int64))
    want = float(np.sqrt(np.sum(pv.double().numpy() ** 2)))
    assert abs(float(runs[0][1][0::2].sum().sqrt()) - want) <= 1e-13 * want and float(runs[0][0][0, 0]) != 1.0


# ------------------------------------------------------------------------------------------------ HipLARS
SGD_KEYS = ("momentum_buffer",)


def _lars_reference():
    if "lars" not in _REF:
        _REF["lars"] = (
            _steps(lambda g: LarsRef(torch.optim.SGD(g, **SGD), **LARS), "cpu", torch.float64),
            _steps(lambda g: LarsRef(torch.optim.SGD(g, foreach=True, **SGD), **LARS), "cuda", torch.float32))
    return _REF["lars"]


def test_lars_three_steps_match_float64_within_twice_the_wrappers_own_error():
    st = _mods()
    (ref_p, ref_o, _), (t_p, t_o, _) = _lars_reference()
    h_p, h_o, _ = _steps(lambda g: st.HipLARS(g, **SGD, **LARS), "cuda", torch.float32)
    torch.cuda.synchronize()
    e, t = _err(h_p, h_o, ref_p, ref_o, SGD_KEYS), _err(t_p, t_o, ref_p, ref_o, SGD_KEYS)
    print("lars: param err %.3e (wrapper %.3e)  momentum_buffer err %.3e (wrapper %.3e)" % (e[0], t[0], e[1], t[1]))
    assert _within(e, t)
    _, p0, _ = _problem()
    assert torch.equal(h_p[SKIP].detach().cpu(), p0[SKIP]) and len(h_o.state.get(h_p[SKIP], {})) == 0
    assert tuple(h_o.ratios.shape) == (7, 2) and bool((h_o.ratios[:, 0] < 1.0).any())  # LARS did scale something
    # partials, ratios and state are views of ONE allocation of the optimizer's
    blk = h_o._lars_block
    lo, hi = blk.data_ptr(), blk.data_ptr() + 4 * blk.numel()
    assert all(lo <= v.data_ptr() < hi for v in (h_o._partials, h_o.ratios, h_o.guard)) and len(h_o._blocks) == 2
    # the state dict is torch.optim.SGD's
    sd = h_o.state_dict()
    assert set(sd) == {"state", "param_groups"} and all(set(s) == {"momentum_buffer"} for s in sd["state"].values())


def test_lars_with_no_group_applying_equals_hipsgd_bit_for_bit():
    st = _mods()
    off = {"apply_LARS": (False, False)}
    l_p, l_o, _ = _steps(lambda g: st.HipLARS(g, **SGD, **LARS), "cuda", torch.float32, groups_extra=off)
    s_p, s_o, _ = _steps(lambda g: st.HipSGD(g, **SGD), "cuda", torch.float32)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(l_p, s_p)):
        assert _same_bits(a.detach(), b.detach())
        if i != SKIP:
            assert _same_bits(l_o.state[a]["momentum_buffer"], s_o.state[b]["momentum_buffer"])
    assert bool((l_o.ratios[:, 0] == 1.0).all())
    a_p, _, _ = _steps(lambda g: st.HipLARS(g, **SGD, **LARS), "cuda", torch.float32)
    assert not _same_bits(a_p[0].detach(), s_p[0].detach())  # and with LARS applied the step differs


def test_nonfinite_gradient_or_a_raised_guard_moves_nothing():
    st = _mods()
    numels, _, grads = _problem()
    h_p, h_o, flat = _steps(lambda g: st.HipLARS(g, **SGD, **LARS), "cuda", torch.float32, steps=2)
    torch.cuda.synchronize()
    assert float(h_o.guard) == 0.0
    live = [p for i, p in enumerate(h_p) if i != SKIP]

    def snapshot():
        return [p.detach().clone() for p in h_p] + [h_o.state[p]["momentum_buffer"].clone() for p in live]

    def now():
        return [p.detach() for p in h_p] + [h_o.state[p]["momentum_buffer"] for p in live]
    before = snapshot()
    # one NaN in one gradient (the last element of the three-chunk tensor): the ratios' guard rises
    _load(flat, grads[2], torch.float32)
    flat[-1] = float("nan")
    gflat = flat.clone()
    h_o.step(zero_grad=True)
    torch.cuda.synchronize()
    assert float(h_o.guard) == 1.0 and float(h_o.nonfinite) == 1.0
    assert all(_same_bits(a, b) for a, b in zip(now(), before)) and _same_bits(flat, gflat)
    # clean gradients, a guard raised by the loss (1, or NaN itself)
    _load(flat, grads[2], torch.float32)
    gflat = flat.clone()
    for bad in (1.0, float("nan")):
        h_o.step(guard=torch.tensor([bad], device="cuda"), zero_grad=True)
        torch.cuda.synchronize()
        assert float(h_o.guard) == 1.0 and float(h_o.nonfinite) == 0.0
    assert all(_same_bits(a, b) for a, b in zip(now(), before)) and _same_bits(flat, gflat)
    # and a guard that reads zero lets the step through
    h_o.step(guard=torch.tensor([0.0], device="cuda"), zero_grad=True)
    torch.cuda.synchronize()
    assert float(h_o.guard) == 0.0 and not _same_bits(h_p[0].detach(), before[0])
    assert bool((flat[:numels[0]].view(torch.int32) == 0).all())


def test_lars_writes_only_what_it_owns():
    st = _mods()
    C = _chunk()
    numels = [C + 1, 3, 2 * C]
    gen = torch.Generator().manual_seed(9)
    wholes, ps, gs, bs = [], [], [], []
    for n in numels:
        for dst in (ps, gs, bs):
            w, v = _guarded(n)
            v.copy_(torch.randn(n, generator=gen))
            wholes.append(w)
            dst.append(v)
    lars = [(p.data_ptr(), g.data_ptr(), n, i % 2, 0) for i, (p, g, n) in enumerate(zip(ps, gs, numels))]
    sgd = [(p.data_ptr(), g.data_ptr(), b.data_ptr(), n, i % 2, 0) for i, (p, g, b, n) in enumerate(zip(ps, gs, bs, numels))]
    ltab, chunks = st.build_lars_tables(lars, C)
    stab, chunks2 = st.build_sgd_tables(sgd, C)
    assert torch.equal(chunks, chunks2) and chunks.shape[0] == 5
    lhyp = torch.tensor([[0.125, 0.0625, 1.0], [0.125, 0.0, 1.0], [2.0 ** -6, 2.0 ** -27, 1.0]], dtype=torch.float32)
    shyp = torch.tensor([[0.125, 0.0625, 0.5, 0.0, 0.0], [0.125, 0.0, 0.5, 0.0, 0.0]], dtype=torch.float32)
    w_part, part = _guarded(4 * chunks.shape[0])
    w_rat, rat = _guarded(2 * len(numels))
    w_st, state = _guarded(8)
    wholes += [w_part, w_rat, w_st]
    p_before = [p.clone() for p in ps]
    chunks_dev = chunks.cuda()
    st.lars_ratios(ltab, ltab.cuda(), chunks, chunks_dev, lhyp, lhyp.cuda(), part.view(torch.float64), rat, state)
    st.lars_sgd_step(stab, stab.cuda(), chunks, chunks_dev, shyp, shyp.cuda(), rat, guard=state[5:6], zero_grad=True)
    torch.cuda.synchronize()
    assert all(_margins_intact(w) for w in wholes)
    assert bool(torch.isfinite(part.view(torch.float64)).all()) and bool(torch.isfinite(rat).all())
    assert state[4:6].tolist() == [0.0, 0.0] and bool(torch.isnan(state[:4]).all()) and bool(torch.isnan(state[6:]).all())
    for p, g, b, q in zip(ps, gs, bs, p_before):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p, q) and bool(torch.isfinite(b).all())
        assert bool((g.view(torch.int32) == 0).all())
