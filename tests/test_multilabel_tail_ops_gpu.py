"""sf_bce and sf_adam_step on the GPU (csrc/step_tail.hip) through slowfast/models/step_tail.py.

Parity is against float64 on the CPU; the bound is the project's rule from test_step_tail_ops_gpu.py: what torch's own
float32 GPU kernels miss the same float64 values by, on the same inputs, times 2.  Every case prints both errors; the
figures measured on an MI355X are in profiles/step_tail_multilabel.txt."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
MARGIN, SENTINEL = 256, -777.0


def _mods():
    from slowfast.models import step_tail
    return step_tail


def _guarded(shape):
    """A NaN-filled buffer of `shape` between two sentinel margins -> (whole allocation, the buffer's view)."""
    n = int(np.prod(shape))
    whole = torch.full((MARGIN + n + MARGIN,), SENTINEL, dtype=torch.float32, device="cuda")
    whole[MARGIN:MARGIN + n] = float("nan")
    return whole, whole[MARGIN:MARGIN + n].view(shape)


def _margins_intact(whole):
    return bool((whole[:MARGIN] == SENTINEL).all()) and bool((whole[-MARGIN:] == SENTINEL).all())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _run_bce(x, y, from_logits, cap=3):
    st = _mods()
    ring = st.StatsRing(cap)
    out = torch.zeros(2, device="cuda")
    d = st.bce(x, y, from_logits, ring, out)
    torch.cuda.synchronize()
    return d, ring, out


def _torch_bce(x, y, from_logits):
    return F.binary_cross_entropy_with_logits(x, y) if from_logits else F.binary_cross_entropy(x, y)


# ------------------------------------------------------------------------------------------------ BCE parity
def _bce_cases():
    cases = []
    for N, K, pad in ((1, 1, 0), (1, 2, 0), (3, 80, 0), (8, 157, 0), (65, 80, 0), (8, 80, 3)):
        for soft in (False, True):
            for from_logits in (False, True):
                cases.append(("%s_n%d_k%d%s_%s" % ("bce_logit" if from_logits else "bce", N, K, "_stride" if pad else "",
                                                   "soft" if soft else "hard"), N, K, pad, soft, None, from_logits))
    cases.append(("bce_p_exactly_0_and_1", 4, 80, 0, False, "ends", False))
    cases.append(("bce_logit_pm80", 8, 80, 0, False, "big", True))
    return cases


@pytest.mark.parametrize("name,N,K,pad,soft,special,from_logits", _bce_cases(), ids=[c[0] for c in _bce_cases()])
def test_bce_matches_float64_within_twice_torchs_own_error(name, N, K, pad, soft, special, from_logits):
    g = torch.Generator().manual_seed(N * 1000 + K + (7 if soft else 0))
    x = torch.randn(N, K + pad, generator=g) * 3.0
    if not from_logits:
        x = torch.sigmoid(x)
    y = torch.rand(N, K + pad, generator=g)
    if not soft:
        y = (y < 0.3).float()
    if special == "ends":  # the -100 clamp of the logs and the 1e-12 clamp of the gradient, against both targets
        x[0, 0:4] = torch.tensor([0.0, 0.0, 1.0, 1.0])
        y[0, 0:4] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    if special == "big":  # exp() of the raw values would overflow float32; log1p(exp(-80)) is far below 1 ulp of 80
        x[2] = torch.where(torch.rand(K, generator=g) < 0.5, torch.tensor(80.0), torch.tensor(-80.0)) + \
            torch.randn(K, generator=g) * 0.01
    x64 = x[:, :K].double().requires_grad_(True)
    ref_loss = _torch_bce(x64, y[:, :K].double(), from_logits)
    ref_loss.backward()
    xg = x.cuda()[:, :K].detach().requires_grad_(True)  # the same strided views on the GPU
    yg = y.cuda()[:, :K]
    t_loss = _torch_bce(xg, yg, from_logits)
    t_loss.backward()
    d, ring, out = _run_bce(x.cuda()[:, :K], yg, from_logits)
    e_loss = abs(float(out[0].double().cpu()) - float(ref_loss.detach()))
    t_e_loss = abs(float(t_loss.detach().double().cpu()) - float(ref_loss.detach()))
    e_grad = float((d.double().cpu() - x64.grad).abs().max())
    t_e_grad = float((xg.grad.double().cpu() - x64.grad).abs().max())
    print("%s: loss err %.3e (torch %.3e)  gradient err %.3e (torch %.3e)" % (name, e_loss, t_e_loss, e_grad, t_e_grad))
    assert e_loss <= 2 * t_e_loss and e_grad <= 2 * t_e_grad
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(out).all())
    row = ring.rows[0].tolist()
    assert row[0] == float(out[0]) and row[3] == 0.0 == float(out[1]) and row[4] == N and row[5] == 0.0
    assert row[1] == 0.0 == row[2] and row[6] == 1.0 and row[7] == 0.0


def test_bce_accepts_float64_and_integer_targets():
    g = torch.Generator().manual_seed(3)
    x = torch.sigmoid(torch.randn(5, 80, generator=g)).cuda()
    y = (torch.rand(5, 80, generator=g) < 0.3)
    base = _run_bce(x, y.float().cuda(), False)
    for t in (y.double().cuda(), y.long().cuda()):
        d, ring, out = _run_bce(x, t, False)
        assert _same_bits(d, base[0]) and _same_bits(out, base[2])


# ------------------------------------------------------------------------------------------------ bad inputs
@pytest.mark.parametrize("from_logits", [False, True], ids=["bce", "bce_logit"])
def test_nan_or_inf_input_sets_the_flag(from_logits):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 80, generator=g)
    if not from_logits:
        x = torch.sigmoid(x)
    y = (torch.rand(4, 80, generator=g) < 0.3).float()
    clean = _run_bce(x.cuda(), y.cuda(), from_logits)
    assert float(clean[1].rows[0, 3]) == 0.0
    keep = torch.ones(4, 80, dtype=torch.bool)
    keep[1, 3] = False
    for where in ("x", "y"):
        for poison in (float("nan"), float("inf")):
            xb, yb = x.clone(), y.clone()
            (xb if where == "x" else yb)[1, 3] = poison
            d, ring, out = _run_bce(xb.cuda(), yb.cuda(), from_logits)
            assert float(ring.rows[0, 3]) == 1.0 and float(out[1]) == 1.0 and float(ring.rows[0, 5]) == 0.0
            assert not bool(torch.isfinite(out[0])) and not bool(torch.isfinite(ring.rows[0, 0]))
            # the other elements' gradients are those of the clean run
            assert _same_bits(d[keep.cuda()], clean[0][keep.cuda()])


def test_targets_and_probabilities_outside_the_unit_interval_are_counted_and_skipped():
    g = torch.Generator().manual_seed(6)
    N, K = 5, 80
    x = torch.sigmoid(torch.randn(N, K, generator=g))
    y = (torch.rand(N, K, generator=g) < 0.3).float()
    xb, yb = x.clone(), y.clone()
    yb[1, 7] = 1.5
    xb[3, 11] = -0.1
    d, ring, out = _run_bce(xb.cuda(), yb.cuda(), False)
    assert float(ring.rows[0, 5]) == 2.0 and float(ring.rows[0, 3]) == 0.0 and float(ring.rows[0, 4]) == N
    assert float(d[1, 7]) == 0.0 and float(d[3, 11]) == 0.0
    good = _run_bce(x.cuda(), y.cuda(), False)
    keep = torch.ones(N, K, dtype=torch.bool)
    keep[1, 7] = keep[3, 11] = False
    assert _same_bits(d[keep.cuda()], good[0][keep.cuda()])  # neighbours intact: the divisor is still N * K
    want = float(F.binary_cross_entropy(x.double()[keep], y.double()[keep], reduction="sum")) / (N * K)
    assert abs(float(out[0]) - want) <= 1e-6 * want
    # with logits torch checks no range: a target of 1.5 is an ordinary value
    d, ring, out = _run_bce(torch.logit(x).cuda(), yb.cuda(), True)
    assert float(ring.rows[0, 5]) == 0.0 and float(ring.rows[0, 3]) == 0.0


# ------------------------------------------------------------------------------------------------ ring, owned memory
def test_ring_rows_wrap_and_counter_counts():
    st = _mods()
    ring = st.StatsRing(3)
    out = torch.zeros(2, device="cuda")
    g = torch.Generator().manual_seed(7)
    losses = []
    for i in range(5):
        x = torch.randn(4, 9, generator=g)
        y = torch.rand(4, 9, generator=g)
        st.bce(x.cuda(), y.cuda(), True, ring, out)
        losses.append(float(out[0]))
    assert int(ring.counter[0]) == 5
    rows = ring.rows.cpu()
    # steps 0..4 landed in rows 0, 1, 2, 0, 1
    assert [float(rows[0, 0]), float(rows[1, 0]), float(rows[2, 0])] == [losses[3], losses[4], losses[2]]
    assert len(set(losses)) == 5


@pytest.mark.parametrize("from_logits", [False, True], ids=["bce", "bce_logit"])
def test_bce_writes_only_what_it_owns_and_repeats_its_bits(from_logits):
    st = _mods()
    g = torch.Generator().manual_seed(8)
    N, K, cap = 7, 83, 3
    x = torch.randn(N, K + 3, generator=g)
    x = (x if from_logits else torch.sigmoid(x)).cuda()[:, :K]
    y = torch.rand(N, K + 5, generator=g).cuda()[:, :K]
    runs = []
    for _ in range(2):
        wd, d = _guarded((N, K))
        wr, rows = _guarded((cap, 8))
        wo, out = _guarded((2,))
        ring = st.StatsRing(cap)
        ring.rows = rows
        cnt_whole = torch.full((64 + 1 + 64,), 12345, dtype=torch.int32, device="cuda")
        cnt_whole[64] = 1  # the next slot is row 1
        ring.counter = cnt_whole[64:65]
        st.bce(x, y, from_logits, ring, out, dgrad=d)
        torch.cuda.synchronize()
        assert _margins_intact(wd) and _margins_intact(wr) and _margins_intact(wo)
        assert bool((cnt_whole[:64] == 12345).all()) and bool((cnt_whole[65:] == 12345).all()) and int(cnt_whole[64]) == 2
        assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(out).all())
        assert bool(torch.isnan(rows[0]).all()) and bool(torch.isnan(rows[2]).all())  # only row 1 was written
        assert bool(torch.isfinite(rows[1]).all())
        runs.append((d.clone(), rows[1].clone(), out.clone()))
    for a, b in zip(*runs):
        assert _same_bits(a, b)


@pytest.mark.parametrize("cls", ["HipBCE", "HipBCEWithLogits"])
def test_autograd_function_and_backward_direct(cls):
    st = _mods()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(6, 80, generator=g)
    x = (torch.sigmoid(x) if cls == "HipBCE" else x).cuda()
    y = (torch.rand(6, 80, generator=g) < 0.3).double().cuda()  # the reference's label dtype
    loss_fun = getattr(st, cls)(st.StatsRing(4))
    a = x.clone().requires_grad_(True)
    loss = loss_fun(a, y)
    loss.backward()
    b = x.clone().requires_grad_(True)
    loss_fun(b, y)
    loss_fun.backward_direct(b)
    assert _same_bits(a.grad, b.grad) and _same_bits(a.grad, loss_fun.dlogits)
    c = x.clone().requires_grad_(True)
    (loss_fun(c, y) * 3.0).backward()
    assert torch.equal(c.grad, loss_fun.dlogits * 3.0)
    assert int(loss_fun.ring.counter[0]) == 3 and float(loss_fun.guard[0]) == 0.0
    with pytest.raises(ValueError, match="empty batch"):
        loss_fun(x[:0], y[:0])


# ------------------------------------------------------------------------------------------------ Adam
def _chunk():
    import sfhip
    return sfhip.lib().sf_sgd_chunk_elems()


def _problem(seed=0):
    """The eight tensors of the SGD test (the chunk path's edge sizes), gradients packed tightly into one flat buffer
    as FlatGradients does: behind the one-element tensor some views are 4-byte- but not 16-byte-aligned."""
    C = _chunk()
    numels = [C, 1, 3, 4, 5, C - 1, C + 1, 2 * C + 1]
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g) for n in numels]
    grads = [[torch.randn(n, generator=g) for n in numels] for _ in range(4)]
    return numels, params, grads


def _bind(params, flat, skip):
    off = 0
    for i, p in enumerate(params):
        p.grad = None if i == skip else flat[off:off + p.numel()]
        off += p.numel()


def _load(flat, grads, dtype):
    flat.copy_(torch.cat(grads).to(dtype))


def _groups(params, wd=(0.0, 5e-2)):
    return [{"params": params[0::2], "weight_decay": wd[0]}, {"params": params[1::2], "weight_decay": wd[1]}]


LRS = (0.1, 0.05, 0.2)
SKIP = 3  # this parameter has grad None throughout
ADAM = dict(lr=0.1, betas=(0.9, 0.999), eps=1e-8)
_REF = {}


def _steps(make_opt, device, dtype, steps=3, **step_kw):
    numels, p0, grads = _problem()
    params = [torch.nn.Parameter(p.to(device=device, dtype=dtype)) for p in p0]
    flat = torch.zeros(sum(numels), device=device, dtype=dtype)
    _bind(params, flat, SKIP)
    opt = make_opt(_groups(params))
    for s in range(steps):
        for gr in opt.param_groups:
            gr["lr"] = LRS[s]
        _load(flat, grads[s], dtype)
        opt.step(**step_kw)
    return params, opt, flat


def _reference(steps):
    """torch.optim.Adam in float64 on the CPU and torch's own float32 foreach run on the GPU: computed once."""
    if steps not in _REF:
        _REF[steps] = (_steps(lambda g: torch.optim.Adam(g, **ADAM), "cpu", torch.float64, steps),
                       _steps(lambda g: torch.optim.Adam(g, foreach=True, **ADAM), "cuda", torch.float32, steps))
    return _REF[steps]


def _err(params, opt, ref_params, ref_opt):
    out = []
    for key in (None, "exp_avg", "exp_avg_sq"):
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


def test_adam_matches_float64_within_twice_torchs_own_error():
    st = _mods()
    (ref_p, ref_o, _), (t_p, t_o, _) = _reference(3)
    h_p, h_o, flat = _steps(lambda g: st.HipAdam(g, **ADAM), "cuda", torch.float32)
    torch.cuda.synchronize()
    # the gradient views really are a mix of 16-byte aligned and merely 4-byte aligned ones
    al = [p.grad.data_ptr() % 16 for i, p in enumerate(h_p) if i != SKIP]
    assert 0 in al and any(a in (4, 8, 12) for a in al)
    e, t = _err(h_p, h_o, ref_p, ref_o), _err(t_p, t_o, ref_p, ref_o)
    print("adam: param err %.3e (torch %.3e)  exp_avg err %.3e (torch %.3e)  exp_avg_sq err %.3e (torch %.3e)" % (
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
        assert s["step"].is_cuda and s["step"].dtype == torch.float32 and s["step"].dim() == 0
        assert float(s["step"]) == 3.0
        assert all(v.data_ptr() % 16 == 0 for v in s.values())
    assert len(h_o._blocks) == 1
    lo, hi = h_o._blocks[0].data_ptr(), h_o._blocks[0].data_ptr() + 4 * h_o._blocks[0].numel()
    assert all(lo <= v.data_ptr() < hi for i, p in enumerate(h_p) if i != SKIP for v in h_o.state[p].values())


def test_adam_zero_grad_and_guard():
    st = _mods()
    base_p, base_o, base_flat = _steps(lambda g: st.HipAdam(g, **ADAM), "cuda", torch.float32)
    z_p, z_o, z_flat = _steps(lambda g: st.HipAdam(g, **ADAM), "cuda", torch.float32, zero_grad=True)
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


def test_checkpoint_round_trip_with_torch_adam():
    st = _mods()
    numels, _, grads = _problem()
    (ref_p, ref_o, _), (t_p, t_o, _) = _reference(3)  # float64 and torch float32 all the way
    h_p, h_o, h_flat = _steps(lambda g: st.HipAdam(g, **ADAM), "cuda", torch.float32, steps=2)
    u_p, u_o, u_flat = _steps(lambda g: torch.optim.Adam(g, foreach=True, **ADAM), "cuda", torch.float32, steps=2)
    torch.cuda.synchronize()
    # HipAdam's state into a fresh torch Adam over the same parameter values, and torch's into a fresh HipAdam
    a_p = [torch.nn.Parameter(p.detach().clone()) for p in h_p]
    a_flat = torch.zeros_like(h_flat)
    _bind(a_p, a_flat, SKIP)
    a_o = torch.optim.Adam(_groups(a_p), foreach=True, **ADAM)
    a_o.load_state_dict(h_o.state_dict())
    b_p = [torch.nn.Parameter(p.detach().clone()) for p in u_p]
    b_flat = torch.zeros_like(u_flat)
    _bind(b_p, b_flat, SKIP)
    b_o = st.HipAdam(_groups(b_p), **ADAM)
    assert not u_o.state[u_p[0]]["step"].is_cuda  # torch's step counts live on the host: adopted all the same
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
    t = _err(t_p, t_o, ref_p, ref_o)
    a = _err(a_p, a_o, ref_p, ref_o)          # two HipAdam steps, then torch
    b = _err(b_p, b_o, ref_p, ref_o)          # two torch steps, then HipAdam
    print("adam round trip (param / exp_avg / exp_avg_sq): torch %.3e %.3e %.3e  hip->torch %.3e %.3e %.3e  "
          "torch->hip %.3e %.3e %.3e" % tuple(t + a + b))
    assert _within(a, t) and _within(b, t)
    assert float(b_o.state[b_p[0]]["step"]) == 3.0 and float(a_o.state[a_p[0]]["step"]) == 3.0


def test_captured_bce_adam_step_follows_the_lr_schedule_and_keeps_counting():
    st = _mods()
    from slowfast.models import engine
    g = torch.Generator().manual_seed(21)
    N, K = 6, 80
    logits0 = torch.randn(N, K, generator=g).cuda()
    targets = (torch.rand(N, K, generator=g) < 0.3).float().cuda()
    w0 = torch.randn(K, generator=g).cuda()
    lrs = (0.3, 0.05, 0.7)

    def make():
        logits = logits0.clone().requires_grad_(True)   # a leaf: its .grad is what the optimizer reads
        bias = torch.nn.Parameter(w0.clone())           # a second parameter, in a group with weight decay
        bias.grad = torch.zeros_like(bias)
        ring = st.StatsRing(8)
        loss_fun = st.HipBCEWithLogits(ring)
        opt = st.HipAdam([{"params": [logits]}, {"params": [bias], "weight_decay": 0.01}], lr=0.1)

        def step():
            loss_fun(logits, targets)
            loss_fun.backward_direct(logits)
            bias.grad.copy_(logits.detach()[1])          # a gradient that changes with every step
            opt.step(guard=loss_fun.guard, zero_grad=True)
        torch.cuda.synchronize()
        return logits, bias, ring, opt, step

    # capture before any eager step: refused
    logits, bias, ring, opt, step = make()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="warm up eagerly"):
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.synchronize()

    def warm(step):
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.synchronize()

    # eager: three warm-up steps, then three steps on the schedule
    logits, bias, ring, opt, step = make()
    warm(step)
    epoch0 = engine._PARAM_EPOCH
    with torch.cuda.stream(side):
        for lr in lrs:
            for gr in opt.param_groups:
                gr["lr"] = lr
            step()
    torch.cuda.synchronize()
    assert engine._PARAM_EPOCH == epoch0 + 3  # the global optimizer-step hook still fires
    eager = (logits.detach().clone(), bias.detach().clone(), ring.rows.clone(), int(ring.counter[0]),
             [opt.state[p]["step"].clone() for p in (logits, bias)])
    assert [float(s) for s in eager[4]] == [6.0, 6.0]

    # replay: the same warm-up, one captured step (one sequential stream), replayed under the same schedule
    logits, bias, ring, opt, step = make()
    warm(step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    with torch.cuda.stream(side):
        for lr in lrs:
            for gr in opt.param_groups:
                gr["lr"] = lr
            assert opt.upload_hyper()
            engine.replay(graph)
    torch.cuda.synchronize()
    assert _same_bits(logits.detach(), eager[0]) and _same_bits(bias.detach(), eager[1])
    assert _same_bits(ring.rows, eager[2]) and int(ring.counter[0]) == eager[3] == 6
    assert [float(opt.state[p]["step"]) for p in (logits, bias)] == [6.0, 6.0]  # the device counts advanced on replay
    assert len(set(ring.rows[:6, 0].tolist())) == 6  # the replayed loss kernel advanced the slot every time
