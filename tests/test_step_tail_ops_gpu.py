"""sf_ce_topk and sf_sgd_step on the GPU (csrc/step_tail.hip) through slowfast/models/step_tail.py.

Parity is against float64 on the CPU; the bound is what torch's own float32 GPU kernels miss the same float64 values
by, on the same inputs, times 2 (the two sum in different orders and both carry a few ulp at these sizes).
Measured on an MI355X, max abs error of this library (of torch's float32 kernels), worst case of each kind — every
case is in profiles/step_tail.txt:
    cross-entropy loss      4.4e-7 (4.4e-7) at N = 3, K = 400; equal to torch's in 14 of 18 cases, below it in the rest
    cross-entropy dlogits   2.6e-8 (2.6e-8) at N = 1, K = 2; elsewhere equal to or below torch's (exp, log and sums in fp64)
    SGD after three steps   parameters 3.5e-7 (3.2e-7), momentum buffers 6.5e-7 (5.5e-7), both in the dampened mode
    checkpoint round trip   parameters 3.5e-7 either way (3.2e-7), momentum 5.7e-7 (5.5e-7)
"""
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


def _run_ce(logits, labels, k_hi, cap=3):
    st = _mods()
    ring = st.StatsRing(cap)
    out = torch.zeros(2, device="cuda")
    d = st.ce_topk(logits, labels, k_hi, ring, out)
    torch.cuda.synchronize()
    return d, ring, out


# ------------------------------------------------------------------------------------------------ CE parity
def _ce_cases():
    cases = []
    for N in (1, 3, 8, 65):
        for K in (1, 2, 27, 400):
            cases.append(("n%d_k%d" % (N, K), N, K, 0, False))
    cases.append(("n8_k27_stride", 8, 27, 3, False))
    cases.append(("n8_k400_pm80", 8, 400, 0, True))
    return cases


@pytest.mark.parametrize("name,N,K,pad,big", _ce_cases(), ids=[c[0] for c in _ce_cases()])
def test_ce_matches_float64_within_twice_torchs_own_error(name, N, K, pad, big):
    g = torch.Generator().manual_seed(N * 1000 + K)
    x = torch.randn(N, K + pad, generator=g) * 3.0
    if big:  # one row near +-80: exp() of the raw values would overflow float32 — the max-subtraction path
        x[2] = torch.where(torch.rand(K, generator=g) < 0.5, torch.tensor(80.0), torch.tensor(-80.0)) + \
            torch.randn(K, generator=g) * 0.01
    y = torch.randint(0, K, (N,), generator=g)
    xv = x[:, :K]
    x64 = xv.double().requires_grad_(True)
    ref_loss = F.cross_entropy(x64, y)
    ref_loss.backward()
    xg = x.cuda()[:, :K].detach().requires_grad_(True)  # the same strided view on the GPU
    t_loss = F.cross_entropy(xg, y.cuda())
    t_loss.backward()
    d, ring, out = _run_ce(x.cuda()[:, :K], y.cuda(), min(5, K))
    e_loss = abs(float(out[0].double().cpu()) - float(ref_loss.detach()))
    t_e_loss = abs(float(t_loss.detach().double().cpu()) - float(ref_loss.detach()))
    e_grad = float((d.double().cpu() - x64.grad).abs().max())
    t_e_grad = float((xg.grad.double().cpu() - x64.grad).abs().max())
    print("ce %s: loss err %.3e (torch %.3e)  dlogits err %.3e (torch %.3e)" % (name, e_loss, t_e_loss, e_grad, t_e_grad))
    assert e_loss <= 2 * t_e_loss and e_grad <= 2 * t_e_grad
    assert float(ring.rows[0, 0]) == float(out[0]) and float(ring.rows[0, 3]) == 0.0 == float(out[1])
    assert float(ring.rows[0, 4]) == N and float(ring.rows[0, 5]) == 0.0


# ------------------------------------------------------------------------------------------------ top-k
def _topks_err(preds, labels, ks):
    """tools/train_net.py:122-125 on utils/metrics.py:9-42 (topks_correct with torch.topk), in float32 as there."""
    _, inds = torch.topk(preds, max(ks), dim=1, largest=True, sorted=True)
    correct = inds.t().eq(labels.view(1, -1).expand(max(ks), -1))
    return [float((1.0 - correct[:k, :].reshape(-1).float().sum() / preds.size(0)) * 100.0) for k in ks]


@pytest.mark.parametrize("N,K", [(3, 7), (8, 27), (65, 400)])
def test_topk_counts_match_topks_correct(N, K):
    g = torch.Generator().manual_seed(N + K)
    # tie-free: every row a permutation of K distinct values
    x = torch.stack([torch.randperm(K, generator=g).float() * 0.37 - 5.0 for _ in range(N)])
    y = torch.randint(0, K, (N,), generator=g)
    for k_hi in (1, 5, K):
        d, ring, out = _run_ce(x.cuda(), y.cuda(), k_hi)
        want = _topks_err(x, y, (1, k_hi))
        got = [float(ring.rows[0, 1]), float(ring.rows[0, 2])]
        assert got == want, (k_hi, got, want)
    assert want[1] == 0.0  # k = K: every row is a hit
    import sfhip
    with pytest.raises(sfhip.SfhipError):
        _run_ce(x.cuda(), y.cuda(), K + 1)


def test_topk_ties_go_to_the_lower_index():
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0],   # label 2: one equal value in front of it -> rank 1
                      [1.0, 3.0, 3.0, 2.0],   # label 1: rank 0
                      [5.0, 5.0, 5.0, 5.0],   # label 3: rank 3
                      [5.0, 5.0, 5.0, 5.0]])  # label 1: rank 1
    y = torch.tensor([2, 1, 3, 1])
    d, ring, out = _run_ce(x.cuda(), y.cuda(), 2)
    assert float(ring.rows[0, 1]) == 75.0 and float(ring.rows[0, 2]) == 25.0  # top-1: row 1; top-2: rows 0, 1, 3
    d, ring, out = _run_ce(x.cuda(), y.cuda(), 4)
    assert float(ring.rows[0, 2]) == 0.0
    d, ring, out = _run_ce(x.cuda(), y.cuda(), 3)
    assert float(ring.rows[0, 2]) == 25.0  # rank 3 is outside the top 3


# ------------------------------------------------------------------------------------------------ bad inputs
def test_nan_row_sets_the_flag_and_counts_as_wrong():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 27, generator=g)
    y = x.argmax(dim=1)  # every row right ...
    clean = _run_ce(x.cuda(), y.cuda(), 5)
    assert float(clean[1].rows[0, 1]) == 0.0 and float(clean[1].rows[0, 3]) == 0.0
    for poison in (float("nan"), float("inf")):
        xb = x.clone()
        xb[1, 3] = poison
        d, ring, out = _run_ce(xb.cuda(), y.cuda(), 5)
        assert float(ring.rows[0, 3]) == 1.0 and float(out[1]) == 1.0
        assert float(ring.rows[0, 1]) == 25.0 and float(ring.rows[0, 2]) == 25.0  # ... but the poisoned one, for every k
        assert float(ring.rows[0, 5]) == 0.0
        assert torch.isnan(out[0]) and torch.isnan(ring.rows[0, 0])
        # the other rows' gradients are those of the clean run
        keep = [0, 2, 3]
        assert _same_bits(d[keep], clean[0][keep])
    # the label itself poisoned with +inf: still wrong
    xb = x.clone()
    xb[1, y[1]] = float("inf")
    d, ring, out = _run_ce(xb.cuda(), y.cuda(), 5)
    assert float(ring.rows[0, 1]) == 25.0 and float(ring.rows[0, 3]) == 1.0


def test_labels_outside_the_classes_are_counted_and_skipped():
    g = torch.Generator().manual_seed(6)
    N, K = 5, 27
    x = torch.randn(N, K, generator=g)
    y = x.argmax(dim=1)
    yb = y.clone()
    yb[1], yb[3] = -1, K
    d, ring, out = _run_ce(x.cuda(), yb.cuda(), 5)
    assert float(ring.rows[0, 5]) == 2.0 and float(ring.rows[0, 3]) == 0.0
    wrong = float((1.0 - torch.tensor(3.0) / N) * 100.0)  # two of five wrong, in float32 as train_net.py:123-125
    assert float(ring.rows[0, 1]) == wrong and float(ring.rows[0, 2]) == wrong
    assert bool((d[1] == 0).all()) and bool((d[3] == 0).all())
    good = _run_ce(x.cuda(), y.cuda(), 5)
    keep = [0, 2, 4]
    assert _same_bits(d[keep], good[0][keep])  # neighbours intact: still (softmax - onehot) / N
    x64 = x.double()
    want = sum(float(F.cross_entropy(x64[i:i + 1], y[i:i + 1])) for i in keep) / N
    assert abs(float(out[0]) - want) <= 1e-6 * want


# ------------------------------------------------------------------------------------------------ ring, owned memory
def test_ring_rows_wrap_and_counter_counts():
    st = _mods()
    ring = st.StatsRing(3)
    out = torch.zeros(2, device="cuda")
    g = torch.Generator().manual_seed(7)
    losses = []
    for i in range(5):
        x = torch.randn(4, 9, generator=g)
        y = torch.randint(0, 9, (4,), generator=g)
        st.ce_topk(x.cuda(), y.cuda(), 5, ring, out)
        losses.append(float(out[0]))
    assert int(ring.counter[0]) == 5
    rows = ring.rows.cpu()
    # steps 0..4 landed in rows 0, 1, 2, 0, 1
    assert [float(rows[0, 0]), float(rows[1, 0]), float(rows[2, 0])] == [losses[3], losses[4], losses[2]]
    assert len(set(losses)) == 5


def test_ce_writes_only_what_it_owns_and_repeats_its_bits():
    st = _mods()
    g = torch.Generator().manual_seed(8)
    N, K, cap = 7, 29, 3
    x = (torch.randn(N, K + 3, generator=g)).cuda()[:, :K]
    y = torch.randint(0, K, (N,), generator=g).cuda()
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
        st.ce_topk(x, y, 5, ring, out, dlogits=d)
        torch.cuda.synchronize()
        assert _margins_intact(wd) and _margins_intact(wr) and _margins_intact(wo)
        assert bool((cnt_whole[:64] == 12345).all()) and bool((cnt_whole[65:] == 12345).all()) and int(cnt_whole[64]) == 2
        assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(out).all())
        assert bool(torch.isnan(rows[0]).all()) and bool(torch.isnan(rows[2]).all())  # only row 1 was written
        assert bool(torch.isfinite(rows[1]).all()) and float(rows[1, 6]) == 0.0 == float(rows[1, 7])
        runs.append((d.clone(), rows[1].clone(), out.clone()))
    for a, b in zip(*runs):
        assert _same_bits(a, b)


def test_autograd_function_and_backward_direct():
    st = _mods()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(6, 27, generator=g).cuda()
    y = torch.randint(0, 27, (6,), generator=g).cuda()
    loss_fun = st.HipCrossEntropy(5, st.StatsRing(4))
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


# ------------------------------------------------------------------------------------------------ SGD
def _chunk():
    import sfhip
    return sfhip.lib().sf_sgd_chunk_elems()


def _sgd_problem(seed=0):
    """Eight tensors (the chunk path's edge sizes), gradients packed tightly into one flat buffer as FlatGradients
    does: behind the one-element tensor some views are 4-byte- but not 16-byte-aligned, others are aligned again."""
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


SGD_MODES = {"nesterov": dict(momentum=0.9, nesterov=True), "dampened": dict(momentum=0.9, dampening=0.1),
             "plain": dict(momentum=0.0)}
LRS = (0.1, 0.05, 0.2)
SKIP = 3  # this parameter has grad None throughout


def _three_steps(make_opt, device, dtype, steps=3, grads_from=0):
    numels, p0, grads = _sgd_problem()
    params = [torch.nn.Parameter(p.to(device=device, dtype=dtype)) for p in p0]
    flat = torch.zeros(sum(numels), device=device, dtype=dtype)
    _bind(params, flat, SKIP)
    opt = make_opt(_groups(params))
    for s in range(steps):
        for gr in opt.param_groups:
            gr["lr"] = LRS[s]
        _load(flat, grads[grads_from + s], dtype)
        opt.step()
    return params, opt, flat


def _err(params, opt, ref_params, ref_opt):
    ep = max(float((a.detach().double().cpu() - b.detach()).abs().max()) for a, b in zip(params, ref_params))
    em = 0.0
    for a, b in zip(params, ref_params):
        mb = ref_opt.state.get(b, {}).get("momentum_buffer")
        if mb is not None:
            em = max(em, float((opt.state[a]["momentum_buffer"].double().cpu() - mb).abs().max()))
    return ep, em


@pytest.mark.parametrize("mode", list(SGD_MODES))
def test_sgd_matches_float64_within_twice_torchs_own_error(mode):
    st = _mods()
    kw = SGD_MODES[mode]
    ref_p, ref_o, _ = _three_steps(lambda g: torch.optim.SGD(g, lr=0.1, **kw), "cpu", torch.float64)
    t_p, t_o, _ = _three_steps(lambda g: torch.optim.SGD(g, lr=0.1, foreach=True, **kw), "cuda", torch.float32)
    h_p, h_o, flat = _three_steps(lambda g: st.HipSGD(g, lr=0.1, **kw), "cuda", torch.float32)
    torch.cuda.synchronize()
    # the gradient views really are a mix of 16-byte aligned and merely 4-byte aligned ones
    al = [p.grad.data_ptr() % 16 for i, p in enumerate(h_p) if i != SKIP]
    assert 0 in al and any(a in (4, 8, 12) for a in al)
    ep, em = _err(h_p, h_o, ref_p, ref_o)
    tp, tm = _err(t_p, t_o, ref_p, ref_o)
    print("sgd %s: param err %.3e (torch %.3e)  momentum err %.3e (torch %.3e)" % (mode, ep, tp, em, tm))
    assert ep <= 2 * tp and em <= 2 * tm
    _, p0, _ = _sgd_problem()
    assert torch.equal(h_p[SKIP].detach().cpu(), p0[SKIP])  # grad None: untouched, no state
    assert "momentum_buffer" not in h_o.state.get(h_p[SKIP], {})
    if kw["momentum"]:
        assert all(h_o.state[p]["momentum_buffer"].data_ptr() % 16 == 0 for i, p in enumerate(h_p) if i != SKIP)
        assert len(h_o._blocks) == 1
    else:
        assert all("momentum_buffer" not in h_o.state.get(p, {}) for p in h_p)


def test_sgd_zero_grad_and_guard():
    st = _mods()
    kw = SGD_MODES["nesterov"]
    base_p, base_o, base_flat = _three_steps(lambda g: st.HipSGD(g, lr=0.1, **kw), "cuda", torch.float32)

    class Zeroing(st.HipSGD):
        def step(self, closure=None):
            return super().step(closure, zero_grad=True)
    z_p, z_o, z_flat = _three_steps(lambda g: Zeroing(g, lr=0.1, **kw), "cuda", torch.float32)
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
    # a guard that reads non-zero: nothing moves — parameters, momentum, gradients
    before = [p.detach().clone() for p in base_p]
    mom = [base_o.state[p]["momentum_buffer"].clone() for i, p in enumerate(base_p) if i != SKIP]
    gflat = base_flat.clone()
    for bad in (1.0, float("nan")):
        base_o.step(guard=torch.tensor([bad], device="cuda"), zero_grad=True)
    torch.cuda.synchronize()
    for a, b in zip(base_p, before):
        assert _same_bits(a.detach(), b)
    for a, b in zip([base_o.state[p]["momentum_buffer"] for i, p in enumerate(base_p) if i != SKIP], mom):
        assert _same_bits(a, b)
    assert _same_bits(base_flat, gflat)
    base_o.step(guard=torch.tensor([0.0], device="cuda"))
    assert not _same_bits(base_p[0].detach(), before[0])


def test_step_with_a_new_lr_does_not_wait_for_the_device():
    """The reference sets a new learning rate every iteration (train_net.py:68-69): step() and upload_hyper() must
    hand the values to the stream and return while earlier work is still running there."""
    st = _mods()
    h_p, h_o, flat = _three_steps(lambda g: st.HipSGD(g, lr=0.1, **SGD_MODES["nesterov"]), "cuda", torch.float32)
    a = torch.randn(8192, 8192, device="cuda")
    b = torch.mm(a, a)  # warm: the first call loads its kernel
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    fresh = _sgd_problem()[2][3]  # a fourth set of gradients (torch's nesterov step changes the ones it read in place)
    _load(flat, fresh, torch.float32)
    for _ in range(6):  # tens of milliseconds of device time queued in front of the step
        torch.mm(a, a, out=b)
    for gr in h_o.param_groups:
        gr["lr"] = 0.0123
    h_o.step()
    for gr in h_o.param_groups:
        gr["lr"] = 0.0456
    assert h_o.upload_hyper() and not h_o.upload_hyper()
    done.record()
    assert not done.query(), "the host waited for the device inside step() / upload_hyper()"
    torch.cuda.synchronize()
    assert h_o._hyper_dev[:, 0].tolist() == [float(torch.tensor(0.0456, dtype=torch.float32))] * 2
    # and the step in between used ITS value: redo it from the same state with blocking torch ops
    ref_p, ref_o, ref_flat = _three_steps(lambda g: torch.optim.SGD(g, lr=0.1, foreach=True, **SGD_MODES["nesterov"]),
                                          "cuda", torch.float32)
    for gr in ref_o.param_groups:
        gr["lr"] = 0.0123
    _load(ref_flat, fresh, torch.float32)
    ref_o.step()
    ep = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(h_p, ref_p))
    assert ep < 1e-5  # lr 0.0456 or 0.2 instead of 0.0123 would move parameters by ~1e-2


def test_checkpoint_round_trip_with_torch_sgd():
    st = _mods()
    kw = SGD_MODES["dampened"]
    numels, _, grads = _sgd_problem()
    ref_p, ref_o, ref_flat = _three_steps(lambda g: torch.optim.SGD(g, lr=0.1, **kw), "cpu", torch.float64, steps=2)
    h_p, h_o, h_flat = _three_steps(lambda g: st.HipSGD(g, lr=0.1, **kw), "cuda", torch.float32, steps=2)
    t_p, t_o, t_flat = _three_steps(lambda g: torch.optim.SGD(g, lr=0.1, foreach=True, **kw), "cuda", torch.float32,
                                    steps=2)
    # HipSGD's state into a fresh torch SGD over the same parameter values, and torch's into a fresh HipSGD
    a_p = [torch.nn.Parameter(p.detach().clone()) for p in h_p]
    a_flat = torch.zeros_like(h_flat)
    _bind(a_p, a_flat, SKIP)
    a_o = torch.optim.SGD(_groups(a_p), lr=0.1, foreach=True, **kw)
    a_o.load_state_dict(h_o.state_dict())
    b_p = [torch.nn.Parameter(p.detach().clone()) for p in t_p]
    b_flat = torch.zeros_like(t_flat)
    _bind(b_p, b_flat, SKIP)
    b_o = st.HipSGD(_groups(b_p), lr=0.1, **kw)
    b_o.load_state_dict(t_o.state_dict())
    for i, p in enumerate(b_p):  # loaded buffers live in the optimizer's own allocation
        if i != SKIP:
            mb = b_o.state[p]["momentum_buffer"]
            assert mb.data_ptr() == b_o._slots[p].data_ptr() and mb.data_ptr() % 16 == 0
    for opt, flat, dtype in ((ref_o, ref_flat, torch.float64), (a_o, a_flat, torch.float32), (b_o, b_flat, torch.float32),
                             (t_o, t_flat, torch.float32)):
        for gr in opt.param_groups:
            gr["lr"] = LRS[2]
        _load(flat, grads[2], dtype)
        opt.step()
    torch.cuda.synchronize()
    tp, tm = _err(t_p, t_o, ref_p, ref_o)          # torch float32 all the way
    ap, am = _err(a_p, a_o, ref_p, ref_o)          # two HipSGD steps, then torch
    bp, bm = _err(b_p, b_o, ref_p, ref_o)          # two torch steps, then HipSGD
    print("round trip: torch %.3e / %.3e  hip->torch %.3e / %.3e  torch->hip %.3e / %.3e" % (tp, tm, ap, am, bp, bm))
    assert ap <= 2 * tp and am <= 2 * tm and bp <= 2 * tp and bm <= 2 * tm


def test_captured_step_follows_the_lr_schedule():
    st = _mods()
    from slowfast.models import engine
    kw = SGD_MODES["nesterov"]
    g = torch.Generator().manual_seed(21)
    N, K = 6, 27
    logits0 = torch.randn(N, K, generator=g).cuda()
    labels = torch.randint(0, K, (N,), generator=g).cuda()
    w0 = torch.randn(K, generator=g).cuda()
    lrs = (0.3, 0.05, 0.7)

    def make():
        logits = logits0.clone().requires_grad_(True)   # a leaf: its .grad is what the optimizer reads
        bias = torch.nn.Parameter(w0.clone())           # a second parameter, in a group with weight decay
        bias.grad = torch.zeros_like(bias)
        ring = st.StatsRing(8)
        loss_fun = st.HipCrossEntropy(5, ring)
        opt = st.HipSGD([{"params": [logits]}, {"params": [bias], "weight_decay": 0.01}], lr=0.1, **kw)

        def step():
            loss_fun(logits, labels)
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
    eager = (logits.detach().clone(), bias.detach().clone(), ring.rows.clone(), int(ring.counter[0]))

    # replay: the same warm-up, one captured step, replayed under the same schedule
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
    assert len(set(ring.rows[:6, 0].tolist())) == 6  # the replayed loss kernel advanced the slot every time
