"""No GPU needed.  (1) The closed-form float64 references of tests/_backward_ref.py against float64 torch.autograd
through the library ops, at 1e-12 relative; (2) the case tables of test_backward_views_gpu.py against the restated
launch predicates: every case lands on the route it declares and every route of backward.hip's launchers is reached."""
import pytest
import torch
import torch.nn.functional as F

import _backward_ref as B
import test_backward_views_gpu as G

TIGHT = 1e-12


def _close(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= TIGHT * float(b.abs().max().clamp_min(1e-300)), float((a - b).abs().max())


def _cf(v):  # NDHWC -> NCTHW
    return v.permute(0, 4, 1, 2, 3)


def _cl(v):  # NCTHW -> NDHWC
    return v.permute(0, 2, 3, 4, 1)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================================================ references
@pytest.mark.parametrize("C,N,S,rep,relu,use_res", [(5, 2, 1, 1, 0, False), (4, 3, 1, 1, 1, True), (3, 2, 1, 4, 2, False),
                                                    (6, 4, 2, 1, 1, True), (3, 8, 4, 2, 2, False)])
def test_bn_backward_reference(C, N, S, rep, relu, use_res):
    g = _gen(C + 10 * S + rep)
    T, H, W = 2, 3, 2
    z = (torch.randn(N, T, H, W, C, generator=g) * 1.5 + 0.3).double().requires_grad_(True)
    gamma = (torch.rand(S * C, generator=g) + (2.5 if relu == 2 else 0.5)).double().requires_grad_(True)
    beta = (torch.randn(S * C, generator=g) * 0.1 + (2.0 if relu == 2 else 0.0)).double().requires_grad_(True)
    res = torch.randn(N, T, H, W, C, generator=g).double().requires_grad_(True) if use_res else None
    zc = _cf(z)
    y = F.batch_norm(zc.reshape(N // S, S * C, T, H, W), None, None, gamma, beta, True, 0.0, 1e-5).reshape(N, C, T, H, W)
    if use_res:
        y = y + _cf(res)
    y = F.relu6(y) if relu == 2 else (F.relu(y) if relu else y)
    y = _cl(y.repeat_interleave(rep, dim=2))
    dy = torch.randn(y.shape, generator=g).double()
    grads = torch.autograd.grad(y, [z, gamma, beta] + ([res] if use_res else []), dy)
    zd = z.detach()
    mean = torch.stack([zd[s::S].mean((0, 1, 2, 3)) for s in range(S)]).reshape(-1)
    var = torch.stack([zd[s::S].var((0, 1, 2, 3), unbiased=False) for s in range(S)]).reshape(-1)
    invstd = torch.rsqrt(var + 1e-5)
    gg, gmag = B.bn_g_ref(dy, B.act_pass(y.detach(), relu, rep), rep)
    dbeta, dgamma, mb, mg = B.bn_sums_ref(gg, gmag, zd, mean, invstd, S)
    dz, mag = B.bn_dz_ref(gg, gmag, zd, mean, invstd, gamma.detach(), dbeta, dgamma, S)
    _close(dz, grads[0])
    _close(dgamma, grads[1])
    _close(dbeta, grads[2])
    assert bool((mb >= dbeta.abs() * (1 - 1e-12)).all()) and bool((mg >= dgamma.abs() * (1 - 1e-12)).all())
    assert bool((mag >= dz.abs() * (1 - 1e-12)).all())
    if use_res:
        _close(B.dres_ref(gg, gmag, None)[0], grads[3])
        base = torch.randn(gg.shape, generator=g)
        _close(B.dres_ref(gg, gmag, base)[0], grads[3] + base.double())
    if relu:
        passed = float(B.act_pass(y.detach(), relu, rep).double().mean())
        assert 0.05 < passed < 0.98, passed


@pytest.mark.parametrize("k,s,p", [((1, 3, 3), (1, 2, 2), (0, 1, 1)), ((3, 3, 3), (1, 2, 2), (1, 1, 1)),
                                   ((2, 2, 2), (2, 2, 2), (0, 0, 0)), ((4, 1, 1), (4, 1, 1), (0, 0, 0))])
@pytest.mark.parametrize("ties", [False, True])
def test_maxpool_backward_reference(k, s, p, ties):
    """With exact ties (quantised, ReLU'd inputs: runs of zeros) the first maximum in scan order takes the gradient."""
    g = _gen(5)
    x = torch.randn(2, 4, 7, 6, 3, generator=g)
    if ties:
        x = torch.relu((x * 2).round() / 2)
        assert float((x == 0).double().mean()) > 0.3
    xd = x.double().requires_grad_(True)
    y = _cl(F.max_pool3d(_cf(xd), k, s, p))
    dy = torch.randn(y.shape, generator=g)
    (want,) = torch.autograd.grad(y, (xd,), dy.double())
    assert torch.equal(B.maxpool_fwd_ref(x, k, s, p).double(), y.detach())
    ref, mag = B.maxpool_bwd_ref(x, dy, k, s, p)
    _close(ref, want)
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
    base = torch.randn(x.shape, generator=g)
    _close(B.maxpool_bwd_ref(x, dy, k, s, p, base)[0], want + base.double())


@pytest.mark.parametrize("k,s,p,d", [((1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1)), ((3, 3, 3), (1, 2, 2), (1, 1, 1), (1, 1, 1)),
                                     ((1, 7, 7), (1, 2, 2), (0, 3, 3), (1, 1, 1)), ((1, 5, 5), (1, 2, 1), (0, 2, 2), (1, 1, 1)),
                                     ((1, 3, 3), (1, 1, 1), (0, 2, 2), (1, 2, 2)), ((3, 3, 1), (2, 1, 1), (2, 0, 0), (2, 1, 1))])
def test_depthwise_backward_reference(k, s, p, d):
    g = _gen(k[1] + s[1])
    C = 5
    x = torch.randn(2, 4, 9, 8, C, generator=g).double().requires_grad_(True)
    w = torch.randn(C, 1, *k, generator=g).double().requires_grad_(True)
    y = _cl(F.conv3d(_cf(x), w, None, s, p, d, C))
    assert tuple(y.shape[1:4]) == B.out_thw((4, 9, 8), k, s, p, d)
    dz = torch.randn(y.shape, generator=g).double()
    dx_want, dw_want = torch.autograd.grad(y, (x, w), dz)
    packed = w.detach().reshape(C, -1).t().contiguous()  # [taps, C]
    _close(B.dw_fwd_ref(x.detach(), packed, k, s, p, d), y.detach())
    dx, mag = B.dw_dgrad_ref(dz, packed, (4, 9, 8), k, s, p, d)
    _close(dx, dx_want)
    assert bool((mag >= dx.abs() * (1 - 1e-12)).all())
    dw, wmag = B.dw_wgrad_ref(x.detach(), dz, k, s, p, d)
    _close(B.dw_to_param(dw, k), dw_want)   # nn.Conv3d's layout [C][1][kT][kH][kW]
    _close(dw, dw_want.reshape(C, -1).t())  # the packed layout [tap][C]
    assert bool((wmag >= dw.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("alpha", [4, 8])
@pytest.mark.parametrize("C", [3, 8])
def test_eca_backward_references(C, alpha):
    g = _gen(C + alpha)
    N, T, H, W = 2, 8, 3, 2
    x = torch.relu((torch.randn(N, T, H, W, C, generator=g) * 2).round() / 2).double().requires_grad_(True)
    dz = torch.randn(N, T // alpha, H, W, C, generator=g).double()
    gate, dpool = torch.rand(N, C, generator=g).double(), torch.randn(N, C, generator=g).double()
    mx = _cl(F.max_pool3d(_cf(x), (alpha, 1, 1), (alpha, 1, 1)))
    _close(B.tmax_dot_ref(x.detach(), alpha, dz)[0], (mx.detach() * dz).sum((1, 2, 3)))
    (want,) = torch.autograd.grad((mx * (dz * gate.view(N, 1, 1, 1, C) + dpool.view(N, 1, 1, 1, C))).sum(), (x,))
    base = torch.randn(x.shape, generator=g)
    ref, mag = B.eca_apply_ref(x.detach(), alpha, dz, gate, dpool, base)
    _close(ref, want + base.double())
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
    # the gate: conv1d(k = 3, pad = 1, no bias) along the channel axis + sigmoid
    pooled = torch.randn(N, C, generator=g).double().requires_grad_(True)
    w3 = torch.randn(3, generator=g).double().requires_grad_(True)
    dg = torch.randn(N, C, generator=g).double()
    gt = torch.sigmoid(F.conv1d(pooled.unsqueeze(1), w3.view(1, 1, 3), None, 1, 1).squeeze(1))
    dp_want, dw_want = torch.autograd.grad(gt, (pooled, w3), dg)
    r = B.eca_gate_bwd_ref(dg, pooled.detach(), w3.detach(), 0.125)
    _close(r["gate"][0], gt.detach())
    _close(r["dpool"][0], dp_want * 0.125)
    _close(r["dw"][0], dw_want)
    for key in r:
        assert bool((r[key][1] >= 0).all())


def test_helper_references():
    g = _gen(3)
    a, b = torch.randn(2, 1, 3, 2, 6, generator=g).double(), torch.randn(2, 1, 3, 2, 6, generator=g).double()
    base = torch.randn(2, 1, 3, 2, 6, generator=g).double()
    _close(B.rowdot_ref(a, b, 0.3)[0], ((a * b).sum(-1) * 0.3).reshape(-1))
    _close(B.axpy_ref(a, -1.7, base)[0], base - 1.7 * a)
    _close(B.axpy_ref(a, -1.7, None)[0], -1.7 * a)
    v = torch.randn(2, 6, generator=g).double()
    _close(B.bcast_add_ref(base, v, 0.3)[0], base + 0.3 * v.view(2, 1, 1, 1, 6))
    for relu, fn in ((1, F.relu), (2, F.relu6)):
        x = (a * 4).requires_grad_(True)
        y = fn(x)
        (want,) = torch.autograd.grad(y, (x,), b)
        _close(B.act_bwd_ref(b, y.detach(), relu, None)[0], want)
        _close(B.act_bwd_ref(b, y.detach(), relu, base)[0], want + base)
    wide = torch.randn(2, 1, 3, 2, 20, generator=g).double()
    _close(B.gather_add_ref(wide, 3, 3, 6, base)[0], base + wide[..., [3, 6, 9, 12, 15, 18]])
    _close(B.gather_add_ref(wide, 1, 2, 6, None)[0], wide[..., [1, 3, 5, 7, 9, 11]])


# ================================================================================================ case tables
def _reduce_route(case):
    v = case["views"]
    return B.bn_reduce_route(case["C"], case["nthw"], v["dy"], v["z"], v["y"], case["rep"], case["relu"], case["S"])


def test_bn_reduce_cases_reach_their_routes():
    reached = set()
    for name, case in G.BN_REDUCE_CASES.items():
        r = _reduce_route(case)
        assert r != B.EINVAL and r["route"] == case["route"], (name, r)
        reached.add(r["route"])
        if name in G.BN_REDUCE_GEOMETRY:
            assert (r["P"], r["chunks"]) == G.BN_REDUCE_GEOMETRY[name], (name, r)
        assert r["P"] * 2 * case["C"] <= B.MAX_P * 2 * case["C"]  # the workspace sf_bn_bwd_ws_floats sizes
    assert reached == set(B.ROUTES["bn_reduce"]), reached
    for name in G.BN_MASK_RAGGED:  # byte mask through the four-rows-per-trip loop, with rows left for the tail loop
        case, r = G.BN_REDUCE_CASES[name], _reduce_route(G.BN_REDUCE_CASES[name])
        assert case["relu"] == 3 and r["four_row_trips"] and r["ragged_tail"], (name, r)
    # the final kernel's unrolled trip is taken by the lanes below P - 192 only
    assert 193 <= _reduce_route(G.BN_REDUCE_CASES["two_C64_P200"])["P"] < 256
    assert _reduce_route(G.BN_REDUCE_CASES["two_C64_P1024"])["P"] == B.MAX_P
    assert any(c["S"] == 2 and c["nthw"][0] == 4 for c in G.BN_REDUCE_CASES.values())
    assert any(c["S"] == 4 and c["nthw"][0] == 8 for c in G.BN_REDUCE_CASES.values())
    assert {c["relu"] for c in G.BN_REDUCE_CASES.values()} == {0, 1, 2, 3}
    assert any(c["rep"] == 4 for c in G.BN_REDUCE_CASES.values()) and any(c["acc"] for c in G.BN_REDUCE_CASES.values())


def test_bn_apply_cases_reach_their_routes():
    reached = set()
    for name, case in G.BN_APPLY_CASES.items():
        r = G._apply_route(case)
        assert r == case["route"], (name, r)
        reached.add(r)
    assert reached == set(B.ROUTES["bn_apply"]), reached
    u4 = [c for c in G.BN_APPLY_CASES.values() if c["route"] == "unroll4"]
    cvs = {c["C"] // 4 for c in u4}
    assert any(cv & (cv - 1) == 0 for cv in cvs) and any(cv & (cv - 1) for cv in cvs), "shift and divide decode"
    assert {(c["relu"], c["dres"]) for c in u4} >= {(r, m) for r in (0, 3) for m in (None, "acc", "first")}
    assert {c["over_z"] for c in u4} == {True, False} and any(c["S"] == 2 for c in u4)
    n, t, h, w = G.U4_256
    assert n * t * h * w * 64 == 262144  # exactly the threshold
    # each view alone takes the float4 path away from a C % 4 == 0 case
    alone = set()
    for c in G.BN_APPLY_CASES.values():
        bad = [k for k, v in c["views"].items() if not B.f4(v) and (k != "dres" or c["dres"]) and
               (k != "dz" or not c["over_z"]) and (k != "y" or c["relu"] in (1, 2))]
        if c["C"] % 4 == 0 and len(bad) == 1:
            assert c["route"] == "scalar"
            alone.add(bad[0])
    assert alone == {"dy", "z", "y", "dz", "dres"}, alone
    for name in G.BN_BIT_PAIRS:
        assert G._apply_route(G.BN_APPLY_CASES[name], False) == "vec4"


def test_other_cases_reach_their_routes():
    reached = set()
    for name, (C, kx, ky, kdy, kdx, route) in G.POOL_VIEWS.items():
        assert B.maxpool_bwd_route(C, G.vw(kx, C), G.vw(ky, C), G.vw(kdy, C), G.vw(kdx, C)) == route, name
        reached.add(route)
    assert reached == set(B.ROUTES["maxpool"])
    reached, shifts = set(), set()
    for name, (C, ka, kb, route, shift) in G.ROWDOT_CASES.items():
        assert B.rowdot_route(C, G.vw(ka, C), G.vw(kb, C))[:2] == (route, shift), name
        reached.add(route)
        shifts.add(shift)
    assert reached == set(B.ROUTES["rowdot"]) and shifts >= {0, 1, 4, 6}
    wreached, dreached, few_rows = set(), set(), False
    for name, (C, nthw, k, s, p, d, kx, kdz, kdx, wroute, droute) in G.DW_CASES.items():
        o = B.out_thw(nthw[1:], k, s, p, d)
        rows = nthw[0] * o[0] * o[1] * o[2]
        wr = B.dw_wgrad_route(C, rows, k[0] * k[1] * k[2], G.vw(kx, C), G.vw(kdz, C))
        assert wr[0] == wroute, (name, wr)
        assert B.dw_dgrad_route(C, G.vw(kdz, C), G.vw(kdx, C), C) == droute, name
        wreached.add(wroute)
        dreached.add(droute)
        few_rows |= rows < 64
        # the march is off in the GPU test; were it on, it would take these shapes away from the generic kernels
    assert wreached == set(B.ROUTES["dw_wgrad"]), wreached
    assert dreached == set(B.ROUTES["dw_dgrad"]) and few_rows
