"""The associative "dot_product" kernels (sf_gram / sf_rowmat, attn_assoc.hip) against torch fp64 on the CPU, measured as
max |a - b| / max |b| at the bound every attention op test uses (tests/test_ops_gpu.py, tests/test_xattn_gpu.py:
TOL = 2e-4), through the binding and through the Nonlocal block they serve.  Every view has pitch = width + 8 and
channel offset 4 in a buffer filled with a sentinel, and nothing outside the channel slice may change."""
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 2e-4
SENTINEL = 7.0

GRAM_SHAPES = [(1, 4, 4), (33, 20, 36), (150, 24, 48), (80, 256, 256), (45, 512, 512), (200, 132, 4), (3000, 16, 16)]
ROWMAT_SHAPES = [(1, 4, 4), (50, 20, 36), (300, 24, 48), (96, 256, 256), (70, 512, 512), (40, 132, 4), (40, 4, 132)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _view(x, fill=None):
    """[B, N, C] cpu tensor (or a shape, with `fill`) -> Act view with pitch C + 8 and channel offset 4."""
    import sfhip
    shape = tuple(x) if fill is not None else tuple(x.shape)
    B, n, c = shape
    buf = torch.full((B, 1, 1, n, c + 8), SENTINEL if fill is None else fill, dtype=torch.float32, device=_dev())
    if fill is None:
        buf[..., 4:4 + c] = x.view(B, 1, 1, n, c).to(buf.device)
    return sfhip.Act(buf, 4, c)


def _get(a):
    return a.buf[:, 0, 0, :, a.coff:a.coff + a.C].cpu()


def _pads_untouched(*acts):
    for a in acts:
        pad = torch.cat([a.buf[..., :4], a.buf[..., 4 + a.C:]], -1)
        assert bool(((pad == SENTINEL) | torch.isnan(pad)).all())


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _gram(a, b, alpha):
    """(G, Gt) on the CPU from cpu tensors a [B,R,da], b [B,R,db] through padded, offset views."""
    import sfhip
    av, bv = _view(a), _view(b)
    before = (av.buf.clone(), bv.buf.clone())
    G, Gt = sfhip.gram(av, bv, alpha, transposed=True)
    torch.cuda.synchronize()
    assert torch.equal(av.buf, before[0]) and torch.equal(bv.buf, before[1])  # inputs, pads included, are unchanged
    return G.cpu(), Gt.cpu()


def _rowmat(x, w, alpha, prev=None):
    """Y on the CPU; prev None: a NaN-filled Y overwritten, else accumulated onto prev."""
    import sfhip
    xv = _view(x)
    yv = _view((x.shape[0], x.shape[1], w.shape[1]), fill=float("nan")) if prev is None else _view(prev)
    out = sfhip.rowmat(xv, w.to(_dev()).contiguous(), alpha, out=yv, accumulate=prev is not None)
    torch.cuda.synchronize()
    assert out is yv
    _pads_untouched(xv, yv)
    return _get(yv)


def test_gram_sweep_holds_split_and_unsplit_shapes():
    """A later re-plan cannot quietly make the sweep below one-sided."""
    import sfhip
    splits = [sfhip.lib().sf_gram_splits(2, R, da, db) for R, da, db in GRAM_SHAPES]
    assert any(s > 1 for s in splits) and any(s == 1 for s in splits), splits


@pytest.mark.parametrize("R,da,db", GRAM_SHAPES)
def test_gram_sweep(R, da, db):
    """B = 2 different samples, alpha != 1: G and G^T against fp64, and G^T the exact transpose of G."""
    _dev()
    a, b, alpha = _randn((2, R, da), 100 + R), _randn((2, R, db), 200 + R), 0.37
    G, Gt = _gram(a, b, alpha)
    ref = alpha * (a.double().transpose(1, 2) @ b.double())
    errs = (_rel(G, ref), _rel(Gt, ref.transpose(1, 2)))
    print("gram %s: G %.2e Gt %.2e" % ((R, da, db), errs[0], errs[1]))
    assert G.shape == (2, da, db) and Gt.shape == (2, db, da)
    assert bool(torch.isfinite(G).all()) and max(errs) < TOL, errs
    assert torch.equal(Gt, G.transpose(1, 2))


def test_gram_two_tiles_per_wavefront():
    """8 samples of 512 x 512 are 2048 output tiles: the launcher then gives every wavefront two of them.  Same checks
    as the sweep, and sample 3 alone (one tile per wavefront) gives the same bits."""
    _dev()
    R, da, db = 40, 512, 512
    a, b, alpha = _randn((8, R, da), 21), _randn((8, R, db), 22), 0.37
    G, Gt = _gram(a, b, alpha)
    ref = alpha * (a.double().transpose(1, 2) @ b.double())
    assert max(_rel(G, ref), _rel(Gt, ref.transpose(1, 2))) < TOL
    assert torch.equal(Gt, G.transpose(1, 2))
    G1, _ = _gram(a[3:4].contiguous(), b[3:4].contiguous(), alpha)
    assert torch.equal(G[3], G1[0])


@pytest.mark.parametrize("R,k,n", ROWMAT_SHAPES)
def test_rowmat_sweep(R, k, n):
    """B = 2, alpha != 1: overwrite of a NaN-filled Y against fp64; accumulate onto a random Y = previous + fresh."""
    _dev()
    x, w, alpha = _randn((2, R, k), 300 + R), _randn((2, n, k), 400 + R), 1.7
    y = _rowmat(x, w, alpha)
    ref = alpha * (x.double() @ w.double().transpose(1, 2))
    err = _rel(y, ref)
    print("rowmat %s: %.2e" % ((R, k, n), err))
    assert bool(torch.isfinite(y).all()) and err < TOL, err
    prev = _randn((2, R, n), 500 + R)
    assert _rel(_rowmat(x, w, alpha, prev=prev), prev + y) < 1e-6


def test_two_runs_give_the_same_bits():
    import sfhip
    _dev()
    R, da, db = 3000, 16, 16
    assert sfhip.lib().sf_gram_splits(2, R, da, db) > 1
    a, b = _randn((2, R, da), 1), _randn((2, R, db), 2)
    first, second = _gram(a, b, 0.5), _gram(a, b, 0.5)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    x, w = _randn((2, 300, 24), 3), _randn((2, 48, 24), 4)
    assert torch.equal(_rowmat(x, w, 1.0), _rowmat(x, w, 1.0))


@pytest.mark.parametrize("R,da,db", [(3000, 16, 16), (80, 256, 256)])
def test_samples_do_not_mix(R, da, db):
    """B = 3 with sample 1 all zeros: G[1] is exactly 0, and samples 0 and 2 carry the bits of their B = 1 runs (the
    chunk plan does not depend on B).  A split and an unsplit shape; rowmat the same way."""
    _dev()
    a, b = _randn((3, R, da), 5), _randn((3, R, db), 6)
    a[1], b[1] = 0.0, 0.0
    G, Gt = _gram(a, b, 0.25)
    assert float(G[1].abs().max()) == 0.0 and float(Gt[1].abs().max()) == 0.0
    for n in (0, 2):
        G1, Gt1 = _gram(a[n:n + 1].contiguous(), b[n:n + 1].contiguous(), 0.25)
        assert torch.equal(G[n], G1[0]) and torch.equal(Gt[n], Gt1[0])
    w = _randn((3, db, da), 7)
    w[1] = 0.0
    y = _rowmat(a, w, 1.0)
    assert float(y[1].abs().max()) == 0.0
    for n in (0, 2):
        assert torch.equal(y[n], _rowmat(a[n:n + 1].contiguous(), w[n:n + 1].contiguous(), 1.0)[0])


def _act(x):
    import sfhip
    return sfhip.Act(x.detach().permute(0, 2, 3, 4, 1).contiguous().to(_dev()))


def _back(a):
    return a.buf[..., a.coff:a.coff + a.C].permute(0, 4, 1, 2, 3).contiguous().cpu()


def test_nonlocal_dot_product_key_width_not_a_multiple_of_16():
    """Nonlocal(40, 20, (1,2,2), "dot_product"): d = 20.  Train mode: output, input gradient and every parameter
    gradient against oracle.nonlocal_block under fp64 autograd, measured as
    tests/test_xattn_gpu.py::test_nonlocal_key_width_not_a_multiple_of_16 measures them; then the same block in eval
    mode, forward only."""
    from oracle import slowfast_oracle as oracle
    from slowfast.models import engine
    from slowfast.models.nonlocal_helper import Nonlocal
    dev = _dev()
    torch.manual_seed(40)
    dim, pool, inst, thw = 40, (1, 2, 2), "dot_product", (2, 6, 6)
    blk = Nonlocal(dim, dim // 2, pool, instantiation=inst).to(dev).train()
    with torch.no_grad():
        for k, v in blk.named_parameters():
            v.copy_(torch.randn_like(v) * (0.3 if v.dim() > 1 else 0.2) + (1.0 if k == "bn.weight" else 0.0))
    x = torch.randn((2, dim) + thw)
    dy = torch.randn((2, dim) + thw)
    sd = {"m." + k: v.detach().double().cpu().requires_grad_(v.dtype.is_floating_point and "running" not in k)
          for k, v in blk.state_dict().items() if "num_batches" not in k}
    xr = x.double().requires_grad_(True)
    ref = oracle.nonlocal_block(sd, "m", xr, pool, inst, True)
    ref.backward(dy.double())
    t = engine.Tape()
    xa = _act(x)
    with torch.no_grad(), engine.taping(t):
        ya = blk.run(xa)
        out = _back(ya)
        t.grad_of(ya).buf.copy_(dy.permute(0, 2, 3, 4, 1).to(dev))
        dxa = t.grad_of(xa)
        t.backward()
    torch.cuda.synchronize()
    errs = {"y": _rel(out, ref), "dx": _rel(_back(dxa), xr.grad)}
    for k, v in blk.named_parameters():
        a, b = t.pgrads[v].double().cpu(), sd["m." + k].grad
        scale = b.abs().max()
        if k.endswith(".bias"):  # exactly-zero bias gradients carry cancellation noise only: relative to the weight's
            scale = torch.maximum(scale, sd["m." + k[:-4] + "weight"].grad.abs().max())
        errs[k] = float((a.reshape(b.shape) - b).abs().max() / scale.clamp_min(1e-30))
    print("nonlocal dot_product d=20:", {k: "%.2e" % e for k, e in errs.items()})
    assert max(errs.values()) < TOL, errs
    # eval mode: the running statistics the train-mode forward just updated
    blk.eval()
    sd_eval = {"m." + k: v.detach().double().cpu() for k, v in blk.state_dict().items() if "num_batches" not in k}
    ref_eval = oracle.nonlocal_block(sd_eval, "m", x.double(), pool, inst, False)
    with torch.no_grad():
        out_eval = _back(blk.run(_act(x)))
    torch.cuda.synchronize()
    err = _rel(out_eval, ref_eval)
    print("nonlocal dot_product d=20 eval: %.2e" % err)
    assert err < TOL, err


def test_no_score_matrix_in_memory():
    """Nonlocal(32, 16, None, "dot_product") on x [1,32,2,48,48]: N_q = N_k = 4608, one score matrix = 85 MB.  Taped
    forward plus backward may raise the allocator's peak by less than 24 MB (the softmax twin's bound)."""
    from slowfast.models import engine
    from slowfast.models.nonlocal_helper import Nonlocal
    dev = _dev()
    torch.manual_seed(3)
    blk = Nonlocal(32, 16, None, instantiation="dot_product").to(dev).train()
    xa = _act(torch.randn(1, 32, 2, 48, 48))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t = engine.Tape()
    with torch.no_grad(), engine.taping(t):
        ya = blk.run(xa)
        t.grad_of(ya).buf.fill_(1.0)
        dxa = t.grad_of(xa)
        t.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise %.1f MB" % (rise / 1e6))
    assert bool(torch.isfinite(dxa.buf).all())
    assert rise < 24e6, rise


def test_nonlocal_forward_is_one_gram_and_one_rowmat():
    """B = 4, eval: between the g projection and conv_out the trace holds one gram and one rowmat for the whole batch,
    no per-sample conv and no row_softmax."""
    import sfhip
    from slowfast.models.nonlocal_helper import Nonlocal
    dev = _dev()
    torch.manual_seed(4)
    blk = Nonlocal(32, 16, (1, 2, 2), instantiation="dot_product").to(dev).eval()
    xa = _act(torch.randn(4, 32, 2, 8, 8))
    sfhip.EVENT_TRACE = []
    try:
        with torch.no_grad():
            blk.run(xa)
        torch.cuda.synchronize()
        tags = [e[0] for e in sfhip.EVENT_TRACE]
    finally:
        sfhip.EVENT_TRACE = None
    kinds = [tg[0] for tg in tags]
    assert kinds.count("gram") == 1 and kinds.count("rowmat") == 1 and "row_softmax" not in kinds, kinds
    i, j = kinds.index("gram"), kinds.index("rowmat")
    assert tags[i] == ("gram", 4, 32, 16, 16), tags[i]
    assert tags[j] == ("rowmat", 4, 128, 16, 16), tags[j]
    assert i < j and kinds[:i].count("conv") == 3 and kinds[i + 1:j].count("conv") == 0, kinds
    assert kinds[j + 1:].count("conv") == 1, kinds


def test_widths_above_512_keep_the_materialised_route():
    """dense_attention(softmax=False) at d = dv = 528, 16 queries of a [1, ., 1, 4, 4] block against 4 keys: refused by
    sf_assoc_accepts, so the per-sample convs run, and the result still matches fp64."""
    import sfhip
    from slowfast.models import nonlocal_helper
    dev = _dev()
    d = 528
    theta, phi, g = _randn((1, 1, 4, 4, d), 8), _randn((1, 1, 2, 2, d), 9), _randn((1, 1, 2, 2, d), 10)
    acts = [sfhip.Act(t.to(dev)) for t in (theta, phi, g)]
    assert not sfhip.assoc_accepts(*acts)
    sfhip.EVENT_TRACE = []
    try:
        with torch.no_grad():
            y = nonlocal_helper.dense_attention(acts[0], acts[1], acts[2], softmax=False)
        torch.cuda.synchronize()
        kinds = [e[0][0] for e in sfhip.EVENT_TRACE]
    finally:
        sfhip.EVENT_TRACE = None
    assert "conv" in kinds and "gram" not in kinds and "rowmat" not in kinds, kinds
    th, ph, gg = [t.double().view(1, -1, d) for t in (theta, phi, g)]
    ref = ((th @ ph.transpose(1, 2)) / 4.0) @ gg
    assert _rel(y.buf.view(1, 16, d), ref) < TOL
