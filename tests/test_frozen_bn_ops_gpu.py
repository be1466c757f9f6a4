"""sf_bn_frozen_bwd (csrc/bn_frozen.hip) through the binding against a float64 restatement on the CPU:

    g = sum_{q<rep} dy[n, t*rep+q] * m(y),   dz = gamma * invstd * g,   dres (=|+=) g,
    dbeta += sum g,   dgamma += sum g * (z - mean) * invstd

at 1e-5 relative L2 per output.  Shapes: C in {3, 4, 20, 64} (scalar and float4 forms, C below and not a multiple of the
block's channel tile), positions in {1, 7, 165, 2196} (one block; ragged multi-block partials — 165 rows split in two
blocks at C = 64, 2196 rows in 2 to 18 blocks at every C, which also enters the four-rows-per-trip loop), rep in {1, 4},
ReLU / ReLU6 / none with y on exact zeros and sixes, dres absent / written / accumulated, channel slices at a non-zero
offset of a wider pitch whose other channels must keep their bits, the byte-mask form against the y form, the gradient
sink's targets against fresh temporaries, and two runs of everything: the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-5
DIMS = {1: (1, 1, 1, 1), 7: (1, 1, 7, 1), 165: (1, 3, 5, 11), 2196: (2, 2, 9, 61)}
# C -> (pitch, offset): float4-addressable slices for 4 / 20 / 64, a scalar one for 3
VIEWS = {3: (8, 2), 4: (12, 4), 20: (28, 4), 64: (72, 4)}


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    n = float(b.norm())
    return float((a - b).norm()) / n if n > 0 else float((a - b).norm())


def _make(C, rows, rep, act, seed, pitch, coff):
    """Random operands in pitch-wide buffers (every channel filled, so untouched ones can be compared bit for bit)."""
    g = torch.Generator().manual_seed(seed)
    N, T, H, W = DIMS[rows]
    z = torch.randn(N, T, H, W, pitch, generator=g) * 1.5 + 0.5
    ybase = torch.randn(N, T, H, W, pitch, generator=g) * 4.0 + 1.0
    flat = ybase.view(-1)
    k = torch.randperm(flat.numel(), generator=g)
    flat[k[: flat.numel() // 5]] = 0.0                          # exact zeros: no gradient through ReLU
    flat[k[flat.numel() // 5: 2 * (flat.numel() // 5)]] = 6.0   # exact sixes: no gradient through ReLU6
    if act:
        ybase.clamp_(min=0.0)
    if act == 6:
        ybase.clamp_(max=6.0)
    y = ybase.repeat_interleave(rep, dim=1).contiguous()        # the T repeat of the forward pass
    dy = torch.randn(N, T * rep, H, W, pitch, generator=g)
    dres = torch.randn(N, T, H, W, pitch, generator=g)
    mean = torch.randn(C, generator=g)
    invstd = torch.rand(C, generator=g) + 0.5
    gamma = torch.randn(C, generator=g)
    acc = torch.randn(2, C, generator=g)                        # what dgamma / dbeta hold before the call
    return dict(z=z, y=y, dy=dy, dres=dres, mean=mean, invstd=invstd, gamma=gamma, acc=acc, coff=coff, C=C, rep=rep)


def _reference(d, act, gamma=True):
    """float64: (dz, g, dbeta, dgamma) over the slice."""
    C, coff, rep = d["C"], d["coff"], d["rep"]
    sl = slice(coff, coff + C)
    z = d["z"][..., sl].double()
    y = d["y"][..., sl].double()
    dy = d["dy"][..., sl].double()
    m = torch.ones_like(y)
    if act:
        m = (y > 0).double()
    if act == 6:
        m = m * (y < 6).double()
    N, T, H, W, _ = z.shape
    g = (dy * m).view(N, T, rep, H, W, C).sum(2)
    inv, mu = d["invstd"].double(), d["mean"].double()
    k = inv * (d["gamma"].double() if gamma else 1.0)
    xh = (z - mu) * inv
    return k * g, g, g.sum((0, 1, 2, 3)), (g * xh).sum((0, 1, 2, 3))


def _mask_bytes(d, act):
    """The byte-per-4-channels mask sf_affine_fwd_mask leaves: bit e of byte [row, c/4] = channel c+e passes."""
    C, coff = d["C"], d["coff"]
    y = d["y"][..., coff:coff + C].reshape(-1, C // 4, 4)
    p = y > 0
    if act == 6:
        p = p & (y < 6)
    w = torch.tensor([1, 2, 4, 8], dtype=torch.int32)
    return (p.int() * w).sum(-1).to(torch.uint8).reshape(-1).contiguous()


def _run(d, act, dres_mode, use_mask=False, gamma=True, grads="acc", inplace=True):
    """One call on the GPU; returns (dz buffer, dres buffer or None, dgamma, dbeta) as CPU tensors."""
    import sfhip
    from sfhip import Act
    C, coff = d["C"], d["coff"]
    dev = torch.device("cuda")
    zb, yb, dyb, rb = d["z"].to(dev), d["y"].to(dev), d["dy"].to(dev), d["dres"].to(dev)
    z, y, dy = Act(zb, coff, C), Act(yb, coff, C), Act(dyb, coff, C)
    dres = Act(rb, coff, C) if dres_mode else None
    out = None
    if not inplace:
        ob = torch.full_like(zb, 7.0)
        out = Act(ob, coff, C)
    g = None
    if grads == "acc":
        g = (d["acc"][0].to(dev).clone(), d["acc"][1].to(dev).clone())
    elif grads == "zero":
        g = (torch.zeros(C, device=dev), torch.zeros(C, device=dev))
    elif grads == "sink":  # slices of one flat zero-filled buffer at an odd offset, as FlatGradients binds .grad
        flat = torch.zeros(2 * C + 5, device=dev)
        g = (flat[3:3 + C], flat[3 + C:3 + 2 * C])
    mask = _mask_bytes(d, act).to(dev) if use_mask else None
    sfhip.bn_frozen_bwd(dy, y if act else None, z, d["mean"].to(dev), d["invstd"].to(dev),
                        d["gamma"].to(dev) if gamma else None, act, rep=d["rep"], dres=dres,
                        dres_overwrite=dres_mode == "write", dz_out=out, grads=g, mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(dyb.cpu(), d["dy"]) and torch.equal(yb.cpu(), d["y"])  # inputs are read only
    if not inplace:
        assert torch.equal(zb.cpu(), d["z"])
    return ((zb if inplace else ob).cpu(), rb.cpu() if dres_mode else None,
            g[0].cpu() if g else None, g[1].cpu() if g else None)


def _check(d, act, dres_mode, got, gamma=True, grads="acc", base=None):
    C, coff = d["C"], d["coff"]
    dz_ref, g_ref, db_ref, dg_ref = _reference(d, act, gamma)
    dzb, rb, dg, db = got
    base = d["z"] if base is None else base
    outside = [c for c in range(dzb.shape[-1]) if not coff <= c < coff + C]
    assert torch.equal(dzb[..., outside], base[..., outside]), "dz: channels outside the slice changed"
    e = _rel(dzb[..., coff:coff + C], dz_ref)
    assert e <= TOL, ("dz", e)
    if dres_mode:
        assert torch.equal(rb[..., outside], d["dres"][..., outside]), "dres: channels outside the slice changed"
        want = g_ref + (d["dres"][..., coff:coff + C].double() if dres_mode == "acc" else 0.0)
        e = _rel(rb[..., coff:coff + C], want)
        assert e <= TOL, ("dres", dres_mode, e)
    if grads:
        a = d["acc"].double() if grads == "acc" else torch.zeros(2, C, dtype=torch.float64)
        e1, e2 = _rel(dg, a[0] + dg_ref), _rel(db, a[1] + db_ref)
        assert e1 <= TOL and e2 <= TOL, ("dgamma, dbeta", e1, e2)


@pytest.mark.parametrize("rows", sorted(DIMS))
@pytest.mark.parametrize("C", sorted(VIEWS))
def test_slices_of_a_wider_pitch_match_fp64_and_leave_their_neighbours(C, rows):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    pitch, coff = VIEWS[C]
    for rep in (1, 4):
        for act in (False, True, 6):
            for dres_mode in ((None, "write", "acc") if rep == 1 else (None,)):  # rep > 1 requires dres == NULL
                d = _make(C, rows, rep, act, 1000 * C + rows + rep, pitch, coff)
                got = _run(d, act, dres_mode)
                _check(d, act, dres_mode, got)
                again = _run(d, act, dres_mode)
                for a, b in zip(got, again):
                    assert (a is None and b is None) or torch.equal(a, b), "two runs differ"


@pytest.mark.parametrize("C,pitch,coff", [(64, 72, 3), (20, 21, 1), (4, 4, 0), (64, 64, 0), (3, 3, 0)])
def test_unaligned_and_dense_views(C, pitch, coff):
    """A float4-sized C at an offset (or pitch) that is not a multiple of 4 takes the scalar form; dense views."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    for rows in (165, 2196):
        for act, dres_mode in ((True, "acc"), (6, "write"), (False, None)):
            d = _make(C, rows, 1, act, 77 + C + rows, pitch, coff)
            _check(d, act, dres_mode, _run(d, act, dres_mode))
    d = _make(C, 165, 4, True, 5, pitch, coff)
    _check(d, True, None, _run(d, True, None))


@pytest.mark.parametrize("C", [4, 20, 64])
@pytest.mark.parametrize("act", [True, 6])
def test_byte_mask_form_gives_the_bits_of_the_y_form(C, act):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    pitch, coff = VIEWS[C]
    for rows in (7, 165, 2196):
        for dres_mode in (None, "write", "acc"):
            d = _make(C, rows, 1, act, 31 * C + rows, pitch, coff)
            from_y = _run(d, act, dres_mode)
            from_mask = _run(d, act, dres_mode, use_mask=True)
            _check(d, act, dres_mode, from_mask)
            for a, b in zip(from_y, from_mask):
                assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("C", sorted(VIEWS))
def test_grad_sink_targets_fresh_temporaries_no_affine_and_a_separate_dz(C):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    pitch, coff = VIEWS[C]
    for rows in (7, 2196):
        d = _make(C, rows, 1, True, 9 * C + rows, pitch, coff)
        plain = _run(d, True, "acc", grads="zero")
        sink = _run(d, True, "acc", grads="sink")  # unaligned slices of a flat buffer: the same bits
        _check(d, True, "acc", plain, grads="zero")
        for a, b in zip(plain, sink):
            assert torch.equal(a, b)
        # a BN without affine: dz = invstd * g, no sums
        bare = _run(d, True, "write", gamma=False, grads=None)
        _check(d, True, "write", bare, gamma=False, grads=None)
        # dz into another buffer: z is left alone, the other channels of the target keep their bits
        sep = _run(d, True, None, inplace=False)
        _check(d, True, None, sep, base=torch.full_like(d["z"], 7.0))
        assert torch.equal(sep[0][..., coff:coff + C], plain[0][..., coff:coff + C])
