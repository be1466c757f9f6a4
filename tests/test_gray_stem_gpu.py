"""The one-channel stem kernels (csrc/conv_stem_gray.hip: sf_ncthw1_pack, sf_stem1_fwd, sf_stem1_wgrad) through their
bindings against torch.nn.functional.conv3d in fp64 on the CPU, and engine.stem_conv_bn_relu on one-channel clips.

Bound: 2e-4 max-norm relative, the project's per-kernel figure (tests/test_detection_gpu.py).

Shapes: the smallest that reach each edge of the index math — T = 3 is shorter than the temporal kernel (every output
frame reads zero frames on both sides), T = 6 has interior frames; 20x20 is the even case, 18x26 has an odd Wo = 13 (a
pair whose second position does not exist) and Ho = 9 (a ragged second band of the weight gradient's 8-row bands),
40x12 has Ho = 20: three bands.  (8, 5) / (16, 5) and (64, 1) / (64, 5) are the weight gradient's 1 / 2 / 8
items-per-thread forms; (64, 5) is also the shape whose weights need more than 64 KB of LDS.
The launch plan (stem1_plan) depends on the SIZE of the problem, so those small shapes all run the forward with bands of
2 output rows and the weight gradient with one frame per workgroup.  LAUNCH_CASES are the sizes at which the plan
changes: 8 x 16 x 112 x 112 (the shape training runs) gives the forward its 8-row bands (8 * 16 * ceil(56 / 8) = 896
>= 512 workgroups) and the weight gradient two frames per workgroup (8 clips * 7 bands = 56 -> 10 parts asked, 16 frames
-> 2 per part: the register sum across frames and the re-staging of LDS behind the barrier); 8 x 16 x 40 x 24 sits
between the thresholds (8 rows: 384 < 512 workgroups, 4 rows: 640) and gives 4-row bands; 8 x 8 x 112 x 112 into 64
channels (the Slow stem's kernel) has 4-row bands both ways (the weight gradient's by LDS) and two frames per workgroup."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 2e-4

KERNELS = [(8, 5), (16, 5), (64, 1)]
SIZES = [(20, 20), (18, 26), (40, 12)]
CASES = [(co, kt, t, hw) for co, kt in KERNELS for t in (3, 6) for hw in SIZES] + [(64, 5, 3, (18, 26))]
# (Cout, kT, N, T, (H, W), forward band rows, weight-gradient bands, frames per weight-gradient workgroup)
LAUNCH_CASES = [(8, 5, 8, 16, (112, 112), 8, 7, 2), (16, 5, 8, 16, (40, 24), 4, 3, 1), (64, 1, 8, 8, (112, 112), 4, 14, 2)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _rel(a, b):
    a = np.asarray(a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _problem(co, kt, t, hw, seed, n=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 1, t, hw[0], hw[1], generator=g)
    w = torch.randn(co, 1, kt, 7, 7, generator=g) * (2.0 / (kt * 49)) ** 0.5
    scale = torch.rand(co, generator=g) + 0.5
    bias = torch.randn(co, generator=g) * 0.3
    return x, w, scale, bias


def _conv64(x, w):
    return F.conv3d(x.double(), w.double(), stride=(1, 2, 2), padding=(w.shape[2] // 2, 3, 3))


def _pack(x, dev):
    import sfhip
    from slowfast.models import engine
    conv = torch.nn.Conv3d(1, 8, (5, 7, 7), stride=(1, 2, 2), padding=(2, 3, 3), bias=False)
    ph, pw, wp = engine.stem_geometry(conv, x.shape[3], x.shape[4])
    return sfhip.ncthw1_pack(x.to(dev), ph, pw, wp), (ph, pw, wp)


def _dense(act):
    """NCTHW copy of an Act's channel slice."""
    return act.buf[..., act.coff:act.coff + act.C].permute(0, 4, 1, 2, 3).contiguous().cpu()


@pytest.mark.parametrize("co,kt,t,hw", CASES)
def test_stem1_kernels_match_fp64_conv3d(co, kt, t, hw):
    import sfhip
    dev = _dev()
    idx = CASES.index((co, kt, t, hw))
    x, w, scale, bias = _problem(co, kt, t, hw, 100 + idx)
    buf, (ph, pw, wp) = _pack(x, dev)
    # the layout: the clip in the interior, exact zeros around it
    pc = sfhip.PackedClip(buf, 1, hw[0], hw[1], ph, pw)
    assert torch.equal(pc.to_ncthw().cpu(), x)
    assert float(buf[:, :, :ph].abs().max()) == 0.0 and float(buf[:, :, ph + hw[0]:].abs().max()) == 0.0
    assert float(buf[:, :, :, :pw].abs().max()) == 0.0 and float(buf[:, :, :, pw + hw[1]:].abs().max()) == 0.0
    assert sfhip.stem1_accepts(buf.shape[2], buf.shape[3], co, (kt, 7, 7), (1, 2, 2))
    ref = _conv64(x, w)
    wd = w.to(dev)
    # output views: dense; a 16-byte-aligned slice of a wider buffer; an unaligned one (scalar stores)
    reserve = [(0, 0), (4, 8), (3, 2)][idx % 3]
    z = sfhip.stem1_fwd(buf, wd, kt // 2, out_reserve=reserve)
    assert (z.coff, z.cs) == (reserve[0], co + sum(reserve)) and tuple(z.shape_ncthw) == tuple(ref.shape)
    e_raw = _rel(_dense(z), ref)
    y = sfhip.stem1_fwd(buf, wd, kt // 2, scale=scale.to(dev), bias=bias.to(dev), relu=True,
                        out_reserve=[(4, 8), (3, 2), (0, 0)][idx % 3])
    ref_y = F.relu(ref * scale.double().view(1, -1, 1, 1, 1) + bias.double().view(1, -1, 1, 1, 1))
    e_epi = _rel(_dense(y), ref_y)
    # weight gradient from a dz that lives in a channel slice as well
    g = torch.Generator().manual_seed(900 + idx)
    dz = torch.randn(ref.shape, generator=g)
    dza = sfhip.new_act(dev, *[ref.shape[i] for i in (0, 2, 3, 4)], co, reserve[1], reserve[0])
    dza.buf.normal_()
    dza.buf[..., dza.coff:dza.coff + co] = dz.permute(0, 2, 3, 4, 1).to(dev)
    w64 = w.double().requires_grad_(True)
    (F.conv3d(x.double(), w64, stride=(1, 2, 2), padding=(kt // 2, 3, 3)) * dz.double()).sum().backward()
    dw1 = sfhip.stem1_wgrad(buf, dza, kt, kt // 2)
    dw2 = sfhip.stem1_wgrad(buf, dza, kt, kt // 2)
    acc = torch.ones_like(dw1)
    sfhip.stem1_wgrad(buf, dza, kt, kt // 2, into=acc)
    torch.cuda.synchronize()
    e_dw = _rel(dw1, w64.grad)
    print("stem1 Cout %2d kT %d T %d %dx%d: raw %.3e  scale+bias+relu %.3e  dW %.3e" % (
        co, kt, t, hw[0], hw[1], e_raw, e_epi, e_dw))
    assert e_raw < TOL and e_epi < TOL and e_dw < TOL, (e_raw, e_epi, e_dw)
    assert tuple(dw1.shape) == (co, 1, kt, 7, 7)
    assert torch.equal(dw1, dw2), "two runs of the weight gradient differ"
    assert _rel(acc - 1.0, w64.grad) < TOL  # `into`: accumulated, not overwritten
    # the slices' neighbours were not written
    if reserve != (0, 0):
        fresh = sfhip.new_act(dev, z.N, z.T, z.H, z.W, co, *reserve)
        fresh.buf.fill_(7.0)
        sfhip.stem1_fwd(buf, wd, kt // 2, out=fresh)
        assert float((fresh.buf[..., :reserve[0]] - 7.0).abs().max() if reserve[0] else 0.0) == 0.0
        assert float((fresh.buf[..., reserve[0] + co:] - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize("co,kt,n,t,hw,bh,wbands,fpw", LAUNCH_CASES)
def test_stem1_kernels_at_the_sizes_that_change_the_launch_plan(co, kt, n, t, hw, bh, wbands, fpw):
    """Forward (raw and with the epilogue) and weight gradient against fp64 where the forward's bands are 8 / 4 output
    rows and a weight-gradient workgroup owns more than one frame."""
    import sfhip
    dev = _dev()
    x, w, scale, bias = _problem(co, kt, t, hw, 500 + co + hw[0], n=n)
    buf, _ = _pack(x, dev)
    ho = hw[0] // 2
    # the plan these sizes are here for (csrc/conv_stem_gray.hip, stem1_plan): forward bands halve while the grid is
    # under 512 workgroups; the weight gradient's workspace holds one [Cout][kT*49] partial per workgroup
    rows = 8
    while rows > 2 and n * t * -(-ho // rows) < 512:
        rows //= 2
    assert rows == bh, (rows, bh)
    ws = sfhip.lib().sf_stem1_wgrad_ws_floats(n, t, buf.shape[2], buf.shape[3], co, kt, kt // 2)
    wgs = n * wbands * (t // fpw)
    assert ws == wgs * co * kt * 49, (ws, wgs)
    w64 = w.double().requires_grad_(True)
    ref64 = F.conv3d(x.double(), w64, stride=(1, 2, 2), padding=(kt // 2, 3, 3))  # once: forward and gradient
    ref = ref64.detach()
    wd = w.to(dev)
    z = sfhip.stem1_fwd(buf, wd, kt // 2)
    y = sfhip.stem1_fwd(buf, wd, kt // 2, scale=scale.to(dev), bias=bias.to(dev), relu=True, out_reserve=(4, 4))
    e_raw = _rel(_dense(z), ref)
    e_epi = _rel(_dense(y), F.relu(ref * scale.double().view(1, -1, 1, 1, 1) + bias.double().view(1, -1, 1, 1, 1)))
    g = torch.Generator().manual_seed(77)
    dz = torch.randn(ref.shape, generator=g)
    (ref64 * dz.double()).sum().backward()
    dza = sfhip.Act(dz.permute(0, 2, 3, 4, 1).contiguous().to(dev))
    dw1 = sfhip.stem1_wgrad(buf, dza, kt, kt // 2)
    dw2 = sfhip.stem1_wgrad(buf, dza, kt, kt // 2)
    torch.cuda.synchronize()
    e_dw = _rel(dw1, w64.grad)
    print("stem1 launch plan Cout %2d kT %d N %d T %2d %dx%d (bands of %d rows, %d wgrad workgroups): raw %.3e  "
          "scale+bias+relu %.3e  dW %.3e" % (co, kt, n, t, hw[0], hw[1], bh, wgs, e_raw, e_epi, e_dw))
    assert e_raw < TOL and e_epi < TOL and e_dw < TOL, (e_raw, e_epi, e_dw)
    assert torch.equal(dw1, dw2), "two runs of the weight gradient differ"


def _bn(co, seed, dev):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm3d(co)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(co, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(co, generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn(co, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(co, generator=g) + 0.5)
    return bn


def test_conv_outside_the_range_keeps_the_padded_route():
    """Cout = 12 is not served by sf_stem1_fwd: engine.stem_conv_bn_relu still answers, through the 4-channel layout —
    from a tensor and from a one-channel PackedClip."""
    import sfhip
    from slowfast.models import engine
    dev = _dev()
    x, w, _, _ = _problem(12, 5, 6, (18, 26), 31)
    conv = torch.nn.Conv3d(1, 12, (5, 7, 7), stride=(1, 2, 2), padding=(2, 3, 3), bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    bn = _bn(12, 32, "cpu").eval()
    ref = F.relu(F.batch_norm(_conv64(x, w), bn.running_mean.double(), bn.running_var.double(), bn.weight.double(),
                              bn.bias.double(), False, 0.0, bn.eps))
    conv, bn = conv.to(dev), bn.to(dev)
    assert not sfhip.stem1_accepts(24, 32, 12, conv.kernel_size, conv.stride)
    with torch.no_grad():
        y = engine.stem_conv_bn_relu(x.to(dev), conv, bn)
        buf, (ph, pw, wp) = _pack(x, dev)
        y2 = engine.stem_conv_bn_relu(sfhip.PackedClip(buf, 1, 18, 26, ph, pw), conv, bn)
    torch.cuda.synchronize()
    assert _rel(_dense(y), ref) < TOL and _rel(_dense(y2), ref) < TOL


@pytest.mark.parametrize("co,kt", [(8, 5), (64, 1)])
def test_stem_conv_bn_relu_train_mode_on_a_one_channel_tensor(co, kt):
    """Train mode: batch-statistics BN + ReLU after the one-channel conv, and conv.weight's gradient from a taped
    backward, against fp64 autograd."""
    import sfhip
    from slowfast.models import engine
    dev = _dev()
    x, w, _, _ = _problem(co, kt, 6, (20, 20), 41 + co)
    conv = torch.nn.Conv3d(1, co, (kt, 7, 7), stride=(1, 2, 2), padding=(kt // 2, 3, 3), bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    bn = _bn(co, 43, "cpu").train()
    w64 = w.double().requires_grad_(True)
    gam, bet = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
    ref = F.relu(F.batch_norm(F.conv3d(x.double(), w64, stride=(1, 2, 2), padding=(kt // 2, 3, 3)), None, None, gam, bet,
                              True, 0.1, bn.eps))
    g = torch.Generator().manual_seed(44)
    dy = torch.randn(ref.shape, generator=g)
    (ref * dy.double()).sum().backward()
    conv, bn = conv.to(dev), bn.to(dev)
    calls = []
    real = sfhip.stem1_wgrad
    sfhip.stem1_wgrad = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        t = engine.Tape()
        with torch.no_grad(), engine.taping(t):
            y = engine.stem_conv_bn_relu(x.to(dev), conv, bn)
            yv = _dense(y)
            t.grad_of(y).buf.copy_(dy.permute(0, 2, 3, 4, 1).to(dev))
            t.backward()
        torch.cuda.synchronize()
    finally:
        sfhip.stem1_wgrad = real
    assert calls == [1], "the one-channel route did not record its weight gradient"
    errs = [_rel(yv, ref), _rel(t.pgrads[conv.weight], w64.grad), _rel(t.pgrads[bn.weight], gam.grad),
            _rel(t.pgrads[bn.bias], bet.grad)]
    print("stem_conv_bn_relu train Cout %d kT %d: out %.3e dW %.3e dgamma %.3e dbeta %.3e" % ((co, kt) + tuple(errs)))
    assert max(errs) < TOL, errs
    assert tuple(t.pgrads[conv.weight].shape) == tuple(conv.weight.shape)
