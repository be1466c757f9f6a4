"""Action detection on the GPU: the fused RoIAlign + MaxPool2d kernels (forward and backward, with the temporal
average pool in front) against float64 autograd of the restatement in tests/_roi_align_ref.py, ResNetRoIHead alone in
train mode against a float64 torch restatement of the whole head, the dilated 1x3x3 res5 convolution of the AVA
configs, and the three AVA models against the fixtures the reference made (tests/golden/make_golden_detection.py)."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _roi_align_ref import roi_align
from _util import case_inputs, load_case, rel_err, sample_activation, seeded_state_dict

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _boxes(K, N, S, seed):
    """K boxes over N clips in input pixels (frame S x S), on a 1/64 grid: ordinary, partly outside, sub-cell."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for k in range(K):
        kind = k % 3
        if kind == 0:
            x1, y1 = (torch.rand(2, generator=g) * 0.6 * S).tolist()
            w, h = (torch.rand(2, generator=g) * 0.6 * S + 1).tolist()
        elif kind == 1:  # partly outside the frame
            x1, y1 = (torch.rand(2, generator=g) * 1.0 * S - 0.5 * S).tolist()
            w, h = (torch.rand(2, generator=g) * 0.9 * S + 0.2 * S).tolist()
        else:  # smaller than a feature cell (stride 16)
            x1, y1 = (torch.rand(2, generator=g) * 0.9 * S).tolist()
            w, h = (torch.rand(2, generator=g) * 10 + 0.5).tolist()
        rows.append([k % N, x1, y1, x1 + w, y1 + h])
    b = torch.tensor(rows, dtype=torch.float64)
    b[:, 1:] = torch.round(b[:, 1:] * 64) / 64
    return b.float()


def _ref_head_pool(x_ncthw, boxes, R, scale, aligned):
    """AvgPool3d([T,1,1]) -> squeeze -> ROIAlign -> MaxPool2d(R): [N,C,T,H,W] -> [K, C] (float64, differentiable)."""
    m = x_ncthw.to(torch.float64).mean(dim=2)
    r = roi_align(m, boxes, R, scale, 0, aligned)
    return F.max_pool2d(r, R, stride=1).reshape(r.shape[0], r.shape[1])


CASES = [  # (C, H, K, T, aligned)
    (256, 14, 7, 4, True), (2048, 4, 7, 2, False), (37, 14, 64, 1, True), (256, 4, 1, 8, False),
    (37, 4, 7, 3, False), (2048, 14, 64, 2, True), (256, 14, 64, 1, False),
]


@pytest.mark.parametrize("C,H,K,T,aligned", CASES)
def test_roi_align_max_forward_backward_against_float64(C, H, K, T, aligned):
    _need_gpu()
    import sfhip
    torch.manual_seed(C + H + K)
    N, R, scale, S = 2, 7, 1.0 / 16, H * 16
    x = torch.randn(N, T, H, H, C + 8, device="cuda")  # channel slice [3, 3 + C) of a wider buffer
    xa = sfhip.Act(x, 3, C)
    boxes = _boxes(K, N, S, seed=K * 7 + H)
    pooled = sfhip.roi_tpool(xa)
    cat = sfhip.new_act("cuda", K, 1, 1, 1, C + 5)
    piece = cat.slice(2, C)  # output into a channel-offset slice
    arg = sfhip.roi_align_max(pooled, boxes.cuda(), R, scale, aligned, out=piece)
    got = cat.buf.view(K, C + 5)[:, 2:2 + C].cpu()
    xr = x[..., 3:3 + C].permute(0, 4, 1, 2, 3).cpu().double().requires_grad_(True)
    ref = _ref_head_pool(xr, boxes, R, scale, aligned)
    assert rel_err(got.numpy(), ref.detach().numpy()) <= 1e-5
    dy = torch.randn(K, C + 5, device="cuda")
    dyv = sfhip.Act(dy.view(K, 1, 1, 1, C + 5), 2, C)
    ref.backward(dy[:, 2:2 + C].cpu().double())
    gref = xr.grad.permute(0, 2, 3, 4, 1)  # [N,T,H,W,C]
    dx = torch.full((N, T, H, H, C + 4), 0.5, device="cuda")
    dxa = sfhip.Act(dx, 4, C)
    sfhip.roi_align_max_bwd(dyv, arg, boxes.cuda(), R, scale, aligned, dxa, accumulate=True)
    torch.cuda.synchronize()
    assert rel_err(dx[..., 4:].cpu().numpy() - 0.5, gref.numpy()) <= 1e-5
    assert float((dx[..., :4] - 0.5).abs().max()) == 0.0  # nothing outside the slice
    dx2 = torch.full_like(dx, 7.0)
    sfhip.roi_align_max_bwd(dyv, arg, boxes.cuda(), R, scale, aligned, sfhip.Act(dx2, 4, C), accumulate=False)
    assert rel_err(dx2[..., 4:].cpu().numpy(), gref.numpy()) <= 1e-5


def test_roi_backward_is_bitwise_reproducible_and_skips_foreign_batch_indices():
    _need_gpu()
    import sfhip
    torch.manual_seed(5)
    N, T, H, C, K = 2, 4, 14, 256, 64
    x = sfhip.Act(torch.randn(N, T, H, H, C, device="cuda"))
    boxes = _boxes(K, N, H * 16, seed=3)
    boxes[5, 0] = 7.0   # batch index outside [0, N): reads nothing, yields zeros
    boxes[9, 0] = -3.0
    boxes = boxes.cuda()
    pooled = sfhip.roi_tpool(x)
    out = sfhip.new_act("cuda", K, 1, 1, 1, C)
    arg = sfhip.roi_align_max(pooled, boxes, 7, 1.0 / 16, True, out=out)
    assert float(out.buf.view(K, C)[[5, 9]].abs().max()) == 0.0
    dy = sfhip.Act(torch.randn(K, 1, 1, 1, C, device="cuda"))
    grads = []
    for _ in range(2):
        dx = sfhip.Act(torch.empty(N, T, H, H, C, device="cuda"))
        sfhip.roi_align_max_bwd(dy, arg, boxes, 7, 1.0 / 16, True, dx, accumulate=False)
        grads.append(dx.buf.cpu())
    assert torch.equal(grads[0], grads[1])
    keep = [k for k in range(K) if k not in (5, 9)]
    dy2 = dy.buf.clone()
    dy2[[5, 9]] = 0  # the foreign boxes contribute nothing
    dx = sfhip.Act(torch.empty(N, T, H, H, C, device="cuda"))
    sfhip.roi_align_max_bwd(sfhip.Act(dy2), arg, boxes, 7, 1.0 / 16, True, dx, accumulate=False)
    assert torch.equal(dx.buf.cpu(), grads[0]) and len(keep) == K - 2


def _head(dim_in, T, classes=80, dropout=0.0, aligned=True):
    from slowfast.models.head_helper import ResNetRoIHead
    torch.manual_seed(1)
    return ResNetRoIHead(dim_in=dim_in, num_classes=classes, pool_size=[[t, 1, 1] for t in T],
                         resolution=[[7, 7]] * len(dim_in), scale_factor=[16] * len(dim_in), dropout_rate=dropout,
                         act_func="sigmoid", aligned=aligned).cuda()


def test_head_eval_without_boxes_returns_empty():
    _need_gpu()
    head = _head([256, 32], [2, 8]).eval()
    xs = [torch.randn(2, 256, 2, 4, 4, device="cuda"), torch.randn(2, 32, 8, 4, 4, device="cuda")]
    with torch.no_grad():
        out = head(xs, torch.zeros(0, 5, device="cuda"))
    assert tuple(out.shape) == (0, 80)


@pytest.mark.parametrize("aligned", [True, False])
def test_head_train_mode_against_float64(aligned):
    """ResNetRoIHead alone on seeded res5-shaped inputs (slow [2, 2048, 4, 14, 14], fast [2, 256, 16, 14, 14]), taped:
    probabilities, dL/d(inputs) and dL/dW / dL/db against float64 autograd of the whole head."""
    _need_gpu()
    from slowfast.models import engine
    import sfhip
    head = _head([2048, 256], [4, 16], aligned=aligned).train()
    torch.manual_seed(2)
    xs = [torch.randn(2, 2048, 4, 14, 14, device="cuda"), torch.randn(2, 256, 16, 14, 14, device="cuda")]
    boxes = _boxes(9, 2, 224, seed=11)
    acts = [sfhip.from_ncthw(x) for x in xs]
    t = engine.Tape()
    with engine.taping(t), engine.internal():
        out = head(acts, boxes.cuda())
    dout = torch.randn_like(out)
    with torch.no_grad(), engine.taping(None):
        g = t.grad_of(t.out_act)
        g.buf.copy_(dout.reshape(g.buf.shape))
        t.backward()
    xr = [x.cpu().double().requires_grad_(True) for x in xs]
    W = head.projection.weight.detach().cpu().double().requires_grad_(True)
    b = head.projection.bias.detach().cpu().double().requires_grad_(True)
    feats = torch.cat([_ref_head_pool(x, boxes, 7, 1.0 / 16, aligned) for x in xr], dim=1)
    ref = torch.sigmoid(feats @ W.t() + b)
    ref.backward(dout.cpu().double())
    assert rel_err(out.detach().cpu().numpy(), ref.detach().numpy()) <= 1e-4
    pg = t.pgrads
    assert rel_err(pg[head.projection.weight].cpu().numpy(), W.grad.numpy()) <= 1e-4
    assert rel_err(pg[head.projection.bias].cpu().numpy(), b.grad.numpy()) <= 1e-4


def test_head_input_gradients_against_float64():
    _need_gpu()
    from slowfast.models import engine
    import sfhip
    head = _head([2048, 256], [4, 16]).train()
    torch.manual_seed(3)
    xs = [torch.randn(2, 2048, 4, 14, 14, device="cuda"), torch.randn(2, 256, 16, 14, 14, device="cuda")]
    boxes = _boxes(9, 2, 224, seed=12)
    acts = [sfhip.from_ncthw(x) for x in xs]
    seen = {}
    t = engine.Tape()
    with engine.taping(t), engine.internal():
        out = head(acts, boxes.cuda())
    dout = torch.randn_like(out)
    orig = t.backward

    def backward():  # keep the gradient buffers the tape frees at the end of its replay
        orig_reset = t.gbuf
        orig()
        seen.update(orig_reset)
    t.backward = backward
    with torch.no_grad(), engine.taping(None):
        g = t.grad_of(t.out_act)
        g.buf.copy_(dout.reshape(g.buf.shape))
        t.backward()
    xr = [x.cpu().double().requires_grad_(True) for x in xs]
    W = head.projection.weight.detach().cpu().double()
    b = head.projection.bias.detach().cpu().double()
    feats = torch.cat([_ref_head_pool(x, boxes, 7, 1.0 / 16, True) for x in xr], dim=1)
    torch.sigmoid(feats @ W.t() + b).backward(dout.cpu().double())
    for a, x in zip(acts, xr):
        gb = seen[a.buf.data_ptr()].view(a.buf.shape)
        got = gb.permute(0, 4, 1, 2, 3).cpu()
        assert rel_err(got.numpy(), x.grad.numpy()) <= 1e-4


@pytest.mark.parametrize("shape", [(2, 8, 14, 14, 512), (2, 32, 14, 14, 64)])
def test_dilated_res5_conv_against_float64(shape):
    """res5's 1x3x3 convolution of the AVA configs: dilation 2, padding 2, stride 1 at 14 x 14 (224^2 input), through
    the planner's routes for the forward, the data gradient and the weight gradient."""
    _need_gpu()
    from slowfast.models import engine
    import sfhip
    N, T, H, W, C = shape
    torch.manual_seed(C)
    conv = torch.nn.Conv3d(C, C, (1, 3, 3), stride=1, padding=(0, 2, 2), dilation=(1, 2, 2), bias=False).cuda()
    x = torch.randn(N, C, T, H, W, device="cuda")
    xa = sfhip.from_ncthw(x)
    seen = {}
    t = engine.Tape()
    with engine.taping(t), engine.internal():
        y = engine.conv_bn_act(xa, conv)
    dy = torch.randn(y.buf.shape, device="cuda")
    orig = t.backward

    def backward():
        keep = t.gbuf
        orig()
        seen.update(keep)
    t.backward = backward
    t.out_act = y
    with torch.no_grad(), engine.taping(None):
        t.grad_of(y).buf.copy_(dy)
        t.backward()
    torch.cuda.synchronize()
    xr = x.cpu().double().requires_grad_(True)
    wr = conv.weight.detach().cpu().double().requires_grad_(True)
    yr = F.conv3d(xr, wr, None, 1, (0, 2, 2), (1, 2, 2))
    yr.backward(dy.cpu().double().permute(0, 4, 1, 2, 3))
    assert rel_err(sfhip.to_ncthw(y).cpu().numpy(), yr.detach().numpy()) <= 2e-4
    gx = seen[xa.buf.data_ptr()].view(xa.buf.shape).permute(0, 4, 1, 2, 3).cpu()
    assert rel_err(gx.numpy(), xr.grad.numpy()) <= 2e-4
    assert rel_err(t.pgrads[conv.weight].cpu().numpy(), wr.grad.numpy()) <= 2e-4


DET_CASES = ["slowfast_r50_ava_s64", "slow_r50_ava_s64", "dual_r50_ava_s64"]


def _build(meta, z):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 1
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    sd = seeded_state_dict(z["sd_keys"], z["sd_shapes"], meta["param_seed"])
    r = model.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    return model


@pytest.mark.parametrize("name", DET_CASES)
def test_detection_model_matches_reference_golden(name):
    """test_net.py / train_net.py:71-96 with boxes: eval probabilities, train-mode BCE loss and sampled parameter
    gradients against the reference's own run (end-to-end bounds of test_models_gpu.py)."""
    _need_gpu()
    z, meta = load_case(name)
    model = _build(meta, z).eval()
    boxes = torch.from_numpy(z["boxes"]).cuda()
    xs = [x.cuda() for x in case_inputs(meta)]
    with torch.no_grad():
        probs = model(xs, boxes)
    assert rel_err(probs.cpu().numpy(), z["eval/out"]) <= 1e-3
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.train()
    p = model(xs, boxes)
    loss = torch.nn.BCELoss()(p, torch.from_numpy(z["labels"]).cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert rel_err(p.detach().cpu().numpy(), z["train/out"]) <= 1e-3
    assert abs(loss.item() - float(z["train/loss"][0])) < 1e-3
    params = dict(model.named_parameters())
    keys = [k[5:] for k in z.files if k.startswith("grad/") and not k.endswith("/stats")]
    assert len(keys) >= 5
    for k in keys:
        g = params[k].grad
        s, _, _ = sample_activation(g.cpu().numpy(), 4096)
        ref = z["grad/" + k].astype(np.float64)
        e = float(np.linalg.norm(s.astype(np.float64) - ref) / max(np.linalg.norm(ref), 1e-30))
        assert e < (0.3 if g.numel() < 16 else 8e-2), (k, e)
        if g.numel() >= 16:
            norm, rnorm = float(g.norm()), float(z["grad/" + k + "/stats"][1])
            assert abs(norm - rnorm) < 5e-2 * rnorm + 1e-9, (k, norm, rnorm)
    missing = [k for k, q in model.named_parameters() if q.grad is None]
    assert not missing, missing[:5]
