"""CMDA's two attention halves as parameter containers (reference wdf_attention_helper.py:13-91).
They are executed by FuseFastAndSlow as fused kernels; called on their own (NCTHW tensor in/out) they run
the same kernels un-fused.

ChannelAttention and ContextBlock3D (reference :97-124, :289-379) are the fork's swap-in alternatives for the CMDA
halves and for stage-level context: same constructors, attributes and state_dict keys, forward on an NCTHW tensor or
an Act (the same kind comes back), on the kernels of csrc/ctx_pool.hip.  The file's remaining two classes,
NonLocalBlock and Stripe_NonLocalBlock, are out of scope: no model instantiates them."""
import torch
import torch.nn as nn

import sfhip
from . import engine


class SpatialAttention(nn.Module):
    """Full softmax self-attention over N = T*H*W positions, no 1/sqrt(d) scaling, q/k/v 1x1x1 convs with
    bias, out = gamma * attn(x) + x with gamma initialised to 0 (wdf_attention_helper.py:17-54)."""

    def __init__(self, channel, reduction=8):
        super(SpatialAttention, self).__init__()
        self.input_channel = channel
        self.query_conv = nn.Conv3d(in_channels=channel, out_channels=channel // reduction, kernel_size=1)
        self.key_conv = nn.Conv3d(in_channels=channel, out_channels=channel // reduction, kernel_size=1)
        self.value_conv = nn.Conv3d(in_channels=channel, out_channels=channel, kernel_size=1)
        self.gamma = nn.Parameter(torch.zeros(1))
        self.softmax = nn.Softmax(dim=-1)

    def qkv(self, x):
        """One pointwise GEMM producing [q | k | v] rows: [N,T,H,W, 3*C].  With reduction r > 1 (the reference class's
        default is 8; no shipped model uses it) q and k have C/r channels: their rows of the merged weight are padded
        with ZERO rows up to C, so the padded channels of q / k are exactly zero, q k^T is unchanged and the flash
        kernels run as for r = 1 (correct, not tuned: the score product is taken over C instead of C/r channels)."""
        c = self.input_channel
        cr = self.query_conv.out_channels
        convs = (self.query_conv, self.key_conv, self.value_conv)

        def padded(t, rows):
            if t.shape[0] == rows:
                return t
            return torch.cat([t, t.new_zeros((rows - t.shape[0],) + tuple(t.shape[1:]))], 0)

        def make():  # (forward pack, bias, data-gradient pack) of the merged projection, once per parameter version
            w = torch.cat([padded(cv.weight, c) for cv in convs], 0)
            b = torch.cat([padded(cv.bias, c) for cv in convs], 0)
            if w.is_cuda:  # both layouts by one launch
                wp_, wtp_ = sfhip.pack_conv_weight_pair(w.detach())
                return wp_, b.contiguous(), wtp_
            return sfhip.pack_conv_weight(w), b.contiguous(), None

        wp, b, wtp = engine._cached(self, "_sf_qkv", engine._key(*[t for cv in convs for t in (cv.weight, cv.bias)]),
                                    make)
        qkv = sfhip.conv(x, wp, (1, 1, 1), bias=b)
        t = engine.tape()
        if t is not None:
            nout = (cr, cr, c)

            def bwd():  # merged q|k|v projection: one wgrad / dgrad, then split per conv
                g = t.grad_of(qkv)
                if t.param_grads:
                    dwp = sfhip.conv_wgrad(x, g, 3 * c, (1, 1, 1), cin_pad=wp.shape[2])
                    dw = sfhip.unpack_conv_weight_grad(dwp, (3 * c, c, 1, 1, 1))
                    db = engine._colsum(g)
                    t.add_pgrads([cv.weight for cv in convs] + [cv.bias for cv in convs],
                                 [dw[i * c:i * c + nout[i]] for i in range(3)] +
                                 [db[i * c:i * c + nout[i]] for i in range(3)])
                sfhip.conv_dgrad(g, wtp, x, (1, 1, 1), out=t.grad_of(x), accumulate=True)

            t.record(bwd)
        return qkv

    def _run_wide(self, x, scale, bias, relu, alpha, out):
        """Heads wider than the flash kernels' 128 channels (SlowFastShuffleNet w2.0 / g3: C = 240 at s4_fuse, where
        N = T*H*W <= 64): three dense 1x1x1 projections and the attention of the Nonlocal block
        (nonlocal_helper.dense_attention with sm_scale = 1, i.e. no 1/sqrt(d): the streaming cross-length kernels of
        attn_cross.hip, no score matrix in memory), then z = gamma * O + x (and the eval-mode BN affine / ReLU /
        nearest T-upsample as one more small pass)."""
        from .nonlocal_helper import dense_attention
        c = self.input_channel
        q = engine.conv_bn_act(x, self.query_conv)
        k = engine.conv_bn_act(x, self.key_conv)
        v = engine.conv_bn_act(x, self.value_conv)
        o = dense_attention(q, k, v, softmax=True, sm_scale=1.0)
        gvec = self.gamma.detach().expand(c).contiguous()
        zero = torch.zeros_like(gvec)  # sf_affine_fwd takes scale and bias together
        t = engine.tape()
        if t is None:
            plain = scale is None and bias is None and not relu and alpha == 1
            z = sfhip.affine(o, scale=gvec, bias=zero, res=x, out=out if plain else None)
            return z if plain else sfhip.affine(z, scale=scale, bias=bias, relu=relu, rep=alpha, out=out)
        assert scale is None and not relu and alpha == 1 and out is None, "taped attention runs un-fused"
        z = sfhip.affine(o, scale=gvec, bias=zero, res=x)

        def bwd():  # z's buffer holds dL/dz (the BN backward wrote it in place), as in run()
            gz = z if getattr(bwd, "grad_in_place", True) else t.grad_of(z)
            if t.param_grads:
                t.add_pgrad(self.gamma, sfhip.rowdot(gz, o).sum().reshape(1))
            sfhip.affine(gz, scale=self.gamma.detach().expand(c).contiguous(), bias=zero, out=t.grad_of(o))  # dO = gamma * dz
            sfhip.axpy(gz, t.grad_of(x), 1.0, accumulate=True)                                     # residual

        t.record(bwd)
        return z

    def run(self, x, scale=None, bias=None, relu=False, alpha=1, out=None):
        c = self.input_channel
        if c > 128:
            return self._run_wide(x, scale, bias, relu, alpha, out)
        qkv = self.qkv(x)
        t = engine.tape()
        save = {} if t is not None else None
        q, k, v = qkv.slice(0, c), qkv.slice(c, c), qkv.slice(2 * c, c)
        z = sfhip.attention(q, k, v, x, self.gamma, scale=scale, bias=bias, relu=relu, alpha=alpha, out=out,
                            save=save)
        if t is not None:
            assert scale is None and not relu and alpha == 1, "taped attention runs un-fused (training-mode BN)"

            def bwd():  # z's grad buffer = the BN backward's in-place dz when z fed a BN, else grad_of(z)
                gz = z if getattr(bwd, "grad_in_place", True) else t.grad_of(z)
                dq = t.grad_of(qkv)
                dvec = sfhip.attention_bwd(q, k, v, gz, save["o"], save["lse"], self.gamma, dq.slice(0, c),
                                           dq.slice(c, c), dq.slice(2 * c, c))
                if t.param_grads:
                    t.add_pgrad(self.gamma, dvec.sum().reshape(1))
                sfhip.axpy(gz, t.grad_of(x), 1.0, accumulate=True)  # residual: z = gamma*O + x

            t.record(bwd)
        return z

    def forward(self, x):
        plain = not isinstance(x, engine.Act)
        a = engine.enter([x])[0]
        y = self.run(a)
        return sfhip.to_ncthw(y) if plain else y


class ECA(nn.Module):
    """Efficient channel attention: global avg-pool -> Conv1d(1,1,k=3,pad=1,bias=False) ALONG THE CHANNEL
    AXIS -> sigmoid -> broadcast multiply (wdf_attention_helper.py:57-91)."""

    def __init__(self, channel, k_size=3):
        super(ECA, self).__init__()
        if k_size != 3:
            raise NotImplementedError("ECA k_size != 3 is never used by the reference models")
        self.avg_pool = nn.AdaptiveAvgPool3d(1)
        self.conv = nn.Conv1d(1, 1, kernel_size=k_size, padding=(k_size - 1) // 2, bias=False)
        self.sigmoid = nn.Sigmoid()

    def run(self, x, alpha=1, scale=None, bias=None, relu=False, out=None):
        """gate(max-pool_alpha(x)) [* BN affine, ReLU], written into `out`."""
        pooled = sfhip.tmax_mean(x, alpha)
        z = sfhip.gate_apply(x, alpha, pooled, w3=self.conv.weight, scale=scale, bias=bias, relu=relu, out=out)
        t = engine.tape()
        if t is not None:
            assert scale is None and not relu, "taped ECA runs un-fused (training-mode BN follows)"
            w3 = self.conv.weight

            def bwd():  # z's buffer holds dL/dz (BN backward wrote it in place)
                dg = sfhip.tmax_dot(x, alpha, z)                       # [N, C] = sum dz * max_r x
                count = float((x.T // alpha) * x.H * x.W)
                tgt = t.pgrad_target(w3)
                dw = tgt if tgt is not None else torch.zeros(3, dtype=torch.float32, device=dg.device)
                # the 3-tap gate's derivative on the [N, C] vectors: one small HIP launch (no vendor conv kernels)
                gate, dpool = sfhip.eca_gate_bwd(dg, pooled, w3.detach().contiguous(), 1.0 / count, dw)
                if tgt is None:
                    t.add_pgrad(w3, dw)
                sfhip.eca_bwd_apply(x, alpha, z, gate, dpool, t.grad_of(x))

            t.record(bwd)
        return z

    def forward(self, x):
        plain = not isinstance(x, engine.Act)
        a = engine.enter([x])[0]
        y = self.run(a)
        return sfhip.to_ncthw(y) if plain else y


def _vec(a):
    """The [N, C] matrix an [N, 1, 1, 1, C] Act views."""
    return a.buf.view(a.N, a.cs)[:, a.coff:a.coff + a.C]


def _same_kind(mod, x, reserve):
    """forward of the two blocks below: an NCTHW tensor gives an NCTHW tensor, an Act gives an Act (allocated with
    `reserve` = (before, after) channels of room around it, as Nonlocal.forward's: a CMDA fusion behind the block
    concatenates in place)."""
    plain = not isinstance(x, engine.Act)
    (a,) = engine.enter([x])
    with engine.internal():
        y = mod.run(a, reserve)
    return sfhip.to_ncthw(y) if plain else y


class ChannelAttention(nn.Module):
    """RCAN-style channel attention with the fork's residual path: y = AdaptiveAvgPool3d(1)(x) -> Conv3d(C, C/r, 1) ->
    ReLU -> Conv3d(C/r, C, 1) -> Sigmoid, out = x * y + x (wdf_attention_helper.py:97-124; C/r = 2 when C // r is 0).
    Global mean (HIP reduction) -> the two 1x1x1 convs on the [N, C] vector through the library's GEMM kernels -> ONE
    pass x * (1 + sigmoid(e)) (sf_sample_affine_fwd); the sigmoid of the [N, C] vector is a torch op, as SqueezeExcite's
    gate derivative is.  Taped in training, activation gradients only under an EvalTape."""

    def __init__(self, channel, reduction=16):
        super(ChannelAttention, self).__init__()
        self.avg_pool = nn.AdaptiveAvgPool3d(1)
        inner_channel = channel // reduction if channel // reduction != 0 else 2
        self.conv_du = nn.Sequential(
            nn.Conv3d(channel, inner_channel, 1, padding=0, bias=True),
            nn.ReLU(inplace=True),
            nn.Conv3d(inner_channel, channel, 1, padding=0, bias=True),
            nn.Sigmoid(),
        )

    def run(self, x, reserve=(0, 0)):
        pooled = engine.global_mean(x)
        e = engine.conv_bn_act(engine.conv_bn_act(pooled, self.conv_du[0], relu=True), self.conv_du[2])
        gate = torch.sigmoid(_vec(e))
        mul = (gate + 1.0).contiguous()
        y = sfhip.sample_affine(x, mul=mul, out=sfhip.new_act(x, x.N, x.T, x.H, x.W, x.C, reserve[0], reserve[1]))
        t = engine.tape()
        if t is not None:
            def bwd():  # dx (+)= dy * (1 + gate) and sum_pos dy * x in one pass over dy and x
                fresh = t.grad_of_uninitialised(x)
                dmul, _ = sfhip.sample_affine_bwd(t.grad_of(y), fresh if fresh is not None else t.grad_of(x), x=x,
                                                  mul=mul, accumulate=fresh is None, want_dmul=True)
                de = (dmul * gate * (1.0 - gate)).contiguous()
                sfhip.axpy(sfhip.Act(de.view(x.N, 1, 1, 1, x.C)), t.grad_of(e), 1.0, accumulate=True)

            t.record(bwd)
        return y

    def forward(self, x, reserve=(0, 0)):
        return _same_kind(self, x, reserve)


class ContextBlock3D(nn.Module):
    """GCNet global-context block (wdf_attention_helper.py:289-379): context = attention pooling ('att': softmax over
    the T*H*W positions of a 1-channel 1x1x1 conv, sf_ctx_pool_fwd — one pass over x, the logits never stored) or the
    global mean ('avg'); out = x + channel_add_conv(context), the add broadcast in ONE pass (sf_sample_affine_fwd).
    The [N, planes] branch conv -> LayerNorm([planes, 1, 1, 1]) -> ReLU -> conv is vector-sized: the convs run on the
    library's GEMM kernels, the LayerNorm + ReLU between them (and their backward) are torch ops on [N, planes].
    'channel_mul': the reference builds nn.LayerNorm([planes, 1, 1]) for a [N, planes, 1, 1, 1] context, which
    PyTorch rejects unless planes == 1 — the constructor and the state_dict keys are kept, forward raises
    NotImplementedError.  NonLocalBlock and Stripe_NonLocalBlock of the same reference file are out of scope (never
    instantiated by any model)."""

    def __init__(self, inplanes, ratio=1., pooling_type='att', fusion_types=('channel_add',)):
        super(ContextBlock3D, self).__init__()
        assert pooling_type in ['avg', 'att']
        assert isinstance(fusion_types, (list, tuple))
        valid_fusion_types = ['channel_add', 'channel_mul']
        assert all([f in valid_fusion_types for f in fusion_types])
        assert len(fusion_types) > 0, 'at least one fusion should be used'
        self.inplanes = inplanes
        self.ratio = ratio
        self.planes = int(inplanes * ratio)
        self.pooling_type = pooling_type
        self.fusion_types = fusion_types
        if pooling_type == 'att':
            self.conv_mask = nn.Conv3d(inplanes, 1, kernel_size=1)
            self.softmax = nn.Softmax(dim=2)
        else:
            self.avg_pool = nn.AdaptiveAvgPool3d(1)
        if 'channel_add' in fusion_types:
            self.channel_add_conv = nn.Sequential(
                nn.Conv3d(self.inplanes, self.planes, kernel_size=1),
                nn.LayerNorm([self.planes, 1, 1, 1]),
                nn.ReLU(inplace=True),
                nn.Conv3d(self.planes, self.inplanes, kernel_size=1))
        else:
            self.channel_add_conv = None
        if 'channel_mul' in fusion_types:
            self.channel_mul_conv = nn.Sequential(
                nn.Conv3d(self.inplanes, self.planes, kernel_size=1),
                nn.LayerNorm([self.planes, 1, 1]),
                nn.ReLU(inplace=True),
                nn.Conv3d(self.planes, self.inplanes, kernel_size=1))
        else:
            self.channel_mul_conv = None
        self.reset_parameters()

    def reset_parameters(self):
        """mmcv's kaiming_init(conv_mask, mode='fan_in') (normal, ReLU gain, bias 0) and constant_init(last conv, 0):
        a fresh block is the identity."""
        if self.pooling_type == 'att':
            nn.init.kaiming_normal_(self.conv_mask.weight, a=0, mode='fan_in', nonlinearity='relu')
            nn.init.constant_(self.conv_mask.bias, 0)
            self.conv_mask.inited = True
        for seq in (self.channel_add_conv, self.channel_mul_conv):
            if seq is not None:
                nn.init.constant_(seq[-1].weight, 0)
                nn.init.constant_(seq[-1].bias, 0)

    def spatial_pool(self, x):
        """The context of the view x as an [N, 1, 1, 1, C] Act (taped)."""
        if self.pooling_type != 'att':
            return engine.global_mean(x)
        w, b = self.conv_mask.weight, self.conv_mask.bias
        ctx, lse = sfhip.ctx_pool(x, w.detach(), b.detach())
        context = sfhip.Act(ctx.view(x.N, 1, 1, 1, x.C))
        t = engine.tape()
        if t is not None:
            def bwd():  # one pass: l recomputed, dx (+)= p * dctx + dl * w, dw from per-workgroup partials
                dctx = t.grad_of(context).buf.view(x.N, x.C)
                fresh = t.grad_of_uninitialised(x)
                dx = fresh if fresh is not None else t.grad_of(x)
                if not t.param_grads:
                    sfhip.ctx_pool_bwd(x, w.detach(), b.detach(), lse, ctx, dctx, dx, accumulate=fresh is None,
                                       want_dw=False)
                    return
                tgt = t.pgrad_target(w)
                if tgt is not None:  # the finish kernel accumulates into the parameter's gradient
                    sfhip.ctx_pool_bwd(x, w.detach(), b.detach(), lse, ctx, dctx, dx, accumulate=fresh is None,
                                       dw=tgt, dw_accumulate=True)
                    if t.pgrad_target(b) is None:
                        t.add_pgrad(b, torch.zeros_like(b))
                    return
                db = torch.empty_like(b)
                dw = sfhip.ctx_pool_bwd(x, w.detach(), b.detach(), lse, ctx, dctx, dx, accumulate=fresh is None, db=db)
                t.add_pgrad(w, dw)
                t.add_pgrad(b, db)

            t.record(bwd)
        return context

    def run(self, x, reserve=(0, 0)):
        if self.channel_mul_conv is not None:
            raise NotImplementedError(
                "ContextBlock3D 'channel_mul': the reference builds nn.LayerNorm([planes, 1, 1]) for a "
                "[N, planes, 1, 1, 1] context, which PyTorch itself rejects unless planes == 1 — there is no defined "
                "result to reproduce; use fusion_types=('channel_add',)")
        context = self.spatial_pool(x)
        seq = self.channel_add_conv
        ln, planes = seq[1], self.planes
        h = engine.conv_bn_act(context, seq[0])
        h = engine.small_torch_op(
            [h], [ln.weight, ln.bias],
            lambda v: torch.relu(torch.nn.functional.layer_norm(v[0], (planes,), ln.weight.reshape(-1),
                                                               ln.bias.reshape(-1), ln.eps)))
        term = engine.conv_bn_act(h, seq[3])
        add = _vec(term).contiguous()
        y = sfhip.sample_affine(x, add=add, out=sfhip.new_act(x, x.N, x.T, x.H, x.W, x.C, reserve[0], reserve[1]))
        t = engine.tape()
        if t is not None:
            def bwd():  # dx (+)= dy and sum_pos dy in one pass over dy
                fresh = t.grad_of_uninitialised(x)
                _, dadd = sfhip.sample_affine_bwd(t.grad_of(y), fresh if fresh is not None else t.grad_of(x),
                                                  accumulate=fresh is None, want_dadd=True)
                sfhip.axpy(sfhip.Act(dadd.view(x.N, 1, 1, 1, x.C)), t.grad_of(term), 1.0, accumulate=True)

            t.record(bwd)
        return y

    def forward(self, x, reserve=(0, 0)):
        if self.channel_mul_conv is not None:
            return self.run(x)  # raises before any tensor is touched
        return _same_kind(self, x, reserve)
