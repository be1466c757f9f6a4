"""CMDA's two attention halves as parameter containers (reference wdf_attention_helper.py:13-91).
They are executed by FuseFastAndSlow as fused kernels; called on their own (NCTHW tensor in/out) they run
the same kernels un-fused.

ChannelAttention and ContextBlock3D (reference :97-124, :289-379) are the fork's swap-in alternatives for the CMDA
halves and for stage-level context: same constructors, attributes and state_dict keys, forward on an NCTHW tensor or
an Act (the same kind comes back), on the kernels of csrc/ctx_pool.hip.

NonLocalBlock and Stripe_NonLocalBlock (reference :129-195, :198-273) complete the file: the same constructors,
attributes and state_dict keys, NCTHW tensor or Act in and the same kind out.  Their convs, max-pool and attention run
on the kernels Nonlocal uses (engine.conv_bn_act, engine.maxpool, nonlocal_helper.dense_attention — with the scale rules
of THIS file: softmax without 1/sqrt(d), 'dot' divided by the query count); the stripe pooling and the per-stripe
broadcast add of Stripe_NonLocalBlock are the kernels of csrc/stripe_pool.hip.  Both are taped for training."""
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
                dx, acc = t.grad_dst(x)
                dmul, _ = sfhip.sample_affine_bwd(t.grad_of(y), dx, x=x, mul=mul, accumulate=acc, want_dmul=True)
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
    NotImplementedError."""

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
                dx, acc = t.grad_dst(x)
                if not t.param_grads:
                    sfhip.ctx_pool_bwd(x, w.detach(), b.detach(), lse, ctx, dctx, dx, accumulate=acc, want_dw=False)
                    return
                tgt = t.pgrad_target(w)
                if tgt is not None:  # the finish kernel accumulates into the parameter's gradient
                    sfhip.ctx_pool_bwd(x, w.detach(), b.detach(), lse, ctx, dctx, dx, accumulate=acc, dw=tgt,
                                       dw_accumulate=True)
                    if t.pgrad_target(b) is None:
                        t.add_pgrad(b, torch.zeros_like(b))
                    return
                db = torch.empty_like(b)
                dw = sfhip.ctx_pool_bwd(x, w.detach(), b.detach(), lse, ctx, dctx, dx, accumulate=acc, db=db)
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
                dx, acc = t.grad_dst(x)
                _, dadd = sfhip.sample_affine_bwd(t.grad_of(y), dx, accumulate=acc, want_dadd=True)
                sfhip.axpy(sfhip.Act(dadd.view(x.N, 1, 1, 1, x.C)), t.grad_of(term), 1.0, accumulate=True)

            t.record(bwd)
        return y

    def forward(self, x, reserve=(0, 0)):
        if self.channel_mul_conv is not None:
            return self.run(x)  # raises before any tensor is touched
        return _same_kind(self, x, reserve)


def _block_attention(theta, phi, g, instance):
    """f = theta phi^T; 'soft': softmax(f) g (no 1/sqrt(d)); 'dot': (f / f.shape[1]) g — f.shape[1] is the QUERY count
    (wdf_attention_helper.py:185-190, :260-265), not Nonlocal's key count.  Through nonlocal_helper.dense_attention;
    a key width none of its kernels takes raises — nothing here runs on torch."""
    from .nonlocal_helper import dense_attention
    soft = instance == 'soft'
    if instance not in ('soft', 'dot'):
        raise NotImplementedError("instance %r: the reference defines 'soft' and 'dot'" % (instance,))
    taken = sfhip.xattn_accepts(theta, phi, g) if soft else sfhip.assoc_accepts(theta, phi, g)
    if not taken and theta.C % 16 != 0:
        raise NotImplementedError(
            "no attention kernel takes a key width of %d (the streaming / associative kernels and the materialised "
            "path, which needs a multiple of 16, all refuse): choose inter_channels as a multiple of 4" % theta.C)
    nq = theta.T * theta.H * theta.W
    return dense_attention(theta, phi, g, softmax=soft, sm_scale=1.0, dot_scale=1.0 / nq)


def _refuse_eval_tape(name):
    if isinstance(engine.tape(), engine.EvalTape):
        raise NotImplementedError("Grad-CAM (the eval-mode tape) does not cover %s" % name)


class NonLocalBlock(nn.Module):
    """The fork's small non-local block (wdf_attention_helper.py:129-195, after STE-NVAN): theta / phi / g 1x1x1 convs,
    f = theta phi^T over all T*H*W positions, softmax ('soft') or f / N_q ('dot'), y = f g, z = W(y) + x with W a conv +
    zero-initialised BatchNorm3d (bn_layer) or a zero-initialised conv.  sub_sample wraps g and phi in
    nn.Sequential(conv, MaxPool3d((1, 2, 2))) (keys g.0.* / phi.0.*): the keys and values are max-pooled (odd H / W
    floored), so N_q = 4 N_k.  Convs through engine.conv_bn_act, the pool through engine.maxpool, the attention through
    nonlocal_helper.dense_attention (streaming softmax / associative dot product), the residual in W's epilogue.  Taped
    for training; the eval-mode tape raises, as Nonlocal's does."""

    def __init__(self, in_channels, inter_channels=None, sub_sample=False, bn_layer=True, instance='soft'):
        super(NonLocalBlock, self).__init__()
        self.sub_sample = sub_sample
        self.instance = instance
        self.in_channels = in_channels
        self.inter_channels = inter_channels
        if self.inter_channels is None:
            self.inter_channels = in_channels // 2
            if self.inter_channels == 0:
                self.inter_channels = 1
        max_pool_layer = nn.MaxPool3d(kernel_size=(1, 2, 2))
        self.g = nn.Conv3d(self.in_channels, self.inter_channels, kernel_size=1, stride=1, padding=0)
        if bn_layer:
            self.W = nn.Sequential(
                nn.Conv3d(self.inter_channels, self.in_channels, kernel_size=1, stride=1, padding=0),
                nn.BatchNorm3d(self.in_channels))
            nn.init.constant_(self.W[1].weight, 0)
            nn.init.constant_(self.W[1].bias, 0)
        else:
            self.W = nn.Conv3d(self.inter_channels, self.in_channels, kernel_size=1, stride=1, padding=0)
            nn.init.constant_(self.W.weight, 0)
            nn.init.constant_(self.W.bias, 0)
        self.theta = nn.Conv3d(self.in_channels, self.inter_channels, kernel_size=1, stride=1, padding=0)
        self.phi = nn.Conv3d(self.in_channels, self.inter_channels, kernel_size=1, stride=1, padding=0)
        if sub_sample:
            self.g = nn.Sequential(self.g, max_pool_layer)
            self.phi = nn.Sequential(self.phi, max_pool_layer)

    def run(self, x, reserve=(0, 0)):
        _refuse_eval_tape("NonLocalBlock")
        theta = engine.conv_bn_act(x, self.theta)
        if self.sub_sample:  # conv, then the pool: the order of the reference's Sequential
            ks = (1, 2, 2)
            if x.H < 2 or x.W < 2:
                raise ValueError("NonLocalBlock(sub_sample=True) needs H, W >= 2, got %r" % (x,))
            phi = engine.maxpool(engine.conv_bn_act(x, self.phi[0]), ks, ks)
            g = engine.maxpool(engine.conv_bn_act(x, self.g[0]), ks, ks)
        else:
            phi = engine.conv_bn_act(x, self.phi)
            g = engine.conv_bn_act(x, self.g)
        y = _block_attention(theta, phi, g, self.instance)
        if isinstance(self.W, nn.Sequential):
            return engine.conv_bn_act(y, self.W[0], self.W[1], res=x, out_reserve=reserve)
        return engine.conv_bn_act(y, self.W, res=x, out_reserve=reserve)

    def forward(self, x, reserve=(0, 0)):
        return _same_kind(self, x, reserve)


class Stripe_NonLocalBlock(nn.Module):
    """Non-local attention between the horizontal stripes of all frames (wdf_attention_helper.py:198-273): every frame
    is cut into `stripe` bands of H / stripe rows, each band pooled to one vector per channel ('mean', 'max', or
    'meanmax': both, concatenated — the g / theta / phi convs then take 2C channels, the reference's in_channels *= 2),
    the T * stripe vectors of a sample attend to each other ('soft' / 'dot', as NonLocalBlock), W = conv + zero-initialised
    BatchNorm3d (batch statistics over the N * T * stripe vectors), and the result is added to every position of its
    band.  The activation-sized steps are ONE pass each: sf_stripe_pool_fwd (x read once) and sf_stripe_add_fwd; the
    backward is two passes over dL/dz — the 'sum' pool (the gradient of the broadcast) before the small attention's
    backward, and sf_stripe_pool_bwd (residual + pooling gradient into dL/dx) after it.  Taped for training; the
    eval-mode tape raises."""

    def __init__(self, stripe, in_channels, inter_channels=None, pool_type='mean', instance='soft'):
        super(Stripe_NonLocalBlock, self).__init__()
        self.instance = instance
        self.stripe = stripe
        self.in_channels = in_channels
        self.pool_type = pool_type
        if pool_type == 'max':
            self.pool = nn.AdaptiveMaxPool2d(1)
        elif pool_type == 'mean':
            self.pool = nn.AdaptiveAvgPool2d(1)
        elif pool_type == 'meanmax':
            self.avgpool = nn.AdaptiveAvgPool2d(1)
            self.maxpool = nn.AdaptiveMaxPool2d(1)
            self.in_channels *= 2
        if inter_channels is None:
            self.inter_channels = in_channels // 2
        else:
            self.inter_channels = inter_channels
        self.g = nn.Conv3d(self.in_channels, self.inter_channels, kernel_size=1, stride=1, padding=0)
        self.theta = nn.Conv3d(self.in_channels, self.inter_channels, kernel_size=1, stride=1, padding=0)
        self.phi = nn.Conv3d(self.in_channels, self.inter_channels, kernel_size=1, stride=1, padding=0)
        if pool_type == 'meanmax':
            self.in_channels //= 2
        self.W = nn.Sequential(
            nn.Conv3d(self.inter_channels, self.in_channels, kernel_size=1, stride=1, padding=0),
            nn.BatchNorm3d(self.in_channels))
        nn.init.constant_(self.W[1].weight, 0)
        nn.init.constant_(self.W[1].bias, 0)

    def run(self, x, reserve=(0, 0)):
        _refuse_eval_tape("Stripe_NonLocalBlock")
        S, c = self.stripe, self.in_channels
        if self.pool_type not in sfhip.STRIPE_MODES or self.pool_type == 'sum':
            raise NotImplementedError("pool_type %r: the reference defines 'mean', 'max' and 'meanmax'" % (self.pool_type,))
        assert x.C == c, "Stripe_NonLocalBlock(in_channels=%d) got %r" % (c, x)
        assert S * (x.H // S) == x.H, "stripe = %d does not divide H = %d" % (S, x.H)
        discri, arg = sfhip.stripe_pool(x, S, self.pool_type)
        t = engine.tape()
        held = {}
        if t is not None:
            def bwd_pool():  # the LAST op of the block's backward: dx (+)= dz + the pooling's gradient, one pass
                dd = t.grad_of(discri)
                dmean = dd.slice(0, c) if self.pool_type in ('mean', 'meanmax') else None
                dmax = dd.slice(dd.C - c, c) if self.pool_type in ('max', 'meanmax') else None
                dx, acc = t.grad_dst(x)
                sfhip.stripe_pool_bwd(dx, S, dz=t.grad_of(held["z"]), dmean=dmean, dmax=dmax, arg=arg, accumulate=acc)

            t.record(bwd_pool)
        g = engine.conv_bn_act(discri, self.g)
        theta = engine.conv_bn_act(discri, self.theta)
        phi = engine.conv_bn_act(discri, self.phi)
        y = _block_attention(theta, phi, g, self.instance)
        wy = engine.conv_bn_act(y, self.W[0], self.W[1])
        z = sfhip.stripe_add(x, wy, out=sfhip.new_act(x, x.N, x.T, x.H, x.W, c, reserve[0], reserve[1]))
        if t is not None:
            held["z"] = z

            def bwd_add():  # the FIRST op: d(W_y)[n,t,s,:] = sum over the band of dz (the 'sum' pool)
                dv, _ = sfhip.stripe_pool(t.grad_of(z), S, "sum")
                sfhip.axpy(dv, t.grad_of(wy), 1.0, accumulate=True)

            t.record(bwd_add)
        return z

    def forward(self, x, reserve=(0, 0)):
        return _same_kind(self, x, reserve)
