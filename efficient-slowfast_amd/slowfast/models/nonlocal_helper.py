"""Non-local block (reference nonlocal_helper.py:8-148) on the HIP path.

The block's attention runs over N_q <= 6272 positions against N_k <= 1568 max-pooled positions with d = 256 / 512
channels: different query and key lengths and widths far outside the flash kernels' d <= 128 register tiling.  The
softmax form STREAMS through the cross-length kernels (`sf_xattn_fwd` / `sf_xattn_bwd`, attn_cross.hip): one forward
launch for the whole batch that leaves the output and the log-sum-exp of every query, and a backward that recomputes
the probabilities from it — no score matrix in memory, any key width that is a multiple of 4.

"dot_product" has no softmax to stream, and without one the product is ASSOCIATIVE:  Y = (theta phi^T / N_k) g =
theta (phi^T g / N_k).  It runs on the two batched kernels of attn_assoc.hip: `sfhip.gram` makes M = phi^T g / N_k (one
d x dv matrix per sample, with its transpose) and `sfhip.rowmat` multiplies theta by it — two launches for the whole
batch, 2 d dv (N_q + N_k) FLOP per sample instead of 2 N_q N_k (d + dv), no score matrix.  The backward keeps only M:
D = theta^T dY (gram), then dtheta += dY M^T, dg += phi D / N_k and dphi += g D^T / N_k (three rowmat).

Views neither pair of kernels accepts (a width above 512 or not a multiple of 4) take the MATERIALISED path: three
launches per sample on the implicit-GEMM kernel with ACTIVATIONS in the weight slot:  S = theta . phi^T (phi's NDHWC
rows [N_k][d] already are the packed-weight layout), the normalisation (`sf_row_softmax_fwd`, or 1/N_k folded into the
GEMM epilogue for "dot_product"), and Y = P . g (weights = g^T from the NDHWC->NCTHW kernel).  Its backward is the same
GEMMs transposed (data-gradient convs and weight-gradient reductions over the query positions)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import sfhip
from . import engine


class Nonlocal(nn.Module):
    """theta/phi/g/out 1x1x1 convs (+bias), optional max-pool of the key side, softmax or dot-product
    normalisation, final BN (zero-initialised when zero_init_final_norm), residual add."""

    def __init__(self, dim, dim_inner, pool_size=None, instantiation="softmax", zero_init_final_conv=False,
                 zero_init_final_norm=True, norm_eps=1e-5, norm_momentum=0.1, norm_module=nn.BatchNorm3d):
        super(Nonlocal, self).__init__()
        self.dim = dim
        self.dim_inner = dim_inner
        self.pool_size = pool_size
        self.instantiation = instantiation
        self.use_pool = False if pool_size is None else any((size > 1 for size in pool_size))
        self.norm_eps = norm_eps
        self.norm_momentum = norm_momentum
        self.conv_theta = nn.Conv3d(dim, dim_inner, kernel_size=1, stride=1, padding=0)
        self.conv_phi = nn.Conv3d(dim, dim_inner, kernel_size=1, stride=1, padding=0)
        self.conv_g = nn.Conv3d(dim, dim_inner, kernel_size=1, stride=1, padding=0)
        self.conv_out = nn.Conv3d(dim_inner, dim, kernel_size=1, stride=1, padding=0)
        self.conv_out.zero_init = zero_init_final_conv
        self.bn = norm_module(num_features=dim, eps=norm_eps, momentum=norm_momentum)
        self.bn.transform_final_bn = zero_init_final_norm
        if self.use_pool:
            self.pool = nn.MaxPool3d(kernel_size=self.pool_size, stride=self.pool_size, padding=[0, 0, 0])
        if instantiation not in ("softmax", "dot_product"):
            raise NotImplementedError("Unknown norm type {}".format(instantiation))

    def forward(self, x, reserve=(0, 0)):
        (xa,) = engine.enter([x])
        with engine.internal():
            y = self.run(xa, reserve)
        return engine.leave([y])[0]

    # ------------------------------------------------------------------------------------------------
    def run(self, x, reserve=(0, 0)):
        if isinstance(engine.tape(), engine.EvalTape):
            raise NotImplementedError("Grad-CAM (the eval-mode tape) does not cover Nonlocal blocks")
        theta = engine.conv_bn_act(x, self.conv_theta)
        xp = x
        if self.use_pool:
            ks = tuple(self.pool_size)
            xp = engine.maxpool(x, ks, ks)
        phi = engine.conv_bn_act(xp, self.conv_phi)
        g = engine.conv_bn_act(xp, self.conv_g)
        y = dense_attention(theta, phi, g, self.instantiation == "softmax", float(self.dim_inner) ** -0.5)
        return engine.conv_bn_act(y, self.conv_out, self.bn, relu=False, res=x, out_reserve=reserve)


def dense_attention(theta, phi, g, softmax=True, sm_scale=1.0, dot_scale=None):
    """Y = normalise(theta phi^T) g per sample: softmax(sm_scale * S) over the keys, or S * dot_scale (softmax=False:
    Nonlocal's "dot_product"; dot_scale None = 1 / N_k, Nonlocal's; NonLocalBlock and Stripe_NonLocalBlock of
    wdf_attention_helper.py divide by the QUERY count).  theta [N, ., d] queries, phi [N, ., d] keys, g [N, ., dv] values,
    NDHWC views.  Taped.  Serves Nonlocal (d = 256 / 512) and SpatialAttention heads wider than the flash kernels' 128 channels
    (SlowFastShuffleNet w2.0 / g3: d = 240 at s4_fuse, N <= 64 positions).  The softmax form streams through the
    cross-length kernels wherever they accept the views (one launch forward, the score matrix never in memory), the
    dot-product form through the associative gram / rowmat kernels (two launches forward, four backward, only the
    d x dv matrix M kept); views neither accepts run with the score matrix MATERIALISED."""
    N, d, dv = theta.N, theta.C, g.C
    nq, nk = theta.T * theta.H * theta.W, phi.T * phi.H * phi.W
    assert phi.C == d and (g.T, g.H, g.W) == (phi.T, phi.H, phi.W)
    if softmax and sfhip.xattn_accepts(theta, phi, g):
        saved = {}
        y = sfhip.cross_attention(theta, phi, g, sm_scale, save=saved)
        t = engine.tape()
        if t is not None:
            def bwd_stream():
                sfhip.cross_attention_bwd(theta, phi, g, y, t.grad_of(y), saved["lse"], sm_scale, t.grad_of(theta),
                                          t.grad_of(phi), t.grad_of(g), accumulate=(True, True, True))
            t.record(bwd_stream)
        return y
    if not softmax and sfhip.assoc_accepts(theta, phi, g):
        inv_nk = 1.0 / nk if dot_scale is None else float(dot_scale)
        Mt, M = sfhip.gram(g, phi, inv_nk, transposed=True)  # M^T = g^T phi / N_k [dv, d] and M [d, dv] per sample
        y = sfhip.rowmat(theta, Mt, 1.0)
        t = engine.tape()
        if t is not None:
            def bwd_assoc():  # D = theta^T dY; only M was kept
                dy = t.grad_of(y)
                D, Dt = sfhip.gram(theta, dy, 1.0, transposed=True)
                sfhip.rowmat(dy, M, 1.0, out=t.grad_of(theta), accumulate=True)     # dtheta += dY M^T
                sfhip.rowmat(phi, Dt, inv_nk, out=t.grad_of(g), accumulate=True)    # dg += phi D / N_k
                sfhip.rowmat(g, D, inv_nk, out=t.grad_of(phi), accumulate=True)     # dphi += g D^T / N_k
            t.record(bwd_assoc)
        return y
    return materialised_attention(theta, phi, g, softmax, sm_scale, dot_scale)


def materialised_attention(theta, phi, g, softmax=True, sm_scale=1.0, dot_scale=None):
    """dense_attention with one [N_q, N_k] score matrix per sample in memory (kept for the backward, which makes a
    second one): whatever the streaming and the associative kernels refuse.  Dense NDHWC buffers, d % 16 == 0."""
    N, d, dv = theta.N, theta.C, g.C
    nq, nk = theta.T * theta.H * theta.W, phi.T * phi.H * phi.W
    if d % 16 != 0:
        raise NotImplementedError("materialised attention needs a key width that is a multiple of 16 on the HIP "
                                  "path (got %d)" % d)
    assert theta.cs == d and phi.cs == d and g.cs == dv and theta.coff == phi.coff == g.coff == 0
    dev = theta.buf.device
    nk_pad = (nk + 15) // 16 * 16
    inv_nk = None if softmax else torch.full((max(nk, d),), 1.0 / nk if dot_scale is None else float(dot_scale),
                                             dtype=torch.float32, device=dev)

    def transposed(a):  # [N, Tp, Hp, Wp, c] -> [N][c][nk_pad]: the packed weights of "multiply by a"
        t = sfhip.to_ncthw(a).view(N, a.C, nk)
        return t if nk_pad == nk else F.pad(t, (0, nk_pad - nk)).contiguous()

    def sample(a, n):
        return sfhip.Act(a.buf[n:n + 1], a.coff, a.C)

    one = (1, 1, 1)
    P = sfhip.new_act(theta, N, theta.T, theta.H, theta.W, nk)
    g_t = transposed(g)
    y = sfhip.new_act(theta, N, theta.T, theta.H, theta.W, dv)
    for n in range(N):  # S_n = theta_n phi_n^T (x 1/N_k for dot_product)
        sfhip.conv(sample(theta, n), phi.buf[n].view(nk, 1, d), one, scale=None if softmax else inv_nk[:nk],
                   out=sample(P, n))
    if softmax:
        sfhip.row_softmax(P, scale=sm_scale)
    for n in range(N):  # Y_n = P_n g_n
        sfhip.conv(sample(P, n), g_t[n].view(dv, 1, nk_pad), one, out=sample(y, n))
    t = engine.tape()
    if t is not None:
        def bwd():
            dy = t.grad_of(y)
            dth, dph, dg = t.grad_of(theta), t.grad_of(phi), t.grad_of(g)
            phi_t = transposed(phi)
            dP = sfhip.new_act(P, N, P.T, P.H, P.W, nk)
            for n in range(N):  # dP_n = dY_n g_n^T ;  dg_n = P_n^T dY_n
                sfhip.conv(sample(dy, n), g.buf[n].view(nk, 1, dv), one, scale=None if softmax else inv_nk[:nk],
                           out=sample(dP, n))
                dgn = sfhip.conv_wgrad(sample(dy, n), sample(P, n), nk, one, cin_pad=dv)
                dg.buf[n].view(nk, dv).add_(dgn.view(nk, dv))
            if softmax:
                sfhip.row_softmax_bwd(P, dP, scale=sm_scale)  # dP now holds dL/dS
            for n in range(N):  # dtheta_n += dS_n phi_n ;  dphi_n = dS_n^T theta_n
                dthn = sample(dth, n)
                sfhip.conv(sample(dP, n), phi_t[n].view(d, 1, nk_pad), one, res=dthn, out=dthn)
                dpn = sfhip.conv_wgrad(sample(theta, n), sample(dP, n), nk, one, cin_pad=d)
                dph.buf[n].view(nk, d).add_(dpn.view(nk, d))
        t.record(bwd)
    return y
