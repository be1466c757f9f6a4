// attn_cross.hip — streaming scaled softmax attention with different query and key lengths and separate key / value
// widths (M/nonlocal_helper.py:105-148: the Nonlocal block; SpatialAttention heads wider than 128 channels):
//   Y[b,i,:] = sum_j softmax_j(sm_scale <Q[b,i,:], K[b,j,:]>) V[b,j,:]      Q [B,Nq,d]  K [B,Nk,d]  V [B,Nk,dv]
// fp32 in and out on v_mfma_f32_32x32x2_f32.  The Nq x Nk scores live in registers only: the forward streams the softmax
// with a running maximum and leaves lse[B,Nq]; the backward recomputes P from lse in two kernels, one stationary on 32
// keys (dK, dV) and one on 32 queries (dQ).  Every output element has one owner lane and a fixed summation order, so
// there are no float atomics and two runs give the same bits.
//
// One workgroup = 4 wavefronts = one 32-row tile of the stationary side, marching over 32-row tiles of the other.
//   * A product that reduces over the WIDTH (S = Q K^T over d, dP = dY V^T over dv) is cut over the four wavefronts:
//     wavefront w takes elements [w WS, (w+1) WS) of every row, WS = bucket / 4, lane half h the half [h WS/2, ..) of it
//     (the reduction order of an MFMA chain is free as long as both operands agree), so every lane reads WS/2 contiguous
//     floats of ONE row straight from global memory as float4 — elements past the width are zeros in registers, never in
//     HBM.  The four partial 32 x 32 tiles meet in LDS and every wavefront sums them in the same order.
//   * A product that reduces over the TILE's 32 rows (Y^T = V^T P^T, dV^T = dY^T P, dK^T = Q^T dS, dQ^T = K^T dS^T)
//     takes the 32 x 32 result above as its B operand as it lies in the accumulator registers (column on the lane, the
//     16 registers = rows r&3 + 8 (r>>2) + 4 h), the A operand X[that row][column block + lane&31] from global memory.
//     Each wavefront owns bucket / 4 output columns: at most four 32 x 32 accumulators = 64 registers.
// Width buckets 128 / 256 / 512 for d and dv separately (9 instantiations per kernel).
//
// Softmax reference: log2 domain.  The reference maximum m of a query is STALE with XATTN_HEADROOM = 16 log2 units of
// headroom: it is refreshed (Y^T and the denominator rescaled by 2^(m_old - m_new), once, before the tile's P exists)
// only when some query of the tile meets a score more than 16 above its reference.  P is then at most 2^16 and a
// denominator at most N_k 2^16: far inside fp32, whose relative precision does not depend on the scale.  Keys past N_k
// score -inf (P = 0 exactly); query rows past N_q are computed on zeros and never stored.
#include "common.h"
#include "attn_tile.h"

namespace {

constexpr float XATTN_HEADROOM = 16.f;
constexpr float XATTN_LOG2E = 1.4426950408889634f;

struct XArgs {
  const float* q; const float* k; const float* v; const float* dy;
  const float* lse; const float* dvec;
  float* y; float* lse_out;
  float* dq; float* dk; float* dv;
  int q_cs, k_cs, v_cs, y_cs, dy_cs, dq_cs, dk_cs, dv_cs;
  int d, dvw, acc_mask;
  long Nq, Nk;
  float sm_scale;
};

// ---------------------------------------------------------------------------------------------------------- forward
template <int WD, int WV>
__global__ __launch_bounds__(256) void xattn_fwd_kernel(XArgs a) {
  constexpr int DS = WD / 4, NB = WV / 128;
  __shared__ float red[2][4096];  // alternating buffers: one barrier per key tile
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
  const int b = blockIdx.y;
  const long q0 = (long)blockIdx.x * 32;
  const float* __restrict__ Q = a.q + (long)b * a.Nq * a.q_cs;
  const float* __restrict__ K = a.k + (long)b * a.Nk * a.k_cs;
  const float* __restrict__ V = a.v + (long)b * a.Nk * a.v_cs;
  const int e0 = w * DS + h * (DS / 2), col0 = w * NB * 32;
  const float c2 = a.sm_scale * XATTN_LOG2E;

  float qs[DS / 2];
  xload_slice<DS>(Q, (q0 + c) * a.q_cs, q0 + c < a.Nq, e0, a.d, qs);
  f32x16 acc[NB];
  xzero<NB>(acc);
  float m = -INFINITY, l = 0.f;  // this lane's query: reference maximum; denominator over this lane half's keys
  const long nkt = (a.Nk + 31) / 32;
  for (long kt = 0; kt < nkt; ++kt) {
    const long k0 = kt * 32;
    float ks[DS / 2];
    xload_slice<DS>(K, (k0 + c) * a.k_cs, k0 + c < a.Nk, e0, a.d, ks);
    f32x16 s = xdot<DS>(ks, qs);  // S^T: rows (registers) = keys, column (lane) = query
    float* buf = red[kt & 1];
    xput(buf, w, lane, s);
    __syncthreads();
    s = xget(buf, lane);
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = k0 + xrow(r, h) < a.Nk ? s[r] * c2 : -INFINITY;
      mt = fmaxf(mt, s[r]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    if (__any(mt > m + XATTN_HEADROOM)) {  // refresh: everything at the old reference is rescaled once, P not yet made
      const float mn = fmaxf(m, mt);       // finite: every tile holds at least one real key
      const float f = exp2f(m - mn);
      m = mn;
      l *= f;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] *= f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = exp2f(s[r] - m);
      l += s[r];
    }
    xacc_t<NB>(acc, V, a.v_cs, k0, a.Nk, col0, a.dvw, s, h, c);  // Y^T += V^T P^T
  }
  l += __shfl_xor(l, 32);
  const bool qv = q0 + c < a.Nq;
  xstore_t<NB>(acc, a.y + (long)b * a.Nq * a.y_cs, (q0 + c) * a.y_cs, qv, col0, a.dvw, 1.f / l, false, h);
  if (w == 0 && h == 0 && qv) a.lse_out[(long)b * a.Nq + q0 + c] = m + log2f(l);
}

// ------------------------------------------------------------------------------- backward, key-stationary: dK and dV
template <int WD, int WV>
__global__ __launch_bounds__(256) void xattn_bwd_dkv_kernel(XArgs a) {
  constexpr int DS = WD / 4, VS = WV / 4, NBD = WD / 128, NBV = WV / 128;
  __shared__ float red[2][4096];  // S and dP partials
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
  const int b = blockIdx.y;
  const long k0 = (long)blockIdx.x * 32;
  const float* __restrict__ Q = a.q + (long)b * a.Nq * a.q_cs;
  const float* __restrict__ K = a.k + (long)b * a.Nk * a.k_cs;
  const float* __restrict__ V = a.v + (long)b * a.Nk * a.v_cs;
  const float* __restrict__ DY = a.dy + (long)b * a.Nq * a.dy_cs;
  const float* __restrict__ lse = a.lse + (long)b * a.Nq;
  const float* __restrict__ dvec = a.dvec + (long)b * a.Nq;
  const int ed = w * DS + h * (DS / 2), ev = w * VS + h * (VS / 2);
  const float c2 = a.sm_scale * XATTN_LOG2E;
  const bool kv = k0 + c < a.Nk;

  float ks[DS / 2], vs[VS / 2];
  xload_slice<DS>(K, (k0 + c) * a.k_cs, kv, ed, a.d, ks);
  xload_slice<VS>(V, (k0 + c) * a.v_cs, kv, ev, a.dvw, vs);
  f32x16 dk[NBD], dv[NBV];
  xzero<NBD>(dk);
  xzero<NBV>(dv);
  const long nqt = (a.Nq + 31) / 32;
  for (long qt = 0; qt < nqt; ++qt) {
    const long q0 = qt * 32;
    f32x16 s, dp;
    {
      float qs[DS / 2];
      xload_slice<DS>(Q, (q0 + c) * a.q_cs, q0 + c < a.Nq, ed, a.d, qs);
      s = xdot<DS>(qs, ks);  // S: rows (registers) = queries, column (lane) = key
    }
    {
      float dys[VS / 2];
      xload_slice<VS>(DY, (q0 + c) * a.dy_cs, q0 + c < a.Nq, ev, a.dvw, dys);
      dp = xdot<VS>(dys, vs);  // dP = dY V^T, same layout
    }
    __syncthreads();  // the previous tile's partials have been read
    xput(red[0], w, lane, s);
    xput(red[1], w, lane, dp);
    __syncthreads();
    s = xget(red[0], lane);
    dp = xget(red[1], lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long qi = q0 + xrow(r, h);
      float p = 0.f, ds = 0.f;
      if (qi < a.Nq) {
        p = exp2f(s[r] * c2 - lse[qi]);
        ds = p * (dp[r] - dvec[qi]) * a.sm_scale;
      }
      s[r] = p;
      dp[r] = ds;
    }
    xacc_t<NBV>(dv, DY, a.dy_cs, q0, a.Nq, w * NBV * 32, a.dvw, s, h, c);  // dV^T += dY^T P
    xacc_t<NBD>(dk, Q, a.q_cs, q0, a.Nq, w * NBD * 32, a.d, dp, h, c);     // dK^T += Q^T dS
  }
  xstore_t<NBD>(dk, a.dk + (long)b * a.Nk * a.dk_cs, (k0 + c) * a.dk_cs, kv, w * NBD * 32, a.d, 1.f,
                (a.acc_mask & 2) != 0, h);
  xstore_t<NBV>(dv, a.dv + (long)b * a.Nk * a.dv_cs, (k0 + c) * a.dv_cs, kv, w * NBV * 32, a.dvw, 1.f,
                (a.acc_mask & 4) != 0, h);
}

// ------------------------------------------------------------------------------------ backward, query-stationary: dQ
template <int WD, int WV>
__global__ __launch_bounds__(256) void xattn_bwd_dq_kernel(XArgs a) {
  constexpr int DS = WD / 4, VS = WV / 4, NBD = WD / 128;
  __shared__ float red[2][4096];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
  const int b = blockIdx.y;
  const long q0 = (long)blockIdx.x * 32;
  const float* __restrict__ Q = a.q + (long)b * a.Nq * a.q_cs;
  const float* __restrict__ K = a.k + (long)b * a.Nk * a.k_cs;
  const float* __restrict__ V = a.v + (long)b * a.Nk * a.v_cs;
  const float* __restrict__ DY = a.dy + (long)b * a.Nq * a.dy_cs;
  const int ed = w * DS + h * (DS / 2), ev = w * VS + h * (VS / 2);
  const float c2 = a.sm_scale * XATTN_LOG2E;
  const bool qv = q0 + c < a.Nq;

  float qs[DS / 2], dys[VS / 2];
  xload_slice<DS>(Q, (q0 + c) * a.q_cs, qv, ed, a.d, qs);
  xload_slice<VS>(DY, (q0 + c) * a.dy_cs, qv, ev, a.dvw, dys);
  const float l2 = qv ? a.lse[(long)b * a.Nq + q0 + c] : 0.f;
  const float dq_i = qv ? a.dvec[(long)b * a.Nq + q0 + c] : 0.f;
  f32x16 dq[NBD];
  xzero<NBD>(dq);
  const long nkt = (a.Nk + 31) / 32;
  for (long kt = 0; kt < nkt; ++kt) {
    const long k0 = kt * 32;
    f32x16 s, dp;
    {
      float ks[DS / 2];
      xload_slice<DS>(K, (k0 + c) * a.k_cs, k0 + c < a.Nk, ed, a.d, ks);
      s = xdot<DS>(ks, qs);  // S^T: rows (registers) = keys, column (lane) = query
    }
    {
      float vs[VS / 2];
      xload_slice<VS>(V, (k0 + c) * a.v_cs, k0 + c < a.Nk, ev, a.dvw, vs);
      dp = xdot<VS>(vs, dys);  // dP^T = V dY^T
    }
    __syncthreads();
    xput(red[0], w, lane, s);
    xput(red[1], w, lane, dp);
    __syncthreads();
    s = xget(red[0], lane);
    dp = xget(red[1], lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float ds = 0.f;
      if (k0 + xrow(r, h) < a.Nk) ds = exp2f(s[r] * c2 - l2) * (dp[r] - dq_i) * a.sm_scale;
      dp[r] = ds;
    }
    xacc_t<NBD>(dq, K, a.k_cs, k0, a.Nk, w * NBD * 32, a.d, dp, h, c);  // dQ^T += K^T dS^T
  }
  xstore_t<NBD>(dq, a.dq + (long)b * a.Nq * a.dq_cs, (q0 + c) * a.dq_cs, qv, w * NBD * 32, a.d, 1.f,
                (a.acc_mask & 1) != 0, h);
}

int bucket(int w) { return w <= 128 ? 0 : (w <= 256 ? 1 : 2); }

bool view_ok(const void* p, int cs, int width) { return sf_aligned16(p) && cs % 4 == 0 && cs >= width; }

#define XATTN_DISPATCH(KERNEL, grid)                                                                     \
  do {                                                                                                    \
    switch (bucket(a.d) * 3 + bucket(a.dvw)) {                                                            \
      case 0: hipLaunchKernelGGL((KERNEL<128, 128>), grid, dim3(256), 0, s, a); break;                    \
      case 1: hipLaunchKernelGGL((KERNEL<128, 256>), grid, dim3(256), 0, s, a); break;                    \
      case 2: hipLaunchKernelGGL((KERNEL<128, 512>), grid, dim3(256), 0, s, a); break;                    \
      case 3: hipLaunchKernelGGL((KERNEL<256, 128>), grid, dim3(256), 0, s, a); break;                    \
      case 4: hipLaunchKernelGGL((KERNEL<256, 256>), grid, dim3(256), 0, s, a); break;                    \
      case 5: hipLaunchKernelGGL((KERNEL<256, 512>), grid, dim3(256), 0, s, a); break;                    \
      case 6: hipLaunchKernelGGL((KERNEL<512, 128>), grid, dim3(256), 0, s, a); break;                    \
      case 7: hipLaunchKernelGGL((KERNEL<512, 256>), grid, dim3(256), 0, s, a); break;                    \
      default: hipLaunchKernelGGL((KERNEL<512, 512>), grid, dim3(256), 0, s, a); break;                   \
    }                                                                                                     \
    SF_CHECK_LAUNCH();                                                                                    \
  } while (0)

}  // namespace

extern "C" int sf_xattn_accepts(long Nq, long Nk, int d, int dv) {
  return Nq >= 1 && Nk >= 1 && Nq <= (1L << 31) - 32 && Nk <= (1L << 31) - 32 && d >= 4 && d <= 512 && d % 4 == 0 &&
                 dv >= 4 && dv <= 512 && dv % 4 == 0
             ? 1
             : 0;
}

extern "C" long sf_xattn_bwd_ws_floats(int B, long Nq, long Nk, int d, int dv) {
  (void)B; (void)Nq; (void)Nk; (void)d; (void)dv;
  return 0;  // every gradient element has one owner lane: no partial planes
}

extern "C" int sf_xattn_fwd(const float* q, int q_cs, const float* k, int k_cs, const float* v, int v_cs, float* y,
                            int y_cs, float* lse, int B, long Nq, long Nk, int d, int dv, float sm_scale,
                            void* stream) {
  if (!q || !k || !v || !y || !lse || B <= 0 || B > 65535) return SF_EINVAL;
  if (!sf_xattn_accepts(Nq, Nk, d, dv)) return SF_ENOTTAKEN;
  if (q_cs < d || k_cs < d || v_cs < dv || y_cs < dv) return SF_EINVAL;
  if (!view_ok(q, q_cs, d) || !view_ok(k, k_cs, d) || !view_ok(v, v_cs, dv) || !view_ok(y, y_cs, dv)) return SF_EALIGN;
  XArgs a = {};
  a.q = q; a.k = k; a.v = v; a.y = y; a.lse_out = lse;
  a.q_cs = q_cs; a.k_cs = k_cs; a.v_cs = v_cs; a.y_cs = y_cs;
  a.d = d; a.dvw = dv; a.Nq = Nq; a.Nk = Nk; a.sm_scale = sm_scale;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((Nq + 31) / 32), (unsigned)B);
  XATTN_DISPATCH(xattn_fwd_kernel, grid);
  return SF_OK;
}

extern "C" int sf_xattn_bwd(const float* q, int q_cs, const float* k, int k_cs, const float* v, int v_cs,
                            const float* dy, int dy_cs, const float* lse, const float* dvec, float* dq, int dq_cs,
                            float* dk, int dk_cs, float* dv_, int dv_cs, int accumulate_mask, int B, long Nq, long Nk,
                            int d, int dv, float sm_scale, float* ws, void* stream) {
  (void)ws;
  if (!q || !k || !v || !dy || !lse || !dvec || !dq || !dk || !dv_ || B <= 0 || B > 65535) return SF_EINVAL;
  if (accumulate_mask < 0 || accumulate_mask > 7) return SF_EINVAL;
  if (!sf_xattn_accepts(Nq, Nk, d, dv)) return SF_ENOTTAKEN;
  if (q_cs < d || k_cs < d || dq_cs < d || dk_cs < d || v_cs < dv || dy_cs < dv || dv_cs < dv) return SF_EINVAL;
  if (!view_ok(q, q_cs, d) || !view_ok(k, k_cs, d) || !view_ok(v, v_cs, dv) || !view_ok(dy, dy_cs, dv) ||
      !view_ok(dq, dq_cs, d) || !view_ok(dk, dk_cs, d) || !view_ok(dv_, dv_cs, dv))
    return SF_EALIGN;
  XArgs a = {};
  a.q = q; a.k = k; a.v = v; a.dy = dy; a.lse = lse; a.dvec = dvec; a.dq = dq; a.dk = dk; a.dv = dv_;
  a.q_cs = q_cs; a.k_cs = k_cs; a.v_cs = v_cs; a.dy_cs = dy_cs; a.dq_cs = dq_cs; a.dk_cs = dk_cs; a.dv_cs = dv_cs;
  a.d = d; a.dvw = dv; a.acc_mask = accumulate_mask; a.Nq = Nq; a.Nk = Nk; a.sm_scale = sm_scale;
  hipStream_t s = (hipStream_t)stream;
  const dim3 gk((unsigned)((Nk + 31) / 32), (unsigned)B), gq((unsigned)((Nq + 31) / 32), (unsigned)B);
  XATTN_DISPATCH(xattn_bwd_dkv_kernel, gk);
  XATTN_DISPATCH(xattn_bwd_dq_kernel, gq);
  return SF_OK;
}
