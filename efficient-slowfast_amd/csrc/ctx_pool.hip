// ctx_pool.hip — the global-context pooling of ContextBlock3D (GCNet; wdf_attention_helper.py:339-358) and the per-sample
// broadcast affine both attention blocks end in (wdf_attention_helper.py:121-124, 371-378).  NDHWC, fp32, gfx950.
//   sf_ctx_pool_fwd:  l[pos] = w . x[pos, :] + b;  p = softmax_pos(l);  ctx[c] = sum_pos p[pos] * x[pos, c]
//       ONE pass over x: every workgroup owns a contiguous run of one sample's positions, keeps a running (max, sum,
//       acc[C]) (online softmax) and leaves its partial in the workspace; a finish kernel merges the partials with the
//       usual max-rescale.  The logits never reach memory.
//   sf_ctx_pool_bwd:  p = exp(l - lse), dl = p * (x . dctx - ctx . dctx), dx (=|+=) p * dctx + dl * w, dw = sum dl * x
//       ONE pass again (l is recomputed), per-workgroup partial sums of dw, added in fp64 by a finish kernel.
//   sf_sample_affine_fwd / _bwd:  out = x * mul[n, c] + add[n, c];  dx (=|+=) dy * mul, dmul = sum_pos dy * x,
//       dadd = sum_pos dy — one pass each, per-sample sums through partials and a finish kernel.
// No atomics, one owner per output element, fixed summation order: bitwise reproducible.  Thread layout of bn_frozen.hip:
// CB lanes cover the channel vectors of a position (CB a power of two <= 64, so a position never leaves its wavefront
// and the dot products are butterflies), 256 / CB positions per trip, NCH channel chunks per lane when C > 64 vectors.
#include <math.h>
#include "common.h"

// Every fused multiply-add below is written out (fma / fmaf): a product and a sum written separately stay separate, so
// an accumulating form gives prior + fresh with `fresh` the very bits the first-writer form stores.
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int CTX_RUN = 128;     // positions per workgroup (at least; more when a sample would need > CTX_MAX_P of them)
constexpr int CTX_MAX_P = 1024;  // workgroups (= partials) per sample
constexpr int CTX_MAX_C = 2048;  // 64 lanes x 8 float4 chunks (x 32 scalar chunks)

struct Parts { int P; long run; };

inline Parts ctx_parts(long rows) {
  long p0 = (rows + CTX_RUN - 1) / CTX_RUN;
  if (p0 > CTX_MAX_P) p0 = CTX_MAX_P;
  if (p0 < 1) p0 = 1;
  const long run = (rows + p0 - 1) / p0;
  return {(int)((rows + run - 1) / run), run};  // no workgroup without a position
}

inline int pow2ceil_c(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

bool slice_ok(int cs, int coff, int C) { return coff >= 0 && C <= cs && coff <= cs - C; }

__device__ __forceinline__ double bfly_sum(double v, int CB) {
  for (int off = CB >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int VEC>
__device__ __forceinline__ void load_vec(const float* p, bool ok, float (&v)[VEC]) {
  if (VEC == 4) {
    const f32x4 t = ok ? *reinterpret_cast<const f32x4*>(p) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = t[e];
  } else {
    v[0] = ok ? p[0] : 0.f;
  }
}

template <int VEC>
__device__ __forceinline__ void store_vec(float* p, const float (&v)[VEC]) {
  if (VEC == 4) {
    *reinterpret_cast<f32x4*>(p) = (f32x4){v[0], v[VEC > 1 ? 1 : 0], v[VEC > 2 ? 2 : 0], v[VEC > 3 ? 3 : 0]};
  } else {
    p[0] = v[0];
  }
}

// ------------------------------------------------------------------------------------------------ context pooling
struct PoolArgs {
  const float* x; int cs, coff;
  const float* w; const float* b;
  float* ws;                 // forward: [N][C + 3][P] planes (max hi, max lo, sum, acc[C]);  backward: [C][N * P]
  const float* lse; const float* ctx; const float* dctx;
  float* dx; int dx_cs, dx_coff, dx_acc;
  long rows, run; int C, CB;
};

// The running maximum and the logits are kept in fp64 (the products of two floats are exact there): what reaches expf
// is the rounded DIFFERENCE l - max, so logits of +-80 cost no more accuracy than logits of +-1.
template <int VEC, int NCH>
__global__ __launch_bounds__(256) void ctx_pool_fwd_kernel(const PoolArgs a) {
  extern __shared__ double lds_d[];
  const int blk = blockIdx.x, n = blockIdx.y, P = gridDim.x;
  const int CB = a.CB, C = a.C;
  const int cl = threadIdx.x % CB, rl = threadIdx.x / CB, rpi = TPB / CB;
  double* const lm = lds_d;                                   // [rpi]
  float* const ls = reinterpret_cast<float*>(lds_d + rpi);    // [rpi]
  float* const la = ls + rpi;                                 // [rpi][C]
  const long r0 = (long)blk * a.run;
  const long r1 = (r0 + a.run < a.rows) ? r0 + a.run : a.rows;
  const float* const xs = a.x + (long)n * a.rows * a.cs + a.coff;
  constexpr int UR = NCH == 1 ? 4 : (NCH == 2 ? 2 : 1);
  float wv[NCH][VEC], acc[NCH][VEC];
  bool cok[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = (j * CB + cl) * VEC;
    cok[j] = c < C;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      wv[j][e] = cok[j] ? a.w[c + e] : 0.f;
      acc[j][e] = 0.f;
    }
  }
  const double bias = a.b ? (double)a.b[0] : 0.0;
  double m = -INFINITY;
  float s = 0.f;
  for (long rb = r0; rb < r1; rb += (long)rpi * UR) {  // the same trip count in every lane: the butterflies are whole
    float xv[UR][NCH][VEC];
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const long r = rb + rl + (long)u * rpi;
#pragma unroll
      for (int j = 0; j < NCH; ++j)
        load_vec<VEC>(xs + r * a.cs + (j * CB + cl) * VEC, r < r1 && cok[j], xv[u][j]);
    }
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const long r = rb + rl + (long)u * rpi;
      double d = 0.0;
#pragma unroll
      for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) d = fma((double)xv[u][j][e], (double)wv[j][e], d);
      d = bfly_sum(d, CB);
      if (r < r1) {
        const double l = d + bias;
        const double mn = l > m ? l : m;
        const float sc = expf((float)(m - mn));  // m = -inf on the first position: 0
        const float p = expf((float)(l - mn));
        s = fmaf(s, sc, p);
#pragma unroll
        for (int j = 0; j < NCH; ++j)
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[j][e] = fmaf(acc[j][e], sc, p * xv[u][j][e]);
        m = mn;
      }
    }
  }
  // the rpi position lanes of this workgroup, merged in lane order
  if (cl == 0) {
    lm[rl] = m;
    ls[rl] = s;
  }
#pragma unroll
  for (int j = 0; j < NCH; ++j)
    if (cok[j]) {
      const int c = (j * CB + cl) * VEC;
#pragma unroll
      for (int e = 0; e < VEC; ++e) la[rl * C + c + e] = acc[j][e];
    }
  __syncthreads();
  double M = -INFINITY;
  for (int i = 0; i < rpi; ++i) M = lm[i] > M ? lm[i] : M;
  float* const wsn = a.ws + (long)n * (C + 3) * P;
  for (int c = threadIdx.x; c < C + 1; c += TPB) {  // item C: the running sum
    float t = 0.f;
    for (int i = 0; i < rpi; ++i) {
      const float g = lm[i] == -INFINITY ? 0.f : expf((float)(lm[i] - M));
      t = fmaf(c < C ? la[i * C + c] : ls[i], g, t);
    }
    wsn[(long)(c < C ? 3 + c : 2) * P + blk] = t;
  }
  if (threadIdx.x == 0) {
    const float hi = (float)M;
    wsn[blk] = hi;
    wsn[(long)P + blk] = M == -INFINITY ? 0.f : (float)(M - (double)hi);
  }
}

// One wavefront per (sample, channel) and one more per sample for lse: lane l merges partials l, l + 64, ... in fp64, the
// 64 lanes are combined by a butterfly — the same order on every run.
__global__ __launch_bounds__(256) void ctx_pool_fwd_finish_kernel(const float* __restrict__ ws, int C, int P,
                                                                  float* __restrict__ ctx, float* __restrict__ lse) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item > C) return;
  const float* const wsn = ws + (long)n * (C + 3) * P;
  double M = -INFINITY;
  for (int i = lane; i < P; i += 64) {
    const double mi = (double)wsn[i] + (double)wsn[(long)P + i];
    M = mi > M ? mi : M;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(M, off, 64);
    M = o > M ? o : M;
  }
  double S = 0.0, A = 0.0;
  const float* const av = wsn + (long)(item < C ? 3 + item : 2) * P;
  for (int i = lane; i < P; i += 64) {
    const float hi = wsn[i];
    const double g = hi == -INFINITY ? 0.0 : (double)expf((float)((double)hi + (double)wsn[(long)P + i] - M));
    S += (double)wsn[2L * P + i] * g;
    A += (double)av[i] * g;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    S += __shfl_xor(S, off, 64);
    A += __shfl_xor(A, off, 64);
  }
  if (lane == 0) {
    if (item < C) ctx[(long)n * C + item] = (float)(A / S);
    else lse[n] = (float)(M + log(S));
  }
}

template <int VEC, int NCH>
__global__ __launch_bounds__(256) void ctx_pool_bwd_kernel(const PoolArgs a) {
  extern __shared__ double lds_d[];
  float* const la = reinterpret_cast<float*>(lds_d);  // [rpi][C]
  const int blk = blockIdx.x, n = blockIdx.y, P = gridDim.x;
  const int CB = a.CB, C = a.C;
  const int cl = threadIdx.x % CB, rl = threadIdx.x / CB, rpi = TPB / CB;
  const long r0 = (long)blk * a.run;
  const long r1 = (r0 + a.run < a.rows) ? r0 + a.run : a.rows;
  const float* const xs = a.x + (long)n * a.rows * a.cs + a.coff;
  float* const dxs = a.dx + (long)n * a.rows * a.dx_cs + a.dx_coff;
  constexpr int UR = NCH == 1 ? 2 : 1;
  float wv[NCH][VEC], gv[NCH][VEC], dwa[NCH][VEC];
  bool cok[NCH];
  double cd = 0.0;  // ctx . dctx of this sample
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = (j * CB + cl) * VEC;
    cok[j] = c < C;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      wv[j][e] = cok[j] ? a.w[c + e] : 0.f;
      gv[j][e] = cok[j] ? a.dctx[(long)n * C + c + e] : 0.f;
      dwa[j][e] = 0.f;
      if (cok[j]) cd = fma((double)a.ctx[(long)n * C + c + e], (double)gv[j][e], cd);
    }
  }
  cd = bfly_sum(cd, CB);
  const double shift = (a.b ? (double)a.b[0] : 0.0) - (double)a.lse[n];
  for (long rb = r0; rb < r1; rb += (long)rpi * UR) {
    float xv[UR][NCH][VEC], pv[UR][NCH][VEC];
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const long r = rb + rl + (long)u * rpi;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        load_vec<VEC>(xs + r * a.cs + (j * CB + cl) * VEC, r < r1 && cok[j], xv[u][j]);
        load_vec<VEC>(dxs + r * a.dx_cs + (j * CB + cl) * VEC, a.dx_acc && r < r1 && cok[j], pv[u][j]);
      }
    }
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const long r = rb + rl + (long)u * rpi;
      double d1 = 0.0, d2 = 0.0;
#pragma unroll
      for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          d1 = fma((double)xv[u][j][e], (double)wv[j][e], d1);
          d2 = fma((double)xv[u][j][e], (double)gv[j][e], d2);
        }
      d1 = bfly_sum(d1, CB);
      d2 = bfly_sum(d2, CB);
      if (r < r1) {
        const float p = expf((float)(d1 + shift));
        const float dl = p * (float)(d2 - cd);
#pragma unroll
        for (int j = 0; j < NCH; ++j)
          if (cok[j]) {
            float o[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              const float fresh = fmaf(dl, wv[j][e], p * gv[j][e]);
              o[e] = a.dx_acc ? pv[u][j][e] + fresh : fresh;
              dwa[j][e] = fmaf(dl, xv[u][j][e], dwa[j][e]);
            }
            store_vec<VEC>(dxs + r * a.dx_cs + (j * CB + cl) * VEC, o);
          }
      }
    }
  }
  if (!a.ws) return;  // no parameter gradient wanted
#pragma unroll
  for (int j = 0; j < NCH; ++j)
    if (cok[j]) {
      const int c = (j * CB + cl) * VEC;
#pragma unroll
      for (int e = 0; e < VEC; ++e) la[rl * C + c + e] = dwa[j][e];
    }
  __syncthreads();
  const long NP = (long)gridDim.y * P;
  for (int c = threadIdx.x; c < C; c += TPB) {
    float t = 0.f;
    for (int i = 0; i < rpi; ++i) t += la[i * C + c];
    a.ws[(long)c * NP + (long)n * P + blk] = t;
  }
}

// dw[c] (=|+=) sum_i partial[c][i] in fp64, one wavefront per channel; db = 0 exactly (the softmax is shift invariant).
__global__ __launch_bounds__(256) void ctx_pool_bwd_finish_kernel(const float* __restrict__ ws, int C, long NP,
                                                                  float* __restrict__ dw, float* __restrict__ db,
                                                                  int accumulate) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (db && !accumulate && blockIdx.x == 0 && threadIdx.x == 0) db[0] = 0.f;
  if (c >= C) return;
  double s = 0.0;
  for (long i = lane; i < NP; i += 64) s += (double)ws[(long)c * NP + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) dw[c] = accumulate ? dw[c] + (float)s : (float)s;
}

// ------------------------------------------------------------------------------------------------ per-sample affine
struct AffArgs {
  const float* x; int x_cs, x_coff;      // backward: NULL when dmul is not wanted
  const float* dy; int dy_cs, dy_coff;   // backward only
  const float* mul; const float* add;    // [N][C], NULL: 1 / 0
  float* out; int out_cs, out_coff, out_acc;
  float* ws;                             // backward: [N][2][C][P]
  long rows, run; int C, CB, nch;
};

template <int VEC>
__global__ __launch_bounds__(256) void sample_affine_fwd_kernel(const AffArgs a) {
  const int blk = blockIdx.x, n = blockIdx.y;
  const int CB = a.CB, C = a.C;
  const int cl = threadIdx.x % CB, rl = threadIdx.x / CB, rpi = TPB / CB;
  const long r0 = (long)blk * a.run;
  const long r1 = (r0 + a.run < a.rows) ? r0 + a.run : a.rows;
  const float* const xs = a.x + (long)n * a.rows * a.x_cs + a.x_coff;
  float* const os = a.out + (long)n * a.rows * a.out_cs + a.out_coff;
  for (int j = 0; j < a.nch; ++j) {
    const int c = (j * CB + cl) * VEC;
    if (c >= C) continue;
    float mu[VEC], ad[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      mu[e] = a.mul ? a.mul[(long)n * C + c + e] : 1.f;
      ad[e] = a.add ? a.add[(long)n * C + c + e] : 0.f;
    }
    long r = r0 + rl;
    for (; r + 3 * (long)rpi < r1; r += 4 * (long)rpi) {  // four positions per trip, the loads issued first
      float v[4][VEC];
#pragma unroll
      for (int u = 0; u < 4; ++u) load_vec<VEC>(xs + (r + (long)u * rpi) * a.x_cs + c, true, v[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[u][e] = fmaf(v[u][e], mu[e], ad[e]);
        store_vec<VEC>(os + (r + (long)u * rpi) * a.out_cs + c, v[u]);
      }
    }
    for (; r < r1; r += rpi) {
      float v[VEC];
      load_vec<VEC>(xs + r * a.x_cs + c, true, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) v[e] = fmaf(v[e], mu[e], ad[e]);
      store_vec<VEC>(os + r * a.out_cs + c, v);
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(256) void sample_affine_bwd_kernel(const AffArgs a) {
  __shared__ float red[2 * TPB * VEC];
  const int blk = blockIdx.x, n = blockIdx.y, P = gridDim.x;
  const int CB = a.CB, C = a.C;
  const int cl = threadIdx.x % CB, rl = threadIdx.x / CB, rpi = TPB / CB;
  const long r0 = (long)blk * a.run;
  const long r1 = (r0 + a.run < a.rows) ? r0 + a.run : a.rows;
  const float* const gs = a.dy + (long)n * a.rows * a.dy_cs + a.dy_coff;
  const float* const xs = a.x ? a.x + (long)n * a.rows * a.x_cs + a.x_coff : nullptr;
  float* const os = a.out + (long)n * a.rows * a.out_cs + a.out_coff;
  for (int j = 0; j < a.nch; ++j) {  // (uniform trip count: the barriers below are reached by every thread)
    const int c = (j * CB + cl) * VEC;
    const bool ok = c < C;
    float mu[VEC], s1[VEC], s2[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      mu[e] = (a.mul && ok) ? a.mul[(long)n * C + c + e] : 1.f;
      s1[e] = 0.f;
      s2[e] = 0.f;
    }
    if (ok) {
      long r = r0 + rl;
      for (; r + (long)rpi < r1; r += 2 * (long)rpi) {  // two positions per trip, the loads issued first
        float g[2][VEC], xv[2][VEC], pv[2][VEC];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const long ru = r + (long)u * rpi;
          load_vec<VEC>(gs + ru * a.dy_cs + c, true, g[u]);
          load_vec<VEC>(xs + ru * a.x_cs + c, xs != nullptr, xv[u]);
          load_vec<VEC>(os + ru * a.out_cs + c, a.out_acc != 0, pv[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          float o[VEC];
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const float fresh = g[u][e] * mu[e];
            o[e] = a.out_acc ? pv[u][e] + fresh : fresh;
            s1[e] += g[u][e];
            s2[e] = fmaf(g[u][e], xv[u][e], s2[e]);
          }
          store_vec<VEC>(os + (r + (long)u * rpi) * a.out_cs + c, o);
        }
      }
      for (; r < r1; r += rpi) {
        float g[VEC], xv[VEC], pv[VEC], o[VEC];
        load_vec<VEC>(gs + r * a.dy_cs + c, true, g);
        load_vec<VEC>(xs + r * a.x_cs + c, xs != nullptr, xv);
        load_vec<VEC>(os + r * a.out_cs + c, a.out_acc != 0, pv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float fresh = g[e] * mu[e];
          o[e] = a.out_acc ? pv[e] + fresh : fresh;
          s1[e] += g[e];
          s2[e] = fmaf(g[e], xv[e], s2[e]);
        }
        store_vec<VEC>(os + r * a.out_cs + c, o);
      }
    }
    if (!a.ws) continue;  // (a.ws is uniform)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      red[threadIdx.x * VEC + e] = s1[e];
      red[(TPB + threadIdx.x) * VEC + e] = s2[e];
    }
    __syncthreads();
    if (rl == 0 && ok) {  // the rpi position lanes of this channel, in lane order
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float t1 = 0.f, t2 = 0.f;
        for (int i = 0; i < rpi; ++i) {
          t1 += red[(i * CB + cl) * VEC + e];
          t2 += red[(TPB + i * CB + cl) * VEC + e];
        }
        a.ws[(((long)n * 2 + 0) * C + c + e) * P + blk] = t1;
        a.ws[(((long)n * 2 + 1) * C + c + e) * P + blk] = t2;
      }
    }
    __syncthreads();
  }
}

// dadd[n][c] = sum_i partial[n][0][c][i], dmul[n][c] = sum_i partial[n][1][c][i]: one wavefront per (n, c), fp64.
__global__ __launch_bounds__(256) void sample_affine_finish_kernel(const float* __restrict__ ws, int N, int C, int P,
                                                                   float* __restrict__ dmul, float* __restrict__ dadd) {
  const int lane = threadIdx.x & 63;
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long)N * C) return;
  const int n = (int)(item / C), c = (int)(item - (long)n * C);
  double s1 = 0.0, s2 = 0.0;
  for (int i = lane; i < P; i += 64) {
    s1 += (double)ws[(((long)n * 2 + 0) * C + c) * P + i];
    s2 += (double)ws[(((long)n * 2 + 1) * C + c) * P + i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_xor(s1, off, 64);
    s2 += __shfl_xor(s2, off, 64);
  }
  if (lane == 0) {
    if (dadd) dadd[item] = (float)s1;
    if (dmul) dmul[item] = (float)s2;
  }
}

struct Layout { int CB, nch; };

inline Layout layout_of(int C, bool vec4) {
  const int cv = sf_cdiv(C, vec4 ? 4 : 1);
  const int cb = pow2ceil_c(cv) < 64 ? pow2ceil_c(cv) : 64;
  return {cb, pow2ceil_c(sf_cdiv(cv, cb))};
}

bool dims_ok(int N, long rows, int C) {
  return N > 0 && N <= 65535 && rows > 0 && C > 0 && C <= CTX_MAX_C && rows <= (1L << 40);
}

#define CTX_DISPATCH(KERNEL, vec4, nch, grid, lds, stream, args)                                                   \
  do {                                                                                                             \
    if (vec4) {                                                                                                    \
      switch (nch) {                                                                                               \
        case 1: hipLaunchKernelGGL((KERNEL<4, 1>), grid, dim3(TPB), lds, stream, args); break;                     \
        case 2: hipLaunchKernelGGL((KERNEL<4, 2>), grid, dim3(TPB), lds, stream, args); break;                     \
        case 4: hipLaunchKernelGGL((KERNEL<4, 4>), grid, dim3(TPB), lds, stream, args); break;                     \
        default: hipLaunchKernelGGL((KERNEL<4, 8>), grid, dim3(TPB), lds, stream, args); break;                    \
      }                                                                                                            \
    } else {                                                                                                       \
      switch (nch) {                                                                                               \
        case 1: hipLaunchKernelGGL((KERNEL<1, 1>), grid, dim3(TPB), lds, stream, args); break;                     \
        case 2: hipLaunchKernelGGL((KERNEL<1, 2>), grid, dim3(TPB), lds, stream, args); break;                     \
        case 4: hipLaunchKernelGGL((KERNEL<1, 4>), grid, dim3(TPB), lds, stream, args); break;                     \
        case 8: hipLaunchKernelGGL((KERNEL<1, 8>), grid, dim3(TPB), lds, stream, args); break;                     \
        case 16: hipLaunchKernelGGL((KERNEL<1, 16>), grid, dim3(TPB), lds, stream, args); break;                   \
        default: hipLaunchKernelGGL((KERNEL<1, 32>), grid, dim3(TPB), lds, stream, args); break;                   \
      }                                                                                                            \
    }                                                                                                              \
  } while (0)

}  // namespace

extern "C" int sf_ctx_pool_parts(long rows_per_sample) {
  return rows_per_sample > 0 ? ctx_parts(rows_per_sample).P : 0;
}

extern "C" long sf_ctx_pool_ws_floats(int N, long rows_per_sample, int C) {
  if (!dims_ok(N, rows_per_sample, C)) return 0;
  return (long)N * ctx_parts(rows_per_sample).P * (C + 3);
}

extern "C" int sf_ctx_pool_fwd(const float* x, int cs, int coff, int N, long rows_per_sample, int C, const float* w,
                               const float* b, float* ctx, float* lse, float* ws, void* stream) {
  if (!x || !w || !ctx || !lse || !ws) return SF_EINVAL;
  if (!dims_ok(N, rows_per_sample, C) || !slice_ok(cs, coff, C)) return SF_EINVAL;
  const bool vec4 = (C % 4 == 0) && (cs % 4 == 0) && (coff % 4 == 0) && sf_aligned16(x);
  const Layout L = layout_of(C, vec4);
  const Parts pt = ctx_parts(rows_per_sample);
  PoolArgs a = {};
  a.x = x; a.cs = cs; a.coff = coff; a.w = w; a.b = b; a.ws = ws;
  a.rows = rows_per_sample; a.run = pt.run; a.C = C; a.CB = L.CB;
  const int rpi = TPB / L.CB;
  const size_t lds = (size_t)rpi * 8 + (size_t)rpi * 4 + (size_t)rpi * C * 4;
  CTX_DISPATCH(ctx_pool_fwd_kernel, vec4, L.nch, dim3(pt.P, N), lds, (hipStream_t)stream, a);
  hipLaunchKernelGGL(ctx_pool_fwd_finish_kernel, dim3(sf_cdiv(C + 1, 4), N), dim3(TPB), 0, (hipStream_t)stream, ws, C,
                     pt.P, ctx, lse);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_ctx_pool_bwd(const float* x, int cs, int coff, int N, long rows_per_sample, int C, const float* w,
                               const float* b, const float* lse, const float* ctx, const float* dctx, float* dx,
                               int dx_cs, int dx_coff, int accumulate, float* dw, float* db, int dw_accumulate,
                               float* ws, void* stream) {
  if (!x || !w || !lse || !ctx || !dctx || !dx) return SF_EINVAL;
  if ((dw && !ws) || (db && !dw)) return SF_EINVAL;
  if (!dims_ok(N, rows_per_sample, C) || !slice_ok(cs, coff, C) || !slice_ok(dx_cs, dx_coff, C)) return SF_EINVAL;
  const bool vec4 = (C % 4 == 0) && (cs % 4 == 0) && (coff % 4 == 0) && (dx_cs % 4 == 0) && (dx_coff % 4 == 0) &&
                    sf_aligned16(x) && sf_aligned16(dx);
  const Layout L = layout_of(C, vec4);
  const Parts pt = ctx_parts(rows_per_sample);
  PoolArgs a = {};
  a.x = x; a.cs = cs; a.coff = coff; a.w = w; a.b = b; a.ws = dw ? ws : nullptr;
  a.lse = lse; a.ctx = ctx; a.dctx = dctx;
  a.dx = dx; a.dx_cs = dx_cs; a.dx_coff = dx_coff; a.dx_acc = accumulate ? 1 : 0;
  a.rows = rows_per_sample; a.run = pt.run; a.C = C; a.CB = L.CB;
  const size_t lds = (size_t)(TPB / L.CB) * C * 4;
  CTX_DISPATCH(ctx_pool_bwd_kernel, vec4, L.nch, dim3(pt.P, N), lds, (hipStream_t)stream, a);
  if (dw)
    hipLaunchKernelGGL(ctx_pool_bwd_finish_kernel, dim3(sf_cdiv(C, 4)), dim3(TPB), 0, (hipStream_t)stream, ws, C,
                       (long)N * pt.P, dw, db, dw_accumulate ? 1 : 0);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" long sf_sample_affine_ws_floats(int N, long rows_per_sample, int C) {
  if (!dims_ok(N, rows_per_sample, C)) return 0;
  return (long)N * ctx_parts(rows_per_sample).P * 2 * C;
}

extern "C" int sf_sample_affine_fwd(const float* x, int cs, int coff, int N, long rows_per_sample, int C,
                                    const float* mul, const float* add, float* out, int out_cs, int out_coff,
                                    void* stream) {
  if (!x || !out) return SF_EINVAL;
  if (!dims_ok(N, rows_per_sample, C) || !slice_ok(cs, coff, C) || !slice_ok(out_cs, out_coff, C)) return SF_EINVAL;
  const bool vec4 = (C % 4 == 0) && (cs % 4 == 0) && (coff % 4 == 0) && (out_cs % 4 == 0) && (out_coff % 4 == 0) &&
                    sf_aligned16(x) && sf_aligned16(out);
  const Layout L = layout_of(C, vec4);
  const Parts pt = ctx_parts(rows_per_sample);
  AffArgs a = {};
  a.x = x; a.x_cs = cs; a.x_coff = coff; a.mul = mul; a.add = add;
  a.out = out; a.out_cs = out_cs; a.out_coff = out_coff;
  a.rows = rows_per_sample; a.run = pt.run; a.C = C; a.CB = L.CB; a.nch = L.nch;
  if (vec4)
    hipLaunchKernelGGL(sample_affine_fwd_kernel<4>, dim3(pt.P, N), dim3(TPB), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(sample_affine_fwd_kernel<1>, dim3(pt.P, N), dim3(TPB), 0, (hipStream_t)stream, a);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_sample_affine_bwd(const float* dy, int dy_cs, int dy_coff, const float* x, int x_cs, int x_coff,
                                    int N, long rows_per_sample, int C, const float* mul, float* dx, int dx_cs,
                                    int dx_coff, int accumulate, float* dmul, float* dadd, float* ws, void* stream) {
  if (!dy || !dx) return SF_EINVAL;
  if (dmul && !x) return SF_EINVAL;
  if ((dmul || dadd) && !ws) return SF_EINVAL;
  if (!dims_ok(N, rows_per_sample, C) || !slice_ok(dy_cs, dy_coff, C) || !slice_ok(dx_cs, dx_coff, C)) return SF_EINVAL;
  if (dmul && !slice_ok(x_cs, x_coff, C)) return SF_EINVAL;
  const bool use_x = dmul != nullptr;
  const bool vec4 = (C % 4 == 0) && (dy_cs % 4 == 0) && (dy_coff % 4 == 0) && (dx_cs % 4 == 0) && (dx_coff % 4 == 0) &&
                    sf_aligned16(dy) && sf_aligned16(dx) &&
                    (!use_x || ((x_cs % 4 == 0) && (x_coff % 4 == 0) && sf_aligned16(x)));
  const Layout L = layout_of(C, vec4);
  const Parts pt = ctx_parts(rows_per_sample);
  AffArgs a = {};
  a.x = use_x ? x : nullptr; a.x_cs = x_cs; a.x_coff = x_coff;
  a.dy = dy; a.dy_cs = dy_cs; a.dy_coff = dy_coff; a.mul = mul;
  a.out = dx; a.out_cs = dx_cs; a.out_coff = dx_coff; a.out_acc = accumulate ? 1 : 0;
  a.ws = (dmul || dadd) ? ws : nullptr;
  a.rows = rows_per_sample; a.run = pt.run; a.C = C; a.CB = L.CB; a.nch = L.nch;
  if (vec4)
    hipLaunchKernelGGL(sample_affine_bwd_kernel<4>, dim3(pt.P, N), dim3(TPB), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(sample_affine_bwd_kernel<1>, dim3(pt.P, N), dim3(TPB), 0, (hipStream_t)stream, a);
  if (a.ws)
    hipLaunchKernelGGL(sample_affine_finish_kernel, dim3(sf_cdiv((long)N * C, 4)), dim3(TPB), 0, (hipStream_t)stream,
                       ws, N, C, pt.P, dmul, dadd);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
