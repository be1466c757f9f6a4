// stripe_pool.hip — the memory-bound half of Stripe_NonLocalBlock (wdf_attention_helper.py:198-273): pooling over the
// horizontal stripes of every frame (:243-254), the per-stripe broadcast add (:269-271) and their backward.
// NDHWC, fp32, gfx950.
//   A frame's H rows are cut into S stripes of hs = H / S rows; stripe s is rows s*hs .. (s+1)*hs-1 and all W columns,
//   what reshape(b*c*t, stripe, h//stripe, w) + adaptive pooling selects.  In NDHWC the L = hs*W positions of stripe
//   unit u = (n*T + t)*S + s are CONTIGUOUS: positions u*L .. (u+1)*L-1 — every kernel sees x as [U][L][C].
//   sf_stripe_pool_fwd:  out[u, c] = mean | max | sum over the L positions (meanmax: mean in [0,C), max in [C,2C)),
//       arg[u, c] = the FIRST position (h, w order) holding the maximum.  x is read once; one workgroup per
//       (unit, chunk of channels), lanes along channels, the 256 / CB position lanes merged in LDS in lane order.
//   sf_stripe_add_fwd:   z[u, l, c] = x[u, l, c] + v[u, c]
//   sf_stripe_pool_bwd:  dx[u, l, c] (=|+=) dz[u, l, c] + dmean[u, c] / L + [l == arg[u, c]] * dmax[u, c]
// No atomics, one owner per output element, fixed summation order: bitwise reproducible.  Thread layout of
// ctx_pool.hip: CB lanes cover the channel vectors of a position (CB a power of two <= 64), 256 / CB positions per trip.
#include <math.h>
#include "common.h"

// a product and a sum written separately stay separate: an accumulating form gives prior + fresh with `fresh` the very
// bits the first-writer form stores
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int RUN = 128;          // positions of a stripe per workgroup in the add / backward kernels (at least)
constexpr int MAX_PARTS = 1024;   // workgroups per stripe unit there
constexpr int MAX_C = 1 << 20;

typedef int i32x4 __attribute__((ext_vector_type(4)));

inline int pow2ceil_s(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

struct Layout { int CB, nch; };

inline Layout layout_of(int C, bool vec4) {
  const int cv = sf_cdiv(C, vec4 ? 4 : 1);
  const int cb = pow2ceil_s(cv) < 64 ? pow2ceil_s(cv) : 64;
  return {cb, sf_cdiv(cv, cb)};
}

struct Parts { int P; int run; };

inline Parts parts_of(int L) {
  int p0 = (L + RUN - 1) / RUN;
  if (p0 > MAX_PARTS) p0 = MAX_PARTS;
  const int run = (L + p0 - 1) / p0;
  return {(L + run - 1) / run, run};  // no workgroup without a position
}

bool slice_ok(int cs, int coff, int C) { return coff >= 0 && C <= cs && coff <= cs - C; }
bool vec_ok(const void* p, int cs, int coff) { return (cs % 4 == 0) && (coff % 4 == 0) && sf_aligned16(p); }

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
__device__ __forceinline__ void load_ivec(const int* p, bool ok, int (&v)[VEC]) {
  if (VEC == 4) {
    const i32x4 t = ok ? *reinterpret_cast<const i32x4*>(p) : (i32x4){-1, -1, -1, -1};
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = t[e];
  } else {
    v[0] = ok ? p[0] : -1;
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

template <int VEC>
__device__ __forceinline__ void store_ivec(int* p, const int (&v)[VEC]) {
  if (VEC == 4) {
    *reinterpret_cast<i32x4*>(p) = (i32x4){v[0], v[VEC > 1 ? 1 : 0], v[VEC > 2 ? 2 : 0], v[VEC > 3 ? 3 : 0]};
  } else {
    p[0] = v[0];
  }
}

// Is (v at position l) ahead of (m at position am) in max-pool order?  The greater value; of equal values the earlier
// position; a NaN ahead of every number (the earliest NaN of several).
__device__ __forceinline__ bool ahead(float v, int l, float m, int am) {
  const bool vn = v != v, mn = m != m;
  if (vn || mn) return vn && (!mn || l < am);
  return v > m || (v == m && l < am);
}

// ------------------------------------------------------------------------------------------------------- pooling
struct PoolArgs {
  const float* x; int cs, coff;
  float* out; int out_cs, out_coff;
  int* arg;
  int L, C, CB, mode;
};

template <int VEC>
__global__ __launch_bounds__(256) void stripe_pool_fwd_kernel(const PoolArgs a) {
  __shared__ double rs[TPB * VEC];
  __shared__ float rm[TPB * VEC];
  __shared__ int ra[TPB * VEC];
  const long u = blockIdx.x;
  const int CB = a.CB, C = a.C, L = a.L;
  const int cl = threadIdx.x % CB, rl = threadIdx.x / CB, rpi = TPB / CB;
  const int c = ((int)blockIdx.y * CB + cl) * VEC;
  const bool ok = c < C;
  const float* const xs = a.x + u * (long)L * a.cs + a.coff + c;
  float s[4][VEC], m[VEC];
  int am[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    s[0][e] = s[1][e] = s[2][e] = s[3][e] = 0.f;
    m[e] = -INFINITY;
    am[e] = 0;  // a stripe of nothing but -inf: position 0, as PyTorch's
  }
  if (ok) {
    int l = rl;
    for (; l + 3 * rpi < L; l += 4 * rpi) {  // four positions per trip, the loads issued first
      float v[4][VEC];
#pragma unroll
      for (int q = 0; q < 4; ++q) load_vec<VEC>(xs + (long)(l + q * rpi) * a.cs, true, v[q]);
#pragma unroll
      for (int q = 0; q < 4; ++q)  // increasing positions: a strict comparison keeps the first of equal values
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          s[q][e] += v[q][e];
          if (ahead(v[q][e], l + q * rpi, m[e], am[e])) {
            m[e] = v[q][e];
            am[e] = l + q * rpi;
          }
        }
    }
    for (; l < L; l += rpi) {
      float v[VEC];
      load_vec<VEC>(xs + (long)l * a.cs, true, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        s[0][e] += v[e];
        if (ahead(v[e], l, m[e], am[e])) {
          m[e] = v[e];
          am[e] = l;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    rs[threadIdx.x * VEC + e] = ((double)s[0][e] + (double)s[1][e]) + ((double)s[2][e] + (double)s[3][e]);
    rm[threadIdx.x * VEC + e] = m[e];
    ra[threadIdx.x * VEC + e] = am[e];
  }
  __syncthreads();
  if (rl != 0 || !ok) return;
  // the rpi position lanes of this channel vector, in lane order (lanes past the stripe's end hold 0 / -inf)
  float mean[VEC], mx[VEC];
  int ar[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    double t = 0.0;
    float bm = -INFINITY;
    int ba = 0;
    const int n_l = rpi < L ? rpi : L;
    for (int i = 0; i < n_l; ++i) {
      const int k = (i * CB + cl) * VEC + e;
      t += rs[k];
      if (i == 0 || ahead(rm[k], ra[k], bm, ba)) {
        bm = rm[k];
        ba = ra[k];
      }
    }
    mean[e] = a.mode == SF_STRIPE_SUM ? (float)t : (float)(t / (double)L);
    mx[e] = bm;
    ar[e] = ba;
  }
  float* const o = a.out + u * (long)a.out_cs + a.out_coff + c;
  if (a.mode == SF_STRIPE_MAX) {
    store_vec<VEC>(o, mx);
  } else {
    store_vec<VEC>(o, mean);
    if (a.mode == SF_STRIPE_MEANMAX) store_vec<VEC>(o + C, mx);
  }
  if (a.mode == SF_STRIPE_MAX || a.mode == SF_STRIPE_MEANMAX) store_ivec<VEC>(a.arg + u * (long)C + c, ar);
}

// ------------------------------------------------------------------------------- broadcast add and the backward
struct BcastArgs {
  const float* x; int x_cs, x_coff;        // add: x;  backward: dz (NULL: 0)
  const float* v; int v_cs, v_coff;        // add: v;  backward: dmean (NULL: 0)
  const float* dmax; int dmax_cs, dmax_coff;
  const int* arg;
  float* out; int out_cs, out_coff, out_acc;
  int L, run, P, C, CB, nch;
  float inv_l;
};

// BWD == false: out = x + v.   BWD == true: out (=|+=) x + v * inv_l + [l == arg] * dmax.
template <int VEC, bool BWD>
__global__ __launch_bounds__(256) void stripe_bcast_kernel(const BcastArgs a) {
  const long u = blockIdx.x / a.P;
  const int part = (int)(blockIdx.x - u * a.P);
  const int CB = a.CB, C = a.C;
  const int cl = threadIdx.x % CB, rl = threadIdx.x / CB, rpi = TPB / CB;
  const int r0 = part * a.run;
  const int r1 = (r0 + a.run < a.L) ? r0 + a.run : a.L;
  const long p0 = u * (long)a.L;
  const float* const xs = a.x ? a.x + p0 * a.x_cs + a.x_coff : nullptr;
  float* const os = a.out + p0 * a.out_cs + a.out_coff;
  for (int j = 0; j < a.nch; ++j) {
    const int c = (j * CB + cl) * VEC;
    if (c >= C) continue;
    float vv[VEC], dm[VEC];
    int ar[VEC];
    load_vec<VEC>(a.v + u * (long)a.v_cs + a.v_coff + c, a.v != nullptr, vv);
    if (BWD) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) vv[e] = vv[e] * a.inv_l;
      load_vec<VEC>(a.dmax + u * (long)a.dmax_cs + a.dmax_coff + c, a.dmax != nullptr, dm);
      load_ivec<VEC>(a.arg + u * (long)C + c, a.dmax != nullptr, ar);
    }
    int l = r0 + rl;
    for (; l + 3 * rpi < r1; l += 4 * rpi) {  // four positions per trip, the loads issued first
      float g[4][VEC], pv[4][VEC];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        load_vec<VEC>(xs + (long)(l + q * rpi) * a.x_cs + c, xs != nullptr, g[q]);
        if (BWD) load_vec<VEC>(os + (long)(l + q * rpi) * a.out_cs + c, a.out_acc != 0, pv[q]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float o[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          float fresh = g[q][e] + vv[e];
          if (BWD) {
            fresh = fresh + (ar[e] == l + q * rpi ? dm[e] : 0.f);
            o[e] = a.out_acc ? pv[q][e] + fresh : fresh;
          } else {
            o[e] = fresh;
          }
        }
        store_vec<VEC>(os + (long)(l + q * rpi) * a.out_cs + c, o);
      }
    }
    for (; l < r1; l += rpi) {
      float g[VEC], pv[VEC], o[VEC];
      load_vec<VEC>(xs + (long)l * a.x_cs + c, xs != nullptr, g);
      if (BWD) load_vec<VEC>(os + (long)l * a.out_cs + c, a.out_acc != 0, pv);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float fresh = g[e] + vv[e];
        if (BWD) {
          fresh = fresh + (ar[e] == l ? dm[e] : 0.f);
          o[e] = a.out_acc ? pv[e] + fresh : fresh;
        } else {
          o[e] = fresh;
        }
      }
      store_vec<VEC>(os + (long)l * a.out_cs + c, o);
    }
  }
}

struct Geom { long U; int L; };

// U = N*T*S stripe units of L = (H/S)*W positions; false for what the entry points refuse
bool geom_of(int N, int T, int H, int W, int C, int S, Geom* g) {
  if (N <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || S <= 0 || C > MAX_C) return false;
  if (H % S != 0) return false;
  const long L = (long)(H / S) * W, U = (long)N * T * S;
  if (L > 0x7fffffffL || U > 0x7fffffffL) return false;
  g->U = U;
  g->L = (int)L;
  return true;
}

}  // namespace

extern "C" int sf_stripe_pool_fwd(const float* x, int cs, int coff, int N, int T, int H, int W, int C, int S, int mode,
                                  float* out, int out_cs, int out_coff, void* arg, void* stream) {
  if (!x || !out) return SF_EINVAL;
  if (mode != SF_STRIPE_MEAN && mode != SF_STRIPE_MAX && mode != SF_STRIPE_MEANMAX && mode != SF_STRIPE_SUM)
    return SF_EINVAL;
  const bool want_arg = mode == SF_STRIPE_MAX || mode == SF_STRIPE_MEANMAX;
  if (want_arg && !arg) return SF_EINVAL;
  Geom g;
  if (!geom_of(N, T, H, W, C, S, &g)) return SF_EINVAL;
  const int cout = mode == SF_STRIPE_MEANMAX ? 2 * C : C;
  if (!slice_ok(cs, coff, C) || !slice_ok(out_cs, out_coff, cout)) return SF_EINVAL;
  const bool vec4 = (C % 4 == 0) && vec_ok(x, cs, coff) && vec_ok(out, out_cs, out_coff) &&
                    (!want_arg || sf_aligned16(arg));
  const Layout lay = layout_of(C, vec4);
  if (lay.nch > 65535) return SF_EINVAL;
  PoolArgs a = {};
  a.x = x; a.cs = cs; a.coff = coff; a.out = out; a.out_cs = out_cs; a.out_coff = out_coff;
  a.arg = want_arg ? static_cast<int*>(arg) : nullptr;
  a.L = g.L; a.C = C; a.CB = lay.CB; a.mode = mode;
  const dim3 grid((unsigned)g.U, (unsigned)lay.nch);
  if (vec4)
    hipLaunchKernelGGL(stripe_pool_fwd_kernel<4>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(stripe_pool_fwd_kernel<1>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_stripe_add_fwd(const float* x, int cs, int coff, const float* v, int v_cs, int v_coff, int N, int T,
                                 int H, int W, int C, int S, float* z, int z_cs, int z_coff, void* stream) {
  if (!x || !v || !z) return SF_EINVAL;
  Geom g;
  if (!geom_of(N, T, H, W, C, S, &g)) return SF_EINVAL;
  if (!slice_ok(cs, coff, C) || !slice_ok(v_cs, v_coff, C) || !slice_ok(z_cs, z_coff, C)) return SF_EINVAL;
  const Parts pt = parts_of(g.L);
  if (g.U * pt.P > 0x7fffffffL) return SF_EINVAL;
  const bool vec4 = (C % 4 == 0) && vec_ok(x, cs, coff) && vec_ok(v, v_cs, v_coff) && vec_ok(z, z_cs, z_coff);
  const Layout lay = layout_of(C, vec4);
  BcastArgs a = {};
  a.x = x; a.x_cs = cs; a.x_coff = coff; a.v = v; a.v_cs = v_cs; a.v_coff = v_coff;
  a.out = z; a.out_cs = z_cs; a.out_coff = z_coff;
  a.L = g.L; a.run = pt.run; a.P = pt.P; a.C = C; a.CB = lay.CB; a.nch = lay.nch; a.inv_l = 1.f;
  const dim3 grid((unsigned)(g.U * pt.P));
  if (vec4)
    hipLaunchKernelGGL((stripe_bcast_kernel<4, false>), grid, dim3(TPB), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((stripe_bcast_kernel<1, false>), grid, dim3(TPB), 0, (hipStream_t)stream, a);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_stripe_pool_bwd(const float* dz, int dz_cs, int dz_coff, const float* dmean, int dmean_cs,
                                  int dmean_coff, const float* dmax, int dmax_cs, int dmax_coff, const void* arg, int N,
                                  int T, int H, int W, int C, int S, float* dx, int dx_cs, int dx_coff, int accumulate,
                                  void* stream) {
  if (!dx) return SF_EINVAL;
  if (dmax && !arg) return SF_EINVAL;
  Geom g;
  if (!geom_of(N, T, H, W, C, S, &g)) return SF_EINVAL;
  if (!slice_ok(dx_cs, dx_coff, C)) return SF_EINVAL;
  if (dz && !slice_ok(dz_cs, dz_coff, C)) return SF_EINVAL;
  if (dmean && !slice_ok(dmean_cs, dmean_coff, C)) return SF_EINVAL;
  if (dmax && !slice_ok(dmax_cs, dmax_coff, C)) return SF_EINVAL;
  const Parts pt = parts_of(g.L);
  if (g.U * pt.P > 0x7fffffffL) return SF_EINVAL;
  const bool vec4 = (C % 4 == 0) && vec_ok(dx, dx_cs, dx_coff) && (!dz || vec_ok(dz, dz_cs, dz_coff)) &&
                    (!dmean || vec_ok(dmean, dmean_cs, dmean_coff)) &&
                    (!dmax || (vec_ok(dmax, dmax_cs, dmax_coff) && sf_aligned16(arg)));
  const Layout lay = layout_of(C, vec4);
  BcastArgs a = {};
  a.x = dz; a.x_cs = dz_cs; a.x_coff = dz_coff; a.v = dmean; a.v_cs = dmean_cs; a.v_coff = dmean_coff;
  a.dmax = dmax; a.dmax_cs = dmax_cs; a.dmax_coff = dmax_coff; a.arg = dmax ? static_cast<const int*>(arg) : nullptr;
  a.out = dx; a.out_cs = dx_cs; a.out_coff = dx_coff; a.out_acc = accumulate ? 1 : 0;
  a.L = g.L; a.run = pt.run; a.P = pt.P; a.C = C; a.CB = lay.CB; a.nch = lay.nch; a.inv_l = 1.f / (float)g.L;
  const dim3 grid((unsigned)(g.U * pt.P));
  if (vec4)
    hipLaunchKernelGGL((stripe_bcast_kernel<4, true>), grid, dim3(TPB), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((stripe_bcast_kernel<1, true>), grid, dim3(TPB), 0, (hipStream_t)stream, a);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
