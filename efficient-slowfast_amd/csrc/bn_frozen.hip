// bn_frozen.hip — backward of an eval-mode ("frozen") BatchNorm3d epilogue under a training tape (NDHWC, fp32, gfx950):
//   y = act(gamma * (z - mean) * invstd + beta + res), mean / invstd from the RUNNING statistics, y repeated `rep` times
//   along T (misc.py:246-254 frozen_bn_stats puts every BatchNorm3d into eval(); torch.nn.BatchNorm3d eval semantics).
// With constant statistics dz does not depend on the per-channel sums, so — unlike the training-mode pair
// sf_bn_bwd_reduce / sf_bn_bwd_apply (backward.hip), which must finish the reduction before the apply pass can start —
// ONE pass over the activation does everything: g = sum_q dy * m; dz = gamma * invstd * g (over z); dres (=|+=) g; and
// per-block partial sums of (g, g * xhat).  A small second kernel adds the partials in a fixed order, in fp64, and
// accumulates into dbeta / dgamma.  No atomics, one owner per output element: bitwise reproducible.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int FROZEN_MAX_P = 1024;  // row blocks = partials per channel; the workspace is sf_bn_bwd_ws_floats(C)

inline int pow2ceil_f(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

struct FrozenArgs {
  const float* dy; int dy_cs, dy_coff;
  const float* y; int y_cs, y_coff;   // relu == 3: the byte mask [rows][C/4]
  const float* z; int z_cs, z_coff;   // may alias dz element for element
  float* dz; int dz_cs, dz_coff;
  float* dres; int dres_cs, dres_coff, dres_acc;
  const float* mean; const float* invstd; const float* gamma;  // gamma NULL: no affine (1)
  float* partial;                     // [P][2][C], NULL: no parameter gradients wanted
  long rows, THW; int HW, C, rep, relu, CB;
};

// g[e] = sum_{q<rep} dy[n, t*rep+q, hw, c+e] * m(n, t*rep, hw, c+e)  (the mask of the first copy: the copies are equal)
template <int VEC>
__device__ __forceinline__ void frozen_g(const FrozenArgs& a, long r, int c, float (&g)[VEC]) {
  long r0 = r;
  if (a.rep > 1) {
    const long n = r / a.THW, rem = r - n * a.THW;
    const long t = rem / a.HW, hw = rem - t * a.HW;
    r0 = (n * (a.THW / a.HW) * a.rep + t * a.rep) * a.HW + hw;
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) g[e] = 0.f;
  for (int q = 0; q < a.rep; ++q) {
    const float* d = a.dy + (r0 + (long)q * a.HW) * a.dy_cs + a.dy_coff + c;
    if (VEC == 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(d);
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] += v[e];
    } else {
      g[0] += d[0];
    }
  }
  if (a.relu == 3) {
    if (VEC == 4) {
      const unsigned mk = reinterpret_cast<const unsigned char*>(a.y)[r0 * a.y_cs + (c >> 2)];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (!((mk >> e) & 1u)) g[e] = 0.f;
    }
  } else if (a.relu) {
    const float* yp = a.y + r0 * a.y_cs + a.y_coff + c;
    if (VEC == 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(yp);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (!(v[e] > 0.f) || (a.relu == 2 && !(v[e] < 6.f))) g[e] = 0.f;
    } else if (!(yp[0] > 0.f) || (a.relu == 2 && !(yp[0] < 6.f))) {
      g[0] = 0.f;
    }
  }
}

// Row-block layout of the per-channel reductions of backward.hip: CB lanes cover the C/VEC channel vectors of a row,
// TPB/CB rows per iteration, gridDim.x = P row blocks, gridDim.y channel groups.  A thread owns its (row, channel
// vector) elements: it reads dy, the mask and z, writes dz (and dres) and keeps the two running sums in registers.
template <int VEC>
__global__ __launch_bounds__(256) void bn_frozen_bwd_kernel(const FrozenArgs a) {
  __shared__ float red[2 * TPB * VEC];
  const int blk = blockIdx.x, cb = blockIdx.y, P = gridDim.x;
  const int CB = a.CB, C = a.C;
  const int cl = threadIdx.x % CB, rl = threadIdx.x / CB, rpi = TPB / CB;
  const int c = (cb * CB + cl) * VEC;
  const long per = (a.rows + P - 1) / P;
  const long r0 = (long)blk * per;
  const long r1 = (r0 + per < a.rows) ? r0 + per : a.rows;
  float s1[VEC], s2[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
  if (c < C) {
    float mu[VEC], is[VEC], k[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      mu[e] = a.mean[c + e];
      is[e] = a.invstd[c + e];
      k[e] = a.gamma ? a.gamma[c + e] * is[e] : is[e];
    }
    long r = r0 + rl;
    if constexpr (VEC == 4) if (a.rep == 1 && (a.relu == 0 || a.relu == 3)) {
      // four rows per trip, every load issued before the first use or store (dz may alias z and dres may alias dy
      // element for element: this thread alone touches these elements, and it has read all of them by then)
      const unsigned char* const mk = reinterpret_cast<const unsigned char*>(a.y);
      for (; r + 3 * (long)rpi < r1; r += 4 * (long)rpi) {
        f32x4 gv[4], zq[4], rv[4];
        unsigned mb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const long ru = r + (long)u * rpi;
          gv[u] = *reinterpret_cast<const f32x4*>(a.dy + ru * a.dy_cs + a.dy_coff + c);
          zq[u] = *reinterpret_cast<const f32x4*>(a.z + ru * a.z_cs + a.z_coff + c);
          mb[u] = a.relu == 3 ? mk[ru * a.y_cs + (c >> 2)] : 0xFu;
          if (a.dres && a.dres_acc) rv[u] = *reinterpret_cast<const f32x4*>(a.dres + ru * a.dres_cs + a.dres_coff + c);
          else rv[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const long ru = r + (long)u * rpi;
          f32x4 ov, gg;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            gg[e] = ((mb[u] >> e) & 1u) ? gv[u][e] : 0.f;
            s1[e] += gg[e];
            s2[e] = fmaf(gg[e], (zq[u][e] - mu[e]) * is[e], s2[e]);
            ov[e] = k[e] * gg[e];
          }
          *reinterpret_cast<f32x4*>(a.dz + ru * a.dz_cs + a.dz_coff + c) = ov;
          if (a.dres) *reinterpret_cast<f32x4*>(a.dres + ru * a.dres_cs + a.dres_coff + c) = rv[u] + gg;
        }
      }
    }
    for (; r < r1; r += rpi) {
      float g[VEC], zv[VEC], o[VEC];
      frozen_g<VEC>(a, r, c, g);
      if (VEC == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(a.z + r * a.z_cs + a.z_coff + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) zv[e] = v[e];
      } else {
        zv[0] = a.z[r * a.z_cs + a.z_coff + c];
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        s1[e] += g[e];
        s2[e] = fmaf(g[e], (zv[e] - mu[e]) * is[e], s2[e]);
        o[e] = k[e] * g[e];
      }
      float* dp = a.dz + r * a.dz_cs + a.dz_coff + c;
      if (VEC == 4) {
        *reinterpret_cast<f32x4*>(dp) = (f32x4){o[0], o[1], o[2], o[3]};
      } else {
        dp[0] = o[0];
      }
      if (a.dres) {
        float* rp = a.dres + r * a.dres_cs + a.dres_coff + c;
        if (VEC == 4) {  // dres_acc == 0: first writer of the residual branch's gradient (no zero fill, no read)
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (a.dres_acc) v = *reinterpret_cast<f32x4*>(rp);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += g[e];
          *reinterpret_cast<f32x4*>(rp) = v;
        } else {
          rp[0] = a.dres_acc ? rp[0] + g[0] : g[0];
        }
      }
    }
  }
  if (!a.partial) return;  // no affine parameters: dz (and dres) only
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    red[threadIdx.x * VEC + e] = s1[e];
    red[(TPB + threadIdx.x) * VEC + e] = s2[e];
  }
  __syncthreads();
  if (rl == 0 && c < C) {  // the rpi row lanes of this channel, in lane order
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float t1 = 0.f, t2 = 0.f;
      for (int i = 0; i < rpi; ++i) {
        t1 += red[(i * CB + cl) * VEC + e];
        t2 += red[(TPB + i * CB + cl) * VEC + e];
      }
      a.partial[((long)blk * 2 + 0) * C + c + e] = t1;
      a.partial[((long)blk * 2 + 1) * C + c + e] = t2;
    }
  }
}

// dbeta[c] += sum_i partial[i][0][c], dgamma[c] += sum_i partial[i][1][c]: one wavefront per channel, lane l adds
// partials l, l + 64, ... in fp64, then the 64 lanes are combined by a butterfly — the same order on every run.
__global__ __launch_bounds__(64) void bn_frozen_finish_kernel(const float* __restrict__ partial, int C, int P,
                                                              float* __restrict__ dbeta, float* __restrict__ dgamma) {
  const int c = blockIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int i = threadIdx.x; i < P; i += 64) {
    s1 += (double)partial[((long)i * 2 + 0) * C + c];
    s2 += (double)partial[((long)i * 2 + 1) * C + c];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_xor(s1, off, 64);
    s2 += __shfl_xor(s2, off, 64);
  }
  if (threadIdx.x == 0) {
    dbeta[c] += (float)s1;
    dgamma[c] += (float)s2;
  }
}

bool slice_ok(int cs, int coff, int C) { return coff >= 0 && C <= cs && coff <= cs - C; }

}  // namespace

extern "C" int sf_bn_frozen_bwd(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff,
                                const float* z, int z_cs, int z_coff, int N, int T, int H, int W, int C, int rep,
                                int relu, const float* mean, const float* invstd, const float* gamma, float* dz,
                                int dz_cs, int dz_coff, float* dres, int dres_cs, int dres_coff, int dres_accumulate,
                                float* dbeta, float* dgamma, float* ws, void* stream) {
  if (!dy || !z || !dz || !mean || !invstd) return SF_EINVAL;
  if (N <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || rep <= 0) return SF_EINVAL;
  if (relu < 0 || relu > 3 || (relu && !y)) return SF_EINVAL;
  if ((dbeta == nullptr) != (dgamma == nullptr) || (dbeta && !ws)) return SF_EINVAL;
  if (dres && rep != 1) return SF_EINVAL;
  if (!slice_ok(dy_cs, dy_coff, C) || !slice_ok(z_cs, z_coff, C) || !slice_ok(dz_cs, dz_coff, C)) return SF_EINVAL;
  if ((relu == 1 || relu == 2) && !slice_ok(y_cs, y_coff, C)) return SF_EINVAL;
  if (dres && !slice_ok(dres_cs, dres_coff, C)) return SF_EINVAL;
  if (relu == 3 && (rep != 1 || (C % 4) != 0 || y_cs != C / 4 || y_coff != 0)) return SF_EINVAL;
  if ((long)H * W > 0x7fffffffL) return SF_EINVAL;
  const bool vec4 = (C % 4 == 0) && (dy_cs % 4 == 0) && (dy_coff % 4 == 0) && (z_cs % 4 == 0) && (z_coff % 4 == 0) &&
                    (dz_cs % 4 == 0) && (dz_coff % 4 == 0) && sf_aligned16(dy) && sf_aligned16(z) && sf_aligned16(dz) &&
                    (!relu || relu == 3 || ((y_cs % 4 == 0) && (y_coff % 4 == 0) && sf_aligned16(y))) &&
                    (!dres || ((dres_cs % 4 == 0) && (dres_coff % 4 == 0) && sf_aligned16(dres)));
  if (relu == 3 && !vec4) return SF_EINVAL;  // the byte mask only exists on the float4 path
  FrozenArgs a;
  a.dy = dy; a.dy_cs = dy_cs; a.dy_coff = dy_coff;
  a.y = relu ? y : nullptr; a.y_cs = y_cs; a.y_coff = y_coff;
  a.z = z; a.z_cs = z_cs; a.z_coff = z_coff;
  a.dz = dz; a.dz_cs = dz_cs; a.dz_coff = dz_coff;
  a.dres = dres; a.dres_cs = dres_cs; a.dres_coff = dres_coff; a.dres_acc = dres_accumulate ? 1 : 0;
  a.mean = mean; a.invstd = invstd; a.gamma = gamma;
  a.partial = dbeta ? ws : nullptr;
  a.rows = (long)N * T * H * W; a.THW = (long)T * H * W; a.HW = H * W; a.C = C; a.rep = rep; a.relu = relu;
  // lanes per row, rows per iteration and row blocks: up to 8 iterations per block, at most FROZEN_MAX_P blocks
  const int cv = sf_cdiv(C, vec4 ? 4 : 1);
  a.CB = pow2ceil_f(cv) < TPB ? pow2ceil_f(cv) : TPB;
  const long chunk = (long)(TPB / a.CB) * 8;
  const long p = (a.rows + chunk - 1) / chunk;
  const int P = (int)(p > FROZEN_MAX_P ? FROZEN_MAX_P : p);
  const int ncb = sf_cdiv(cv, a.CB);
  if (vec4)
    hipLaunchKernelGGL(bn_frozen_bwd_kernel<4>, dim3(P, ncb), dim3(TPB), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(bn_frozen_bwd_kernel<1>, dim3(P, ncb), dim3(TPB), 0, (hipStream_t)stream, a);
  if (dbeta)
    hipLaunchKernelGGL(bn_frozen_finish_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, ws, C, P, dbeta, dgamma);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
