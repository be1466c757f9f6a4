// attn_tile.h — the 32 x 32 tile products of v_mfma_f32_32x32x2_f32 shared by attn_cross.hip and attn_assoc.hip.
//   * a product that reduces over the WIDTH of two row-major operands: every lane holds a slice of ONE row in registers
//     (xload_slice: float4 loads, zeros past the width), xdot chains the MFMAs, xput / xget sum the four wavefronts'
//     partial tiles through LDS in wavefront order;
//   * a product that reduces over a tile's 32 ROWS: the B operand lies in accumulator layout (column on the lane, the 16
//     registers = rows xrow(r, h)), the A operand X[that row][column block + lane & 31] comes from global memory
//     (xacc_t); xstore_t writes the transposed result as float4 rows.
// Rows past the row count and elements past the width are zeros in registers, never read from memory.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ int xrow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// elements [e0, e0 + WS/2) of one row (null row: zeros), zero from `width` on
template <int WS>
__device__ __forceinline__ void xload_slice(const float* __restrict__ base, long row_off, bool valid, int e0, int width,
                                            float (&r)[WS / 2]) {
#pragma unroll
  for (int u = 0; u < WS / 8; ++u) {
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    if (valid && e0 + 4 * u < width) t = *reinterpret_cast<const f32x4*>(base + row_off + e0 + 4 * u);
    r[4 * u] = t.x; r[4 * u + 1] = t.y; r[4 * u + 2] = t.z; r[4 * u + 3] = t.w;
  }
}

template <int WS>
__device__ __forceinline__ f32x16 xdot(const float (&a)[WS / 2], const float (&b)[WS / 2]) {
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < WS / 2; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc, 0, 0, 0);
  return acc;
}

// sum of the four wavefronts' partial tiles, in wavefront order, in every wavefront (buf: [4][1024] floats)
__device__ __forceinline__ void xput(float* buf, int w, int lane, const f32x16& s) {
#pragma unroll
  for (int r = 0; r < 16; ++r) buf[w * 1024 + r * 64 + lane] = s[r];
}
__device__ __forceinline__ f32x16 xget(const float* buf, int lane) {
  f32x16 s;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    s[r] = ((buf[r * 64 + lane] + buf[1024 + r * 64 + lane]) + buf[2048 + r * 64 + lane]) + buf[3072 + r * 64 + lane];
  return s;
}

// acc[nb] += X[row0 + xrow(r, h)][col0 + 32 nb + lane&31]^T . p   for the column blocks this wavefront owns
template <int NB>
__device__ __forceinline__ void xacc_t(f32x16 (&acc)[NB], const float* __restrict__ x, int cs, long row0, long nrows,
                                       int col0, int width, const f32x16& p, int h, int c) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (col0 + 32 * nb < width) {  // wave-uniform
      const int col = col0 + 32 * nb + c;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long row = row0 + xrow(r, h);
        float a = 0.f;
        if (row < nrows && col < width) a = x[row * cs + col];
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p[r], acc[nb], 0, 0, 0);
      }
    }
  }
}

// out[row of this lane][col0 + ...] (+)= mul * acc^T: registers 4g .. 4g+3 are four consecutive columns
template <int NB>
__device__ __forceinline__ void xstore_t(const f32x16 (&acc)[NB], float* __restrict__ out, long row_off, bool valid,
                                         int col0, int width, float mul, bool accumulate, int h) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int col = col0 + 32 * nb + 8 * g + 4 * h;
      if (valid && col < width) {
        f32x4* p = reinterpret_cast<f32x4*>(out + row_off + col);
        f32x4 t = {acc[nb][4 * g] * mul, acc[nb][4 * g + 1] * mul, acc[nb][4 * g + 2] * mul, acc[nb][4 * g + 3] * mul};
        if (accumulate) t += *p;
        *p = t;
      }
    }
  }
}

template <int NB>
__device__ __forceinline__ void xzero(f32x16 (&acc)[NB]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
}

}  // namespace
