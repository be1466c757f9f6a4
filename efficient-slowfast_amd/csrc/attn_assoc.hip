// attn_assoc.hip — the Nonlocal block's "dot_product" instantiation in its associative form
// (M/nonlocal_helper.py:105-148):
//   Y = (theta phi^T / N_k) g = theta (phi^T g / N_k)          theta [N_q,d]   phi [N_k,d]   g [N_k,dv]
// There is no softmax between the two products, so the N_q x N_k scores never need to exist: M = phi^T g / N_k is one
// d x dv matrix per sample, and the backward is three more products of the same two shapes around D = theta^T dY.
// fp32 in and out on v_mfma_f32_32x32x2_f32, tile products of attn_tile.h.  Every output element has one owner and a
// fixed summation order: no float atomics, two runs give the same bits.
//
// gram:   G[b] = alpha A[b]^T B[b]   A [B,R,da], B [B,R,db] views, G [B,da,db] dense (and G^T [B,db,da] when asked).
//   The reduction runs over the R rows.  One WAVEFRONT owns NB 32 x 32 output tiles of one 32-column block of B: it
//   reads the B tile column[lane & 31] of rows xrow(r, h) into accumulator layout and multiplies by the A tiles read
//   the same way (xacc_t) — 128-byte row segments of both operands, no LDS, no barrier.  G is stored one row segment per
//   register, G^T as float4 rows (xstore_t) from the same registers, so G^T is the exact transpose.
//   Few output tiles (Fast-pathway widths): R is cut into S chunks of whole 32-row tiles, every chunk writes its
//   partial plane ws[s][b][da][db], and a finish pass sums the planes in chunk order.  S depends on (R, da, db) only —
//   not on B — so the bits of a sample do not depend on the batch it is in.
// rowmat: Y[b,r,j] (+)= alpha sum_i X[b,r,i] W[b,j,i]   X [B,R,k] view, W [B,n,k] dense ("weight layout"), Y view.
//   Both operands reduce along contiguous floats.  One workgroup = 4 wavefronts = 32 rows of X, stationary in registers
//   and cut over the wavefronts along k (xload_slice), marching over 32-row tiles of W with the next tile's loads in
//   flight; the four partial tiles meet in LDS (alternating buffers, one barrier per tile) and wavefront w sums and
//   stores rows 8w .. 8w+7 of the tile: 128-byte segments of Y, one owner per element.
#include "common.h"
#include "attn_tile.h"

namespace {

constexpr long ASSOC_MAX_ROWS = (1L << 31) - 32;

struct GramArgs {
  const float* a; const float* b;
  float* g; float* gt; float* ws;
  int a_cs, b_cs, da, db, tiles_a, splits;
  long R, chunk;
  float alpha;
};

// grid: x = column block of B * groups of NB column blocks of A, y = chunk, z = sample; 64 threads
template <int NB>
__global__ __launch_bounds__(64) void gram_kernel(GramArgs a) {
  const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
  const int b = blockIdx.z, s = blockIdx.y;
  const int groups = (a.tiles_a + NB - 1) / NB;
  const int j0 = (blockIdx.x / groups) * 32, i0 = (blockIdx.x % groups) * (32 * NB);
  const float* __restrict__ A = a.a + (long)b * a.R * a.a_cs;
  const float* __restrict__ Bm = a.b + (long)b * a.R * a.b_cs;
  const long r_begin = (long)s * a.chunk;
  const long r_end = r_begin + a.chunk < a.R ? r_begin + a.chunk : a.R;
  const int colb = j0 + c;
  const bool cv = colb < a.db;

  f32x16 acc[NB];
  xzero<NB>(acc);
  for (long row0 = r_begin; row0 < r_end; row0 += 32) {
    f32x16 p;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long row = row0 + xrow(r, h);
      float v = 0.f;
      if (row < r_end && cv) v = Bm[row * a.b_cs + colb];
      p[r] = v;
    }
    xacc_t<NB>(acc, A, a.a_cs, row0, r_end, i0, a.da, p, h, c);  // G[i0 + ..][j0 + c] += A^T B
  }

  const long plane = (long)a.da * a.db;
  if (a.splits > 1) {  // partial plane, unscaled; the finish pass owns G and G^T
    float* __restrict__ P = a.ws + ((long)s * gridDim.z + b) * plane;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = i0 + 32 * nb + xrow(r, h);
        if (i < a.da && cv) P[(long)i * a.db + colb] = acc[nb][r];
      }
    return;
  }
  float* __restrict__ G = a.g + (long)b * plane;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + 32 * nb + xrow(r, h);
      if (i < a.da && cv) G[(long)i * a.db + colb] = acc[nb][r] * a.alpha;
    }
  if (a.gt) xstore_t<NB>(acc, a.gt + (long)b * plane, (long)colb * a.da, cv, i0, a.da, a.alpha, false, h);
}

// G[b][i][j] = alpha (((P_0 + P_1) + P_2) + ...), G^T[b][j][i] the same value; one thread per element
__global__ __launch_bounds__(256) void gram_finish_kernel(GramArgs a, int B) {
  const long plane = (long)a.da * a.db;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= plane * B) return;
  float sum = a.ws[e];
  for (int s = 1; s < a.splits; ++s) sum += a.ws[(long)s * B * plane + e];
  sum *= a.alpha;
  a.g[e] = sum;
  if (a.gt) {
    const long b = e / plane, ij = e % plane;
    const int i = (int)(ij / a.db), j = (int)(ij % a.db);
    a.gt[b * plane + (long)j * a.da + i] = sum;
  }
}

struct RowmatArgs {
  const float* x; const float* w;
  float* y;
  int x_cs, y_cs, k, n, accumulate;
  long R;
  float alpha;
};

// grid: x = 32-row tile of X, y = sample; 256 threads
template <int WK>
__global__ __launch_bounds__(256) void rowmat_kernel(RowmatArgs a) {
  constexpr int KS = WK / 4;
  __shared__ float red[2][4096];  // alternating buffers: one barrier per tile of W
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
  const int b = blockIdx.y;
  const long r0 = (long)blockIdx.x * 32;
  const float* __restrict__ X = a.x + (long)b * a.R * a.x_cs;
  const float* __restrict__ W = a.w + (long)b * a.n * a.k;
  float* __restrict__ Y = a.y + (long)b * a.R * a.y_cs;
  const int e0 = w * KS + h * (KS / 2);

  float xs[KS / 2], ws[KS / 2];
  xload_slice<KS>(X, (r0 + c) * a.x_cs, r0 + c < a.R, e0, a.k, xs);
  xload_slice<KS>(W, (long)c * a.k, c < a.n, e0, a.k, ws);
  const int njt = (a.n + 31) / 32;
  for (int jt = 0; jt < njt; ++jt) {
    const int j0 = jt * 32;
    float wn[KS / 2];  // the next tile of W (rows past n: zeros, nothing read)
    xload_slice<KS>(W, (long)(j0 + 32 + c) * a.k, j0 + 32 + c < a.n, e0, a.k, wn);
    const f32x16 s = xdot<KS>(xs, ws);  // rows (registers) = rows of X, column (lane) = row j of W
    float* buf = red[jt & 1];
    xput(buf, w, lane, s);
    __syncthreads();
    const int col = j0 + c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 4 * w + q;
      const long row = r0 + xrow(r, h);
      float t = ((buf[r * 64 + lane] + buf[1024 + r * 64 + lane]) + buf[2048 + r * 64 + lane]) +
                buf[3072 + r * 64 + lane];
      t *= a.alpha;
      if (row < a.R && col < a.n) {
        float* p = Y + row * a.y_cs + col;
        if (a.accumulate) t += *p;
        *p = t;
      }
    }
#pragma unroll
    for (int t = 0; t < KS / 2; ++t) ws[t] = wn[t];
  }
}

bool view_ok(const void* p, int cs) { return sf_aligned16(p) && cs % 4 == 0; }
bool width_ok(int w) { return w >= 4 && w <= 512 && w % 4 == 0; }

// Chunks of R for gram: none while one sample alone has 64 output tiles (256 x 256: with the batch that fills the
// chip, and a chunked 512 x 512 plane set would outgrow the score matrix it replaces); below that about 256
// wavefronts per sample, every chunk a whole number of 32-row tiles and at least 64 rows.
int gram_plan(long R, int da, int db, long* chunk_out) {
  const int tiles = sf_cdiv(da, 32) * sf_cdiv(db, 32);
  long want = tiles >= 64 ? 1 : (256 + tiles - 1) / tiles;
  const long most = (R + 63) / 64;
  if (want > most) want = most;
  if (want < 1) want = 1;
  const long chunk = ((R + want - 1) / want + 31) / 32 * 32;
  if (chunk_out) *chunk_out = chunk;
  return (int)((R + chunk - 1) / chunk);
}

}  // namespace

extern "C" int sf_assoc_accepts(long Nq, long Nk, int d, int dv) {
  return Nq >= 1 && Nk >= 1 && Nq <= ASSOC_MAX_ROWS && Nk <= ASSOC_MAX_ROWS && width_ok(d) && width_ok(dv) ? 1 : 0;
}

extern "C" int sf_gram_splits(int B, long R, int da, int db) {
  if (B < 1 || R < 1 || R > ASSOC_MAX_ROWS || !width_ok(da) || !width_ok(db)) return 1;
  return gram_plan(R, da, db, nullptr);
}

extern "C" long sf_gram_ws_floats(int B, long R, int da, int db) {
  const int S = sf_gram_splits(B, R, da, db);
  return S > 1 && B > 0 ? (long)S * B * da * db : 0;
}

extern "C" int sf_gram(const float* a, int a_cs, const float* b, int b_cs, float* g, float* gt, int B, long R, int da,
                       int db, float alpha, float* ws, void* stream) {
  if (!a || !b || !g || B <= 0 || B > 65535 || R <= 0) return SF_EINVAL;
  if (R > ASSOC_MAX_ROWS || !width_ok(da) || !width_ok(db)) return SF_ENOTTAKEN;
  if (a_cs < da || b_cs < db) return SF_EINVAL;
  if (!view_ok(a, a_cs) || !view_ok(b, b_cs) || !sf_aligned16(g) || !sf_aligned16(gt)) return SF_EALIGN;
  GramArgs k = {};
  k.splits = gram_plan(R, da, db, &k.chunk);
  if (k.splits > 1 && !ws) return SF_EINVAL;
  if (k.splits > 1 && !sf_aligned16(ws)) return SF_EALIGN;
  k.a = a; k.b = b; k.g = g; k.gt = gt; k.ws = ws;
  k.a_cs = a_cs; k.b_cs = b_cs; k.da = da; k.db = db; k.tiles_a = sf_cdiv(da, 32);
  k.R = R; k.alpha = alpha;
  hipStream_t s = (hipStream_t)stream;
  const int tiles_b = sf_cdiv(db, 32);
  // two tiles per wavefront where that still leaves a wavefront for every SIMD of the chip (512 x 512 with 8 samples)
  const bool two = k.tiles_a % 2 == 0 && (long)k.tiles_a * tiles_b * B * k.splits >= 2048;
  if (two) {
    hipLaunchKernelGGL((gram_kernel<2>), dim3((unsigned)(tiles_b * (k.tiles_a / 2)), (unsigned)k.splits, (unsigned)B),
                       dim3(64), 0, s, k);
  } else {
    hipLaunchKernelGGL((gram_kernel<1>), dim3((unsigned)(tiles_b * k.tiles_a), (unsigned)k.splits, (unsigned)B),
                       dim3(64), 0, s, k);
  }
  SF_CHECK_LAUNCH();
  if (k.splits > 1) {
    const long n = (long)B * da * db;
    hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, k, B);
    SF_CHECK_LAUNCH();
  }
  return SF_OK;
}

extern "C" int sf_rowmat(const float* x, int x_cs, const float* w, float* y, int y_cs, int B, long R, int k, int n,
                         float alpha, int accumulate, void* stream) {
  if (!x || !w || !y || B <= 0 || B > 65535 || R <= 0) return SF_EINVAL;
  if (R > ASSOC_MAX_ROWS || !width_ok(k) || !width_ok(n)) return SF_ENOTTAKEN;
  if (x_cs < k || y_cs < n) return SF_EINVAL;
  if (!view_ok(x, x_cs) || !view_ok(y, y_cs) || !sf_aligned16(w)) return SF_EALIGN;
  RowmatArgs a = {};
  a.x = x; a.w = w; a.y = y; a.x_cs = x_cs; a.y_cs = y_cs; a.k = k; a.n = n; a.accumulate = accumulate ? 1 : 0;
  a.R = R; a.alpha = alpha;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((R + 31) / 32), (unsigned)B);
  if (k <= 64) hipLaunchKernelGGL((rowmat_kernel<64>), grid, dim3(256), 0, s, a);
  else if (k <= 128) hipLaunchKernelGGL((rowmat_kernel<128>), grid, dim3(256), 0, s, a);
  else if (k <= 256) hipLaunchKernelGGL((rowmat_kernel<256>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((rowmat_kernel<512>), grid, dim3(256), 0, s, a);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
