// grad_clip.hip — torch/nn/utils/clip_grad.py (clip_grad_norm_, clip_grad_value_) between the backward pass and the
// optimizer's step, addressed like sf_sgd_step: an int64 table of (gradient address, numel) rows and the (tensor, first
// element) chunk list tiled at sf_sgd_chunk_elems(), one workgroup per chunk.
//   sf_grad_norm   two launches: a partial per chunk (fp64, fixed order), then ONE workgroup that folds the partials
//                  in a fixed order and leaves norm, coefficient, non-finite flag and guard in a state block in device
//                  memory (and the norm in column 7 of the step's ring row).  No atomics, no "last block" finish.
//   sf_grad_scale  g *= coefficient; returns without touching memory when the guard is raised or the coefficient is 1.
//   sf_grad_clamp  g = min(max(g, -v), v), torch.clamp's bits.
// Nothing here needs the host: max_norm / the clamp value are read from device memory, and every scalar the next
// kernel needs stays there, so clip + step replay inside a captured graph.
#include "chunk_table.h"
#include "common.h"
#include "stats_row.h"

#include <math.h>

namespace {
constexpr int GC_TAB_ROW = 2;  // gradient address, numel

// the chunk of this workgroup: its first element and length, or nullptr for a chunk chunk_resolve refuses or a gradient
// address that is null or off 4 bytes
__device__ __forceinline__ float* chunk_of(const long* __restrict__ table, const long* __restrict__ chunks, int n_tensors,
                                           int* len) {
  Chunk c;
  if (!chunk_resolve(table, chunks, n_tensors, GC_TAB_ROW, 1, &c)) return nullptr;
  const long addr = c.row[0];
  if (addr == 0 || (addr & 3) != 0) return nullptr;
  *len = c.len;
  return as_global(addr) + c.start;
}

// max with NaN propagating (torch.max): fmaxf drops a NaN
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }
__device__ __forceinline__ double max_nan(double a, double b) {
  return (a != a || b != b) ? (double)NAN : (a > b ? a : b);
}
// how two partial results of the norm combine: the greater (inf norm) or the sum (L2), in span_reduce's order and
// block_fold's
template <bool INF>
struct NormFold {
  __device__ __forceinline__ double operator()(double a, double b) const { return INF ? max_nan(a, b) : a + b; }
};
struct AbsMax {  // span_reduce: the inf norm's element step
  __device__ __forceinline__ float operator()(float top, float v) const { return max_nan(top, fabsf(v)); }
};

// Pass 1: span_reduce over the chunk (the partial does not depend on the gradient's alignment), then block_fold.
template <bool INF>
__global__ __launch_bounds__(CHUNK_TPB) void grad_norm_partial_kernel(const long* __restrict__ table,
                                                                   const long* __restrict__ chunks, int n_tensors,
                                                                   double* __restrict__ partials) {
  int len = 0;
  const float* g = chunk_of(table, chunks, n_tensors, &len);
  if (g == nullptr) {  // block-uniform
    if (threadIdx.x == 0) partials[blockIdx.x] = 0.0;
    return;
  }
  double r[1];
  if (INF)
    r[0] = (double)span_reduce(g, len, 0.f, AbsMax());
  else
    r[0] = span_reduce(g, len, 0.0, SumSq());
  block_fold(r, NormFold<INF>());
  if (threadIdx.x == 0) partials[blockIdx.x] = r[0];
}

// Pass 2, ONE workgroup: thread t folds partials t, t + 256, ... in order, then block_fold.  Thread 0 writes the state.
template <bool INF>
__global__ __launch_bounds__(CHUNK_TPB) void grad_norm_finish_kernel(const double* __restrict__ partials, int n_chunks,
                                                                  const float* __restrict__ max_norm,
                                                                  const float* __restrict__ guard_in,
                                                                  float* __restrict__ state, float* __restrict__ ring,
                                                                  const int* __restrict__ counter, int cap) {
  const NormFold<INF> comb;
  double v[1] = {0.0};
  for (int i = threadIdx.x; i < n_chunks; i += CHUNK_TPB) v[0] = comb(v[0], partials[i]);
  block_fold(v, comb);
  if (threadIdx.x != 0) return;
  const double tot = v[0];
  const double norm = INF ? tot : sqrt(tot);
  const float norm32 = (float)norm;
  const bool bad = !isfinite(norm);
  // torch: clip_coef = max_norm / (total_norm + 1e-6), clamped at 1 — here in fp64, rounded once.  No max_norm, one
  // that is not positive (the Python side refuses it) or a norm that is not finite: 1, the scale pass does nothing.
  float coef = 1.f;
  if (max_norm != nullptr && !bad) {
    const double mx = (double)max_norm[0];
    if (mx > 0.0) {
      const double c = mx / (norm + 1e-6);
      coef = (float)(c < 1.0 ? c : 1.0);
    }
  }
  const bool raised = guard_in != nullptr && guard_in[0] != 0.f;  // NaN != 0: raised
  *reinterpret_cast<double*>(state) = norm;
  state[ST_NORM32] = norm32;
  state[ST_COEF] = coef;
  state[ST_FLAG] = bad ? 1.f : 0.f;
  state[ST_GUARD] = (raised || bad) ? 1.f : 0.f;
  if (ring != nullptr && counter != nullptr) {
    const int step = counter[0];
    if (step > 0) {  // the row the step's loss kernel wrote; its column 7 is 0 until now
      const int slot = (step - 1) % cap;
      ring[(long)slot * RING_ROW + 7] = norm32;
    }
  }
}

__global__ __launch_bounds__(CHUNK_TPB) void grad_scale_kernel(const long* __restrict__ table,
                                                            const long* __restrict__ chunks, int n_tensors,
                                                            const float* __restrict__ state) {
  const float coef = state[ST_COEF];
  // the guard is raised (a loss or a gradient that is not finite), or nothing to clip: g * 1.0f is g, so not writing is
  // exact.  Anything that is not a coefficient in [0, 1) — a NaN, a state nobody wrote — moves nothing either.
  if (state[ST_GUARD] != 0.f || !(coef >= 0.f && coef < 1.f)) return;
  int len = 0;
  float* g = chunk_of(table, chunks, n_tensors, &len);
  if (g == nullptr) return;
  if (((unsigned long)g & 15) == 0) {
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += CHUNK_TPB) {
      f32x4 v = reinterpret_cast<f32x4*>(g)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= coef;
      reinterpret_cast<f32x4*>(g)[i] = v;
    }
    const int i = (n4 << 2) + threadIdx.x;  // up to three elements left
    if (i < len) g[i] *= coef;
  } else {
    for (int i = threadIdx.x; i < len; i += CHUNK_TPB) g[i] *= coef;
  }
}

// torch.clamp(g, -v, v): a NaN fails both comparisons and passes, -0.0 is inside and keeps its sign
__device__ __forceinline__ float clamp1(float g, float v) { return g < -v ? -v : (g > v ? v : g); }

__global__ __launch_bounds__(CHUNK_TPB) void grad_clamp_kernel(const long* __restrict__ table,
                                                            const long* __restrict__ chunks, int n_tensors,
                                                            const float* __restrict__ value) {
  const float v = value[0];
  if (!(v > 0.f)) return;  // not positive, or a NaN (the Python side refuses both): nothing moves
  int len = 0;
  float* g = chunk_of(table, chunks, n_tensors, &len);
  if (g == nullptr) return;
  if (((unsigned long)g & 15) == 0) {
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += CHUNK_TPB) {
      const f32x4 x = reinterpret_cast<f32x4*>(g)[i];
      f32x4 y;
      bool moved = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        y[e] = clamp1(x[e], v);
        moved |= x[e] < -v || x[e] > v;
      }
      if (moved) reinterpret_cast<f32x4*>(g)[i] = y;  // elements inside the range are not written again
    }
    const int i = (n4 << 2) + threadIdx.x;  // up to three elements left
    if (i < len && (g[i] < -v || g[i] > v)) g[i] = clamp1(g[i], v);
  } else {
    for (int i = threadIdx.x; i < len; i += CHUNK_TPB)
      if (g[i] < -v || g[i] > v) g[i] = clamp1(g[i], v);
  }
}

bool clip_tables_ok(const long* tab, int n_tensors, const long* chunks, int n_chunks) {
  for (int t = 0; t < n_tensors; ++t) {
    const long* r = tab + (long)t * GC_TAB_ROW;
    if (r[0] == 0 || (r[0] & 3) != 0 || r[1] <= 0) return false;
  }
  return chunks_tile(tab, GC_TAB_ROW, 1, n_tensors, chunks, n_chunks);
}

bool clip_args_ok(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
                  int n_chunks) {
  return tables_args_ok(table_host, table, n_tensors, chunks_host, chunks, n_chunks) &&
         clip_tables_ok(table_host, n_tensors, chunks_host, n_chunks);
}
}  // namespace

extern "C" int sf_grad_norm(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                            const long* chunks, int n_chunks, int norm_type, const float* max_norm,
                            const float* guard_in, double* partials, float* state, float* ring, int* counter, int cap,
                            void* stream) {
  if (!clip_args_ok(table_host, table, n_tensors, chunks_host, chunks, n_chunks)) return SF_EINVAL;
  if (!partials || !state || (norm_type != SF_NORM_L2 && norm_type != SF_NORM_INF)) return SF_EINVAL;
  if ((ring != nullptr) != (counter != nullptr) || (ring != nullptr && cap <= 0)) return SF_EINVAL;
  if ((reinterpret_cast<uintptr_t>(partials) & 7) != 0 || (reinterpret_cast<uintptr_t>(state) & 7) != 0)
    return SF_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  if (norm_type == SF_NORM_INF) {
    hipLaunchKernelGGL(grad_norm_partial_kernel<true>, dim3(n_chunks), dim3(CHUNK_TPB), 0, s, table, chunks, n_tensors,
                       partials);
    SF_CHECK_LAUNCH();
    hipLaunchKernelGGL(grad_norm_finish_kernel<true>, dim3(1), dim3(CHUNK_TPB), 0, s, partials, n_chunks, max_norm,
                       guard_in, state, ring, counter, cap);
  } else {
    hipLaunchKernelGGL(grad_norm_partial_kernel<false>, dim3(n_chunks), dim3(CHUNK_TPB), 0, s, table, chunks, n_tensors,
                       partials);
    SF_CHECK_LAUNCH();
    hipLaunchKernelGGL(grad_norm_finish_kernel<false>, dim3(1), dim3(CHUNK_TPB), 0, s, partials, n_chunks, max_norm,
                       guard_in, state, ring, counter, cap);
  }
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_grad_scale(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                             const long* chunks, int n_chunks, const float* state, void* stream) {
  if (!clip_args_ok(table_host, table, n_tensors, chunks_host, chunks, n_chunks) || !state) return SF_EINVAL;
  if ((reinterpret_cast<uintptr_t>(state) & 7) != 0) return SF_EALIGN;
  hipLaunchKernelGGL(grad_scale_kernel, dim3(n_chunks), dim3(CHUNK_TPB), 0, (hipStream_t)stream, table, chunks, n_tensors,
                     state);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_grad_clamp(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                             const long* chunks, int n_chunks, const float* value, void* stream) {
  if (!clip_args_ok(table_host, table, n_tensors, chunks_host, chunks, n_chunks) || !value) return SF_EINVAL;
  hipLaunchKernelGGL(grad_clamp_kernel, dim3(n_chunks), dim3(CHUNK_TPB), 0, (hipStream_t)stream, table, chunks, n_tensors,
                     value);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
