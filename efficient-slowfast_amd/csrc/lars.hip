// lars.hip — the layer-wise trust ratio of LARS / LARC (upstream SlowFast's SOLVER.LARS_ON, NVIDIA apex's LARC) between
// the backward pass and sf_lars_sgd_step: ||p|| and ||g|| of EVERY tensor of the model in two launches, addressed like
// the optimizers (an int64 table of tensors, the chunk list tiled at sf_sgd_chunk_elems(), so one tensor's chunks are
// contiguous).
//   launch 1   one workgroup per chunk reads its span of p and of g once and leaves sum p^2 and sum g^2 (fp64, the
//              fixed order of grad_clip.hip's norm pass) as two partials.
//   launch 2   one workgroup per tensor folds that tensor's partials in chunk order and writes {r, wd_t}; one more
//              workgroup of the same launch looks at every partial and writes the guard.  Each word has one writer:
//              no atomics, no "last workgroup" finish, equal inputs give equal bits.
// Nothing here needs the host: lr, weight decay, the trust coefficient, eps and the switches are read from device memory.
#include "common.h"
#include "stats_row.h"

#include <math.h>

#include <cmath>

namespace {
constexpr int LR_TPB = 256;
constexpr int LR_WAVES = LR_TPB / 64;
constexpr int LR_CHUNK = 4096;   // == sf_sgd_chunk_elems() (checked at the entry): the optimizers' chunk list serves
constexpr int LR_TAB_ROW = 6;    // parameter, gradient, numel, group, first chunk, ignored (0 / 1)
constexpr int LR_HYP_ROW = 3;    // per group: lr, weight_decay, apply; the row behind them: trust_coefficient, eps, clip
constexpr int ST_FLAG = 4, ST_GUARD = 5;  // sf_grad_norm's state block: [4] non-finite, [5] guard_out

__device__ __forceinline__ const float* as_global(long addr) {
  // the address names global memory (a hipMalloc'ed span): say so, or every access becomes a flat one
  return (const float*)(__attribute__((address_space(1))) const float*)(unsigned long)addr;
}

// two thread-sequential values -> xor butterfly -> wavefronts in order through LDS; thread 0 holds the results
__device__ __forceinline__ void block_fold2(double* a, double* b) {
  __shared__ double s_part[LR_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double va = wave_sum(*a), vb = wave_sum(*b);
  if (lane == 0) {
    s_part[wave][0] = va;
    s_part[wave][1] = vb;
  }
  __syncthreads();
  double ra = s_part[0][0], rb = s_part[0][1];
#pragma unroll
  for (int w = 1; w < LR_WAVES; ++w) {
    ra += s_part[w][0];
    rb += s_part[w][1];
  }
  *a = ra;
  *b = rb;
}

// thread t owns the groups of four elements t, t + 256, ... of the span, element by element in order, then the element
// behind the last whole group (up to three are left).  The 16-byte path and the 4-byte path read the same elements in
// the same order in the same thread: the sum does not depend on the alignment.
__device__ __forceinline__ double span_sumsq(const float* __restrict__ x, int len) {
  double acc = 0.0;
  const int n4 = len >> 2;
  if (((unsigned long)x & 15) == 0) {
    for (int i = threadIdx.x; i < n4; i += LR_TPB) {
      const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += (double)v[e] * (double)v[e];
    }
  } else {
    for (int i = threadIdx.x; i < n4; i += LR_TPB) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = x[4 * i + e];
        acc += (double)v * (double)v;
      }
    }
  }
  const int i = (n4 << 2) + threadIdx.x;
  if (i < len) {
    const float v = x[i];
    acc += (double)v * (double)v;
  }
  return acc;
}

// Launch 1.  partials[2 c] = sum p^2, partials[2 c + 1] = sum g^2 of chunk c; a chunk whose device row fails the checks
// the host entry made on its copy writes two zeros, never a wild access.
__global__ __launch_bounds__(LR_TPB) void lars_partial_kernel(const long* __restrict__ table,
                                                              const long* __restrict__ chunks, int n_tensors,
                                                              double* __restrict__ partials) {
  const long* c = chunks + (long)blockIdx.x * 2;
  const long ti = c[0], start = c[1];
  bool ok = ti >= 0 && ti < n_tensors;  // block-uniform
  long pa = 0, ga = 0, numel = 0;
  if (ok) {
    const long* row = table + ti * LR_TAB_ROW;
    pa = row[0];
    ga = row[1];
    numel = row[2];
    ok = pa != 0 && ga != 0 && ((pa | ga) & 3) == 0 && start >= 0 && start < numel;
  }
  double sp = 0.0, sg = 0.0;
  if (ok) {
    const int len = (int)(numel - start < LR_CHUNK ? numel - start : LR_CHUNK);
    sp = span_sumsq(as_global(pa) + start, len);
    sg = span_sumsq(as_global(ga) + start, len);
  }
  block_fold2(&sp, &sg);
  if (threadIdx.x == 0) {
    partials[2 * (long)blockIdx.x] = sp;
    partials[2 * (long)blockIdx.x + 1] = sg;
  }
}

// Launch 2.  Workgroup t < n_tensors: thread i folds the tensor's partials i, i + 256, ... in chunk order, then the two
// steps above; thread 0 writes ratios[t] = {r, wd_t}, evaluated in fp64 and rounded once.  Workgroup n_tensors: any
// partial that is not finite (a sum of squares in fp64 is finite unless an element is not) raises the guard.
__global__ __launch_bounds__(LR_TPB) void lars_ratio_kernel(const long* __restrict__ table, int n_tensors,
                                                            const float* __restrict__ hyper, int n_groups,
                                                            const double* __restrict__ partials, int n_chunks,
                                                            const float* __restrict__ guard_in,
                                                            float* __restrict__ ratios, float* __restrict__ state) {
  if ((int)blockIdx.x == n_tensors) {
    __shared__ int s_bad[LR_WAVES];
    int bad = 0;
    for (long i = threadIdx.x; i < 2 * (long)n_chunks; i += LR_TPB) bad |= !isfinite(partials[i]);
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0) s_bad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
      int any = 0;
      for (int w = 0; w < LR_WAVES; ++w) any |= s_bad[w];
      const bool raised = guard_in != nullptr && guard_in[0] != 0.f;  // NaN != 0: raised
      state[ST_FLAG] = any ? 1.f : 0.f;
      state[ST_GUARD] = (raised || any) ? 1.f : 0.f;
    }
    return;
  }
  const long t = blockIdx.x;
  const long* row = table + t * LR_TAB_ROW;
  const long numel = row[2], grp = row[3], first = row[4];
  const long nch = numel > 0 ? (numel + LR_CHUNK - 1) / LR_CHUNK : 0;
  // block-uniform: a device row that differs from the checked host copy reads no partial and leaves plain SGD behind
  const bool ok = numel > 0 && grp >= 0 && grp < n_groups && first >= 0 && first <= n_chunks - nch;
  double sp = 0.0, sg = 0.0;
  if (ok) {
    const double* part = partials + 2 * first;
    for (long i = threadIdx.x; i < nch; i += LR_TPB) {
      sp += part[2 * i];
      sg += part[2 * i + 1];
    }
  }
  block_fold2(&sp, &sg);
  if (threadIdx.x != 0) return;
  float r = 1.f, wd_t = 0.f;
  if (ok) {
    const float* hy = hyper + grp * LR_HYP_ROW;
    const float* gl = hyper + (long)n_groups * LR_HYP_ROW;
    const double lr = (double)hy[0], wd = (double)hy[1], trust = (double)gl[0], eps = (double)gl[1];
    const bool apply = hy[2] == 1.f && row[5] == 0, clip = gl[2] == 1.f;
    const double pn = sqrt(sp), gn = sqrt(sg);
    wd_t = hy[1];
    if (apply && isfinite(pn) && isfinite(gn)) {
      if (pn != 0.0 && gn != 0.0) {
        double q = trust * pn / (gn + pn * wd + eps);
        if (clip) {
          q = q / lr;
          q = q < 1.0 ? q : 1.0;  // min(q / lr, 1); a NaN (0 / 0) leaves 1
        }
        r = (float)q;
      } else {
        wd_t = 0.f;  // a zero norm: no scaling and no decay
      }
    }
  }
  ratios[2 * t] = r;
  ratios[2 * t + 1] = wd_t;
}

bool lars_tables_ok(const long* tab, int n_tensors, const long* chunks, int n_chunks, const float* hyper, int n_groups) {
  if (sf_sgd_chunk_elems() != LR_CHUNK) return false;
  for (int g = 0; g < n_groups; ++g) {
    const float a = hyper[g * LR_HYP_ROW + 2];
    if (a != 0.f && a != 1.f) return false;
  }
  const float clip = hyper[n_groups * LR_HYP_ROW + 2];
  if (clip != 0.f && clip != 1.f) return false;
  long first = 0;
  for (int t = 0; t < n_tensors; ++t) {
    const long* r = tab + (long)t * LR_TAB_ROW;
    if (r[0] == 0 || r[1] == 0 || ((r[0] | r[1]) & 3) != 0 || r[2] <= 0) return false;
    if (r[3] < 0 || r[3] >= n_groups || r[4] != first || (r[5] != 0 && r[5] != 1)) return false;
    first += (r[2] + LR_CHUNK - 1) / LR_CHUNK;
  }
  if (first != n_chunks) return false;
  long t = 0, s = 0;  // step_tail.hip::chunks_tile: (0, 0), (0, C), ..., (1, 0), ...
  for (int i = 0; i < n_chunks; ++i) {
    if (t >= n_tensors || chunks[2 * i] != t || chunks[2 * i + 1] != s) return false;
    s += LR_CHUNK;
    if (s >= tab[t * LR_TAB_ROW + 2]) {
      ++t;
      s = 0;
    }
  }
  return t == n_tensors && s == 0;
}
}  // namespace

extern "C" int sf_lars_ratios(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                              const long* chunks, int n_chunks, const float* hyper_host, const float* hyper,
                              int n_groups, const float* guard_in, double* partials, float* ratios, float* state,
                              void* stream) {
  if (!table_host || !table || !chunks_host || !chunks || !hyper_host || !hyper) return SF_EINVAL;
  if (!partials || !ratios || !state || n_tensors <= 0 || n_chunks <= 0 || n_groups <= 0) return SF_EINVAL;
  if (!lars_tables_ok(table_host, n_tensors, chunks_host, n_chunks, hyper_host, n_groups)) return SF_EINVAL;
  if ((reinterpret_cast<uintptr_t>(ratios) & 3) != 0) return SF_EINVAL;
  if ((reinterpret_cast<uintptr_t>(partials) & 7) != 0 || (reinterpret_cast<uintptr_t>(state) & 7) != 0)
    return SF_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lars_partial_kernel, dim3(n_chunks), dim3(LR_TPB), 0, s, table, chunks, n_tensors, partials);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(lars_ratio_kernel, dim3(n_tensors + 1), dim3(LR_TPB), 0, s, table, n_tensors, hyper, n_groups,
                     partials, n_chunks, guard_in, ratios, state);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
