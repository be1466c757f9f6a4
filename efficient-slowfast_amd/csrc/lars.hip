// lars.hip — the layer-wise trust ratio of LARS / LARC (upstream SlowFast's SOLVER.LARS_ON, NVIDIA apex's LARC) between
// the backward pass and sf_lars_sgd_step: ||p|| and ||g|| of EVERY tensor of the model in two launches, addressed like
// the optimizers (an int64 table of tensors, the chunk list tiled at sf_sgd_chunk_elems(), so one tensor's chunks are
// contiguous).
//   launch 1   one workgroup per chunk reads its span of p and of g once and leaves sum p^2 and sum g^2 (fp64, in
//              chunk_table.h's fixed order: span_reduce, then block_fold — what sf_grad_norm uses) as two partials.
//   launch 2   one workgroup per tensor folds that tensor's partials in chunk order and writes {r, wd_t}; one more
//              workgroup of the same launch looks at every partial and writes the guard.  Each word has one writer:
//              no atomics, no "last workgroup" finish, equal inputs give equal bits.
// Nothing here needs the host: lr, weight decay, the trust coefficient, eps and the switches are read from device memory.
#include "chunk_table.h"
#include "common.h"
#include "stats_row.h"

#include <math.h>

#include <cmath>

namespace {
constexpr int LR_TAB_ROW = 6;  // parameter, gradient, numel, group, first chunk, ignored (0 / 1)
constexpr int LR_HYP_ROW = 3;  // per group: lr, weight_decay, apply; the row behind them: trust_coefficient, eps, clip

// Launch 1.  partials[2 c] = sum p^2, partials[2 c + 1] = sum g^2 of chunk c; a chunk whose device row fails the checks
// the host entry made on its copy writes two zeros, never a wild access.
__global__ __launch_bounds__(CHUNK_TPB) void lars_partial_kernel(const long* __restrict__ table,
                                                              const long* __restrict__ chunks, int n_tensors,
                                                              double* __restrict__ partials) {
  Chunk c;
  double s[2] = {0.0, 0.0};  // sum p^2, sum g^2
  if (chunk_resolve(table, chunks, n_tensors, LR_TAB_ROW, 2, &c)) {  // block-uniform
    const long pa = c.row[0], ga = c.row[1];
    if (pa != 0 && ga != 0 && ((pa | ga) & 3) == 0) {
      s[0] = span_reduce(as_global(pa) + c.start, c.len, 0.0, SumSq());
      s[1] = span_reduce(as_global(ga) + c.start, c.len, 0.0, SumSq());
    }
  }
  block_fold(s, Sum());
  if (threadIdx.x == 0) {
    partials[2 * (long)blockIdx.x] = s[0];
    partials[2 * (long)blockIdx.x + 1] = s[1];
  }
}

// Launch 2.  Workgroup t < n_tensors: thread i folds the tensor's partials i, i + 256, ... in chunk order, then
// block_fold; thread 0 writes ratios[t] = {r, wd_t}, evaluated in fp64 and rounded once.  Workgroup n_tensors: any
// partial that is not finite (a sum of squares in fp64 is finite unless an element is not) raises the guard.
__global__ __launch_bounds__(CHUNK_TPB) void lars_ratio_kernel(const long* __restrict__ table, int n_tensors,
                                                            const float* __restrict__ hyper, int n_groups,
                                                            const double* __restrict__ partials, int n_chunks,
                                                            const float* __restrict__ guard_in,
                                                            float* __restrict__ ratios, float* __restrict__ state) {
  if ((int)blockIdx.x == n_tensors) {
    __shared__ int s_bad[CHUNK_WAVES];
    int bad = 0;
    for (long i = threadIdx.x; i < 2 * (long)n_chunks; i += CHUNK_TPB) bad |= !isfinite(partials[i]);
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0) s_bad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
      int any = 0;
      for (int w = 0; w < CHUNK_WAVES; ++w) any |= s_bad[w];
      const bool raised = guard_in != nullptr && guard_in[0] != 0.f;  // NaN != 0: raised
      state[ST_FLAG] = any ? 1.f : 0.f;
      state[ST_GUARD] = (raised || any) ? 1.f : 0.f;
    }
    return;
  }
  const long t = blockIdx.x;
  const long* row = table + t * LR_TAB_ROW;
  const long numel = row[2], grp = row[3], first = row[4];
  const long nch = numel > 0 ? (numel + CHUNK_ELEMS - 1) / CHUNK_ELEMS : 0;
  // block-uniform: a device row that differs from the checked host copy reads no partial and leaves plain SGD behind
  const bool ok = numel > 0 && grp >= 0 && grp < n_groups && first >= 0 && first <= n_chunks - nch;
  double s[2] = {0.0, 0.0};
  if (ok) {
    const double* part = partials + 2 * first;
    for (long i = threadIdx.x; i < nch; i += CHUNK_TPB) {
      s[0] += part[2 * i];
      s[1] += part[2 * i + 1];
    }
  }
  block_fold(s, Sum());
  if (threadIdx.x != 0) return;
  const double sp = s[0], sg = s[1];
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
    first += (r[2] + CHUNK_ELEMS - 1) / CHUNK_ELEMS;
  }
  return first == n_chunks && chunks_tile(tab, LR_TAB_ROW, 2, n_tensors, chunks, n_chunks);
}
}  // namespace

extern "C" int sf_lars_ratios(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                              const long* chunks, int n_chunks, const float* hyper_host, const float* hyper,
                              int n_groups, const float* guard_in, double* partials, float* ratios, float* state,
                              void* stream) {
  if (!tables_args_ok(table_host, table, n_tensors, chunks_host, chunks, n_chunks)) return SF_EINVAL;
  if (!hyper_host || !hyper || !partials || !ratios || !state || n_groups <= 0) return SF_EINVAL;
  if (!lars_tables_ok(table_host, n_tensors, chunks_host, n_chunks, hyper_host, n_groups)) return SF_EINVAL;
  if ((reinterpret_cast<uintptr_t>(ratios) & 3) != 0) return SF_EINVAL;
  if ((reinterpret_cast<uintptr_t>(partials) & 7) != 0 || (reinterpret_cast<uintptr_t>(state) & 7) != 0)
    return SF_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lars_partial_kernel, dim3(n_chunks), dim3(CHUNK_TPB), 0, s, table, chunks, n_tensors, partials);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(lars_ratio_kernel, dim3(n_tensors + 1), dim3(CHUNK_TPB), 0, s, table, n_tensors, hyper, n_groups,
                     partials, n_chunks, guard_in, ratios, state);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
