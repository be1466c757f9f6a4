// weight_avg.hip — a second, averaged copy of the weights behind the optimizer update: the EMA of parameters and BN
// buffers that large-batch recipes evaluate and checkpoint (torch.optim.swa_utils.AveragedModel with
// get_ema_multi_avg_fn), the equal-weight mean of SWA, and the running mean of per-batch statistics of the precise-BN
// pass (utils/precise_bn.py) — one table of tensor pairs, addressed like the optimizers (an int64 table of tensors, the
// chunk list tiled at sf_sgd_chunk_elems(), one workgroup per chunk).
//   sf_avg_update    every pair of the table in ONE launch, then a one-thread launch that advances the count: every
//                    workgroup of the first reads the count the second has not touched yet.
//   sf_avg_exchange  swap / copy the two sides of every pair in ONE launch: evaluation on the averaged weights swaps
//                    them into the model and back, through the model's own packed-weight caches.
// Pure streaming: 12 bytes per averaged element (read both, write one), 16 per swapped one.  Every element has one
// owner and one formula: the 16-byte and the 4-byte path give the same bits, no atomics.
#include "chunk_table.h"
#include "common.h"

#include <math.h>

#include <cmath>

namespace {
constexpr int AVG_TAB_ROW = 4;  // average address, source address, numel, kind
constexpr long KIND_AVG = 0;    // float32, averaged
constexpr long KIND_COPY = 1;   // float32, copied source -> average (a buffer when buffers are not averaged)
constexpr long KIND_WORDS = 2;  // int64 words, copied (num_batches_tracked); numel counts 8-byte words

// The two sides of this workgroup's chunk as float spans (a word is two floats: moved, never computed with).  false
// (block-uniform): the device row fails what the host entry checked on its copy — nothing is touched.
struct Pair {
  float* a;
  float* s;
  int len;
  long kind;
};
__device__ __forceinline__ bool pair_resolve(const long* __restrict__ table, const long* __restrict__ chunks,
                                             int n_tensors, Pair* p) {
  Chunk c;
  if (!chunk_resolve(table, chunks, n_tensors, AVG_TAB_ROW, 2, &c)) return false;
  const long aa = c.row[0], sa = c.row[1], kind = c.row[3];
  if (aa == 0 || sa == 0 || kind < KIND_AVG || kind > KIND_WORDS) return false;
  if (((aa | sa) & (kind == KIND_WORDS ? 7 : 3)) != 0) return false;
  // The row's numel against the chunk list: the tensor's last chunk sits where the numel says and the chunk behind it
  // belongs to another tensor.  A numel that grew or shrank across a chunk boundary behind the host's check switches
  // every chunk of the tensor off; one that moved inside the last chunk's slack cannot be told from the chunk list.
  const long numel = c.row[2];
  if (numel > (1L << 48) || c.start % CHUNK_ELEMS != 0) return false;
  const long n_mine = (numel + CHUNK_ELEMS - 1) / CHUNK_ELEMS;
  const long last = (long)blockIdx.x + (n_mine - 1 - c.start / CHUNK_ELEMS);
  if (last >= (long)gridDim.x) return false;
  if (chunks[2 * last] != c.ti || chunks[2 * last + 1] != (n_mine - 1) * CHUNK_ELEMS) return false;
  if (last + 1 < (long)gridDim.x && chunks[2 * last + 2] == c.ti) return false;
  const long per = kind == KIND_WORDS ? 2 : 1;
  p->a = as_global(aa) + c.start * per;
  p->s = as_global(sa) + c.start * per;
  p->len = c.len * (int)per;
  p->kind = kind;
  return true;
}

// dst[i] = src[i] over a span: 16-byte accesses where both addresses allow, else 4-byte ones — the same bits
__device__ __forceinline__ void span_copy(float* dst, const float* src, int len) {
  if ((((unsigned long)dst | (unsigned long)src) & 15) == 0) {
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += CHUNK_TPB)
      reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
    const int i = (n4 << 2) + threadIdx.x;  // up to three elements left
    if (i < len) dst[i] = src[i];
  } else {
    for (int i = threadIdx.x; i < len; i += CHUNK_TPB) dst[i] = src[i];
  }
}

// f(a[i], s[i]) over a span, a[i] written back and, with WRITE_S, s[i] too; the access widths as in span_copy
template <bool WRITE_S, typename F>
__device__ __forceinline__ void span_pairs(float* a, float* s, int len, F f) {
  if ((((unsigned long)a | (unsigned long)s) & 15) == 0) {
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += CHUNK_TPB) {
      f32x4 av = reinterpret_cast<f32x4*>(a)[i];
      f32x4 sv = reinterpret_cast<f32x4*>(s)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x = av[e], y = sv[e];
        f(x, y);
        av[e] = x;
        sv[e] = y;
      }
      reinterpret_cast<f32x4*>(a)[i] = av;
      if (WRITE_S) reinterpret_cast<f32x4*>(s)[i] = sv;
    }
    const int i = (n4 << 2) + threadIdx.x;  // up to three elements left
    if (i < len) {
      float x = a[i], y = s[i];
      f(x, y);
      a[i] = x;
      if (WRITE_S) s[i] = y;
    }
  } else {
    for (int i = threadIdx.x; i < len; i += CHUNK_TPB) {
      float x = a[i], y = s[i];
      f(x, y);
      a[i] = x;
      if (WRITE_S) s[i] = y;
    }
  }
}

struct Lerp {  // torch's lerp: w < 0.5 ? a + w (s - a) : s - (s - a) (1 - w), each branch one fused multiply-add
  float w, rest;  // rest = 1 - w
  __device__ __forceinline__ void operator()(float& a, float& s) const {
    const float d = s - a;
    a = w < 0.5f ? fmaf(w, d, a) : fmaf(-d, rest, s);
  }
};
// The running mean as torch's GPU kernels evaluate  m += (s - m) / n  for a host number n: the division by a host scalar
// is a multiply by the fp32 reciprocal (ATen's true-divide for a CPU-scalar divisor), and the three tensor operations
// round one by one — subtract, multiply, add, never a fused multiply-add.
struct Mean {
  float inv;  // 1.f / n
  __device__ __forceinline__ void operator()(float& a, float& s) const {
#pragma clang fp contract(off)
    const float d = s - a;
    const float q = d * inv;
    a = a + q;
  }
};
struct Swap {
  __device__ __forceinline__ void operator()(float& a, float& s) const {
    const float t = a;
    a = s;
    s = t;
  }
};

__global__ __launch_bounds__(CHUNK_TPB) void avg_update_kernel(const long* __restrict__ table,
                                                              const long* __restrict__ chunks, int n_tensors, int mode,
                                                              const float* __restrict__ hyper,
                                                              const long* __restrict__ count,
                                                              const float* __restrict__ guard) {
  if (guard != nullptr && guard[0] != 0.f) return;  // the step's loss was not finite (or NaN itself): nothing moves
  Pair p;
  if (!pair_resolve(table, chunks, n_tensors, &p)) return;
  const long n = count[0];  // advanced by avg_tick_kernel, the launch behind this one
  if (n < 0) return;
  if (p.kind != KIND_AVG || n == 0) {  // the first update is a copy, as in torch
    span_copy(p.a, p.s, p.len);
    return;
  }
  const float n1 = (float)(n + 1);
  if (mode == 2) {
    span_pairs<false>(p.a, p.s, p.len, Mean{1.f / n1});
  } else {
    const float w = mode == 0 ? hyper[0] : 1.f / n1;
    span_pairs<false>(p.a, p.s, p.len, Lerp{w, 1.f - w});
  }
}

__global__ void avg_tick_kernel(long* __restrict__ count, const float* __restrict__ guard) {
  if (guard != nullptr && guard[0] != 0.f) return;
  count[0] += 1;  // the only writer: a plain store
}

__global__ __launch_bounds__(CHUNK_TPB) void avg_exchange_kernel(const long* __restrict__ table,
                                                                const long* __restrict__ chunks, int n_tensors,
                                                                int op) {
  Pair p;
  if (!pair_resolve(table, chunks, n_tensors, &p)) return;
  if (op == 0)
    span_pairs<true>(p.a, p.s, p.len, Swap());
  else if (op == 1)
    span_copy(p.s, p.a, p.len);
  else
    span_copy(p.a, p.s, p.len);
}

// SF_OK, SF_EINVAL or SF_EALIGN for the host copy of both tables
int avg_tables_check(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                     const long* chunks, int n_chunks) {
  if (!tables_args_ok(table_host, table, n_tensors, chunks_host, chunks, n_chunks)) return SF_EINVAL;
  bool misaligned = false;
  for (int t = 0; t < n_tensors; ++t) {
    const long* r = table_host + (long)t * AVG_TAB_ROW;
    if (r[0] == 0 || r[1] == 0 || r[2] <= 0 || r[3] < KIND_AVG || r[3] > KIND_WORDS) return SF_EINVAL;
    misaligned |= ((r[0] | r[1]) & (r[3] == KIND_WORDS ? 7 : 3)) != 0;
  }
  if (!chunks_tile(table_host, AVG_TAB_ROW, 2, n_tensors, chunks_host, n_chunks)) return SF_EINVAL;
  return misaligned ? SF_EALIGN : SF_OK;
}
}  // namespace

extern "C" int sf_avg_update(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                             const long* chunks, int n_chunks, int mode, const float* hyper_host, const float* hyper,
                             long* count, const float* guard, void* stream) {
  if (mode < 0 || mode > 2 || !count) return SF_EINVAL;
  if (mode == 0) {
    if (!hyper_host || !hyper) return SF_EINVAL;
    if (!(hyper_host[0] >= 0.f && hyper_host[0] <= 1.f)) return SF_EINVAL;  // (a NaN fails both)
  }
  const int rc = avg_tables_check(table_host, table, n_tensors, chunks_host, chunks, n_chunks);
  if (rc != SF_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(count) & 7) != 0 || (reinterpret_cast<uintptr_t>(hyper) & 3) != 0) return SF_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(avg_update_kernel, dim3(n_chunks), dim3(CHUNK_TPB), 0, s, table, chunks, n_tensors, mode, hyper,
                     count, guard);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(avg_tick_kernel, dim3(1), dim3(1), 0, s, count, guard);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_avg_exchange(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                               const long* chunks, int n_chunks, int op, void* stream) {
  if (op < 0 || op > 2) return SF_EINVAL;
  const int rc = avg_tables_check(table_host, table, n_tensors, chunks_host, chunks, n_chunks);
  if (rc != SF_OK) return rc;
  hipLaunchKernelGGL(avg_exchange_kernel, dim3(n_chunks), dim3(CHUNK_TPB), 0, (hipStream_t)stream, table, chunks,
                     n_tensors, op);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
