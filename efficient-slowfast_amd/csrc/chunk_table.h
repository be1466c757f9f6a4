// chunk_table.h — what the kernels addressed through an int64 tensor table and a chunk list share (step_tail.hip: the
// optimizers; grad_clip.hip; lars.hip; weight_avg.hip; tensor_stats.hip).  A table row describes one tensor (addresses,
// numel, ...; the row width and the numel column differ per table), a chunk is (tensor index, first element) and covers at most CHUNK_ELEMS elements of one
// tensor, one workgroup of CHUNK_TPB threads per chunk.  Here, once each: the sizes, the address cast, the rule that turns
// a workgroup's chunk into a span or into "do nothing", the host check that the chunks tile the tensors, the fixed-order
// read-only walk over a span, the fixed-order block fold, and the state block sf_grad_norm / sf_lars_ratios leave.
#pragma once
#include "common.h"

constexpr int CHUNK_ELEMS = 4096;  // sf_sgd_chunk_elems(): four 16-byte accesses per thread and array
constexpr int CHUNK_TPB = 256;
constexpr int CHUNK_WAVES = CHUNK_TPB / 64;
// the state block, in floats: [0..1] the norm as ONE fp64, then norm (fp32), coefficient, non-finite flag, guard_out
constexpr int ST_NORM32 = 2, ST_COEF = 3, ST_FLAG = 4, ST_GUARD = 5;

__device__ __forceinline__ float* as_global(long addr) {
  // the address names global memory (a hipMalloc'ed span): say so, or every access becomes a flat one
  return (float*)(__attribute__((address_space(1))) float*)(unsigned long)addr;
}

// The chunk of this workgroup: its tensor, that tensor's table row, its first element and its length.  false
// (block-uniform): the chunk fails the checks the host entry made on its copy of both tables — a device row that
// differs does nothing, never a wild access.  What a kernel asks of its own columns (null addresses, alignment, the
// group) it checks behind this.
struct Chunk {
  const long* row;
  long ti, start;
  int len;
};
__device__ __forceinline__ bool chunk_resolve(const long* __restrict__ table, const long* __restrict__ chunks,
                                              int n_tensors, int row_width, int numel_col, Chunk* k) {
  const long* c = chunks + (long)blockIdx.x * 2;
  const long ti = c[0], start = c[1];
  if (ti < 0 || ti >= n_tensors) return false;
  const long* row = table + ti * row_width;
  const long numel = row[numel_col];
  if (start < 0 || start >= numel) return false;
  k->row = row;
  k->ti = ti;
  k->start = start;
  k->len = (int)(numel - start < CHUNK_ELEMS ? numel - start : CHUNK_ELEMS);
  return true;
}

// the chunks tile the tensors exactly, in table order: (0, 0), (0, C), ..., (1, 0), ... (numel: column `col` of a row)
static inline bool chunks_tile(const long* tab, int row, int col, int n_tensors, const long* chunks, int n_chunks) {
  long t = 0, s = 0;
  for (int i = 0; i < n_chunks; ++i) {
    if (t >= n_tensors || chunks[2 * i] != t || chunks[2 * i + 1] != s) return false;
    s += CHUNK_ELEMS;
    if (s >= tab[t * row + col]) {
      ++t;
      s = 0;
    }
  }
  return t == n_tensors && s == 0;
}

// the six table and count arguments every table entry checks first
static inline bool tables_args_ok(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                                  const long* chunks, int n_chunks) {
  return table_host && table && chunks_host && chunks && n_tensors > 0 && n_chunks > 0;
}

// The read-only walk over a span: acc = f(acc, x[i]) with thread t owning the groups of four elements t, t + 256, ... of
// the span, element by element in order, then the element behind the last whole group (up to three are left).  The
// 16-byte path and the 4-byte path read the same elements in the same order in the same thread: the result does not
// depend on the span's alignment.
template <typename T, typename F>
__device__ __forceinline__ T span_reduce(const float* __restrict__ x, int len, T acc, F f) {
  const int n4 = len >> 2;
  if (((unsigned long)x & 15) == 0) {
    for (int i = threadIdx.x; i < n4; i += CHUNK_TPB) {
      const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = f(acc, v[e]);
    }
  } else {
    for (int i = threadIdx.x; i < n4; i += CHUNK_TPB) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = f(acc, x[4 * i + e]);
    }
  }
  const int i = (n4 << 2) + threadIdx.x;
  if (i < len) acc = f(acc, x[i]);
  return acc;
}

struct SumSq {  // span_reduce: the sum of squares in fp64
  __device__ __forceinline__ double operator()(double acc, float v) const { return acc + (double)v * (double)v; }
};
struct Sum {  // block_fold
  __device__ __forceinline__ double operator()(double a, double b) const { return a + b; }
};

// N thread-sequential values -> xor butterfly -> wavefronts in order through LDS, one array and one barrier for all N;
// thread 0 holds the results.  No kernel calls ONE instantiation twice: a second call reuses s_part and would need a
// barrier between the first call's reads and its own writes (tensor_stats.hip's second launch calls two: <2, Sum> and
// <2, Max>, each with an array of its own).
template <int N, typename F>
__device__ __forceinline__ void block_fold(double (&v)[N], F comb) {
  __shared__ double s_part[CHUNK_WAVES][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int n = 0; n < N; ++n) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[n] = comb(v[n], __shfl_xor(v[n], o, 64));
  }
  if (lane == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) s_part[wave][n] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) {
    double r = s_part[0][n];
#pragma unroll
    for (int w = 1; w < CHUNK_WAVES; ++w) r = comb(r, s_part[w][n]);
    v[n] = r;
  }
}
