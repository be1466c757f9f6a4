// stats_row.h — what the kernels that write a StatsRing row share (step_tail.hip: sf_ce_topk, sf_bce; eval_metrics.hip:
// sf_topk_errors): the row layout, the wavefront reductions in their fixed order, the top-k rank rule and the error
// percentages of train_net.py:123-125 / :230-232.
#pragma once
#include "common.h"

constexpr int CE_WAVES = 16;
constexpr int CE_TPB = CE_WAVES * 64;
constexpr int RING_ROW = 8;
// row[6]: which kernel wrote the row (0: cross-entropy)
constexpr float KIND_BCE = 1.f;
constexpr float KIND_EVAL = 2.f;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Class j (value v) stands in front of the label l (value xl) in torch.topk's order: greater, or equal with a lower
// index.  A row is a top-k hit iff fewer than k classes do.
__device__ __forceinline__ int beats_label(float v, float xl, int j, long l) {
  return (v > xl || (v == xl && j < l)) ? 1 : 0;
}

// (1 - correct / N) * 100 in float32, as the reference computes it on a float tensor
__device__ __forceinline__ float topk_error_pct(int correct, float n) { return (1.0f - (float)correct / n) * 100.0f; }
