// mix_row.h — the mix row (include/sfhip.h, SF_MIX_ROW) that sf_clip_batch_mix (input_prologue.hip) and sf_ce_mix
// (step_tail.hip) both read: partner row, mode, lam as float32 bits, the CutMix box.  One set of checks serves the host
// entries (their copy of the rows) and the kernels (the device copy).
#pragma once
#include "common.h"

constexpr int MIX_ROW = SF_MIX_ROW;
constexpr int MIX_NONE = 0, MIX_MIXUP = 1, MIX_CUTMIX = 2;

__host__ __device__ __forceinline__ float mix_lambda(long bits) {
  const unsigned u = (unsigned)bits;
  float f;
  __builtin_memcpy(&f, &u, sizeof(f));
  return f;
}

// what the loss reads: the partner inside [0, n) and lam inside [0, 1] (a NaN fails; the high 32 bits are zero)
__host__ __device__ __forceinline__ bool mix_pair_ok(const long* r, long n) {
  if (r[0] < 0 || r[0] >= n || r[2] < 0 || r[2] > 0xffffffffL) return false;
  const float l = mix_lambda(r[2]);
  return l >= 0.f && l <= 1.f;
}

__host__ __device__ __forceinline__ bool mix_row_ok(const long* r, long n) {
  return mix_pair_ok(r, n) && r[1] >= MIX_NONE && r[1] <= MIX_CUTMIX;
}

// the box in output crop coordinates: 0 <= y0 <= y1 <= crop, 0 <= x0 <= x1 <= crop
__host__ __device__ __forceinline__ bool mix_box_ok(const long* r, long crop) {
  return r[3] >= 0 && r[3] <= r[5] && r[5] <= crop && r[4] >= 0 && r[4] <= r[6] && r[6] <= crop;
}
