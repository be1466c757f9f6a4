// ensemble.hip — the test-time ensemble of utils/meters.py TestMeter.update_stats (reference :283-317) on the device.
//
// The host meter adds (or maxes) the clip predictions of a batch into per-video rows one clip at a time.  Here thread
// (b, k) looks at clip b's video: if b is the FIRST clip of that video in the batch the thread owns element
// (video, k) for this call — it loads the row's value, walks the rest of the batch in index order and folds in every
// clip of the same video, then stores once.  One owner per (video, class) element and the host loop's order: the sum
// is the host meter's bit for bit, and nothing needs an atomic.  The class-0 owner also writes the video's label (the
// last clip's, as the host's indexed assignment leaves it) and adds its clips to clip_count.  Rows of videos that have
// no clip in the batch are not touched: the launch is B x K threads whatever the number of videos.
// sf_ensemble_update_ml is the multi-label meter (labels are rows, :290-297) on the same owner rule and fold.
#include "common.h"

namespace {
constexpr int TPB = 256;

// What both kernels share.  Thread (b, k): counts the clips with a video outside [0, Nv) (thread 0 alone), finds out
// whether clip b is its video's first in the batch and, if so, folds the batch's clips of that video into element
// (video, k) in index order.  Returns the video (-1: this thread owns nothing); *n = its clips in the batch.
__device__ __forceinline__ int fold_owned(const float* __restrict__ preds, const int* __restrict__ video_idx,
                                          float* __restrict__ video_preds, int* __restrict__ bad_count, long i, int b,
                                          int k, int B, int K, int Nv, int mode, int* n) {
  if (i == 0) {  // the one owner of the error count: clips whose video is outside [0, Nv)
    int bad = 0;
    for (int j = 0; j < B; ++j) bad += (video_idx[j] < 0 || video_idx[j] >= Nv) ? 1 : 0;
    if (bad) *bad_count += bad;
  }
  const int v = video_idx[b];
  if (v < 0 || v >= Nv) return -1;
  for (int j = 0; j < b; ++j)
    if (video_idx[j] == v) return -1;  // an earlier clip of this video owns the row
  float acc = video_preds[(long)v * K + k];
  int cnt = 0;
  for (int j = b; j < B; ++j) {
    if (video_idx[j] != v) continue;
    const float p = preds[(long)j * K + k];
    acc = mode == 0 ? acc + p : ((p > acc || p != p) ? p : acc);  // amax: a NaN prediction propagates, as in torch
    ++cnt;
  }
  video_preds[(long)v * K + k] = acc;
  *n = cnt;
  return v;
}

__global__ void ensemble_update_kernel(const float* __restrict__ preds, const int* __restrict__ video_idx,
                                       const int* __restrict__ labels, float* __restrict__ video_preds,
                                       int* __restrict__ video_labels, int* __restrict__ clip_count,
                                       int* __restrict__ bad_count, int B, int K, int Nv, int mode) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x;
  if (i >= (long)B * K) return;
  const int b = (int)(i / K), k = (int)(i - (long)b * K);
  int n = 0;
  const int v = fold_owned(preds, video_idx, video_preds, bad_count, i, b, k, B, K, Nv, mode, &n);
  if (v < 0 || k != 0) return;
  clip_count[v] += n;
  if (labels) {
    int last = b;
    for (int j = b + 1; j < B; ++j)
      if (video_idx[j] == v) last = j;
    video_labels[v] = labels[last];
  }
}

// The multi-label meter (utils/meters.py:290-297): labels are fp32 rows [B][K] and video_labels [Nv][K].  The class-0
// owner of a video walks its clips in order as the host loop does: when the row the video holds (the stored one, then
// the previous clip's) has a positive sum and differs from the clip's, that is the reference's failed `assert
// torch.equal` — counted in bad_count[1]; the last clip's row is stored.  One thread per video does this (B x K
// loads at most): nobody else reads or writes the label rows.
__global__ void ensemble_update_ml_kernel(const float* __restrict__ preds, const int* __restrict__ video_idx,
                                          const float* __restrict__ labels, int ldl, float* __restrict__ video_preds,
                                          float* __restrict__ video_labels, int* __restrict__ clip_count,
                                          int* __restrict__ bad_count, int B, int K, int Nv, int mode) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x;
  if (i >= (long)B * K) return;
  const int b = (int)(i / K), k = (int)(i - (long)b * K);
  int n = 0;
  const int v = fold_owned(preds, video_idx, video_preds, bad_count, i, b, k, B, K, Nv, mode, &n);
  if (v < 0 || k != 0) return;
  clip_count[v] += n;
  float* stored = video_labels + (long)v * K;
  const float* have = stored;
  int mismatches = 0;
  for (int j = b; j < B; ++j) {
    if (video_idx[j] != v) continue;
    const float* row = labels + (long)j * ldl;
    float sum = 0.f;
    int differs = 0;
    for (int c = 0; c < K; ++c) {
      sum += have[c];
      differs |= !(have[c] == row[c]);
    }
    mismatches += (sum > 0.f && differs) ? 1 : 0;
    have = row;
  }
  if (have != stored)
    for (int c = 0; c < K; ++c) stored[c] = have[c];
  if (mismatches) atomicAdd(&bad_count[1], mismatches);  // one owner per VIDEO: several may count in one launch
}
}  // namespace

extern "C" int sf_ensemble_update(const float* preds, const int* video_idx, const int* labels, float* video_preds,
                                  int* video_labels, int* clip_count, int* bad_count, int B, int K, int Nv, int mode,
                                  void* stream) {
  if (!preds || !video_idx || !video_preds || !video_labels || !clip_count || !bad_count || B <= 0 || K <= 0 ||
      Nv <= 0 || (mode != 0 && mode != 1))
    return SF_EINVAL;
  hipLaunchKernelGGL(ensemble_update_kernel, dim3(sf_cdiv((long)B * K, TPB)), dim3(TPB), 0, (hipStream_t)stream, preds,
                     video_idx, labels, video_preds, video_labels, clip_count, bad_count, B, K, Nv, mode);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_ensemble_update_ml(const float* preds, const int* video_idx, const float* labels, int ldl,
                                     float* video_preds, float* video_labels, int* clip_count, int* bad_count, int B,
                                     int K, int Nv, int mode, void* stream) {
  if (!preds || !video_idx || !labels || !video_preds || !video_labels || !clip_count || !bad_count || B <= 0 ||
      K <= 0 || Nv <= 0 || ldl < K || (mode != 0 && mode != 1))
    return SF_EINVAL;
  hipLaunchKernelGGL(ensemble_update_ml_kernel, dim3(sf_cdiv((long)B * K, TPB)), dim3(TPB), 0, (hipStream_t)stream,
                     preds, video_idx, labels, ldl, video_preds, video_labels, clip_count, bad_count, B, K, Nv, mode);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
