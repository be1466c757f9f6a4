// ensemble.hip — the test-time ensemble of utils/meters.py TestMeter.update_stats (reference :283-317) on the device.
//
// The host meter adds (or maxes) the clip predictions of a batch into per-video rows one clip at a time.  Here thread
// (b, k) looks at clip b's video: if b is the FIRST clip of that video in the batch the thread owns element
// (video, k) for this call — it loads the row's value, walks the rest of the batch in index order and folds in every
// clip of the same video, then stores once.  One owner per (video, class) element and the host loop's order: the sum
// is the host meter's bit for bit, and nothing needs an atomic.  The class-0 owner also writes the video's label (the
// last clip's, as the host's indexed assignment leaves it) and adds its clips to clip_count.  Rows of videos that have
// no clip in the batch are not touched: the launch is B x K threads whatever the number of videos.
#include "common.h"

namespace {
constexpr int TPB = 256;

__global__ void ensemble_update_kernel(const float* __restrict__ preds, const int* __restrict__ video_idx,
                                       const int* __restrict__ labels, float* __restrict__ video_preds,
                                       int* __restrict__ video_labels, int* __restrict__ clip_count,
                                       int* __restrict__ bad_count, int B, int K, int Nv, int mode) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x;
  if (i >= (long)B * K) return;
  const int b = (int)(i / K), k = (int)(i - (long)b * K);
  if (i == 0) {  // the one owner of the error count: clips whose video is outside [0, Nv)
    int bad = 0;
    for (int j = 0; j < B; ++j) bad += (video_idx[j] < 0 || video_idx[j] >= Nv) ? 1 : 0;
    if (bad) *bad_count += bad;
  }
  const int v = video_idx[b];
  if (v < 0 || v >= Nv) return;
  for (int j = 0; j < b; ++j)
    if (video_idx[j] == v) return;  // an earlier clip of this video owns the row
  float acc = video_preds[(long)v * K + k];
  int n = 0, last = b;
  for (int j = b; j < B; ++j) {
    if (video_idx[j] != v) continue;
    const float p = preds[(long)j * K + k];
    acc = mode == 0 ? acc + p : ((p > acc || p != p) ? p : acc);  // amax: a NaN prediction propagates, as in torch
    last = j;
    ++n;
  }
  video_preds[(long)v * K + k] = acc;
  if (k == 0) {
    clip_count[v] += n;
    if (labels) video_labels[v] = labels[last];
  }
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
