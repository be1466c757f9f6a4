// ava_eval.hip — AVA frame-mAP at IoU 0.5 (reference utils/ava_eval_helper.py + utils/ava_evaluation/, the port of the TF
// object-detection API's PascalDetectionEvaluator) from device tensors: which detection is a true positive
// (sf_ava_match) and the VOC average precision of every class (sf_ava_ap).  The idiom is sf_map's (eval_metrics.hip):
// no sort, integer counts, no float atomics, fp64 sums folded in a fixed order — the same inputs give the same bits.
// Nothing here reads anything back: the meter copies four doubles (and the per-class AP) once per epoch.
#include "common.h"
#include "stats_row.h"

#include <math.h>

// np_box_ops.py:31-89 is plain fp64 numpy: every product, sum and quotient is rounded on its own.  A fused
// multiply-add would round (area1 + area2 - inter) or the area products once instead of twice and moves the IoU of some
// boxes across the 0.5 threshold.
#pragma clang fp contract(off)

namespace {
constexpr int AVA_TPB = 256;
constexpr int AVA_WAVES = AVA_TPB / 64;
constexpr int ROW_DROPPED = 0, ROW_VALID = 1, ROW_BADKEY = 2;  // the `valid` byte of a row

struct AvaGt {
  const double* box;  // [G][4] x1, y1, x2, y2 as the CSV holds them
  const int* cls;     // [G] column of preds (class id - 1)
  const int* off;     // [I + 1] rows of image m: off[m] .. off[m + 1], grouped by class, CSV order within a class
  const int* lut;     // [V][S] (video index, second) -> image id; -1: not in the ground truth; -2: excluded
  const unsigned char* wl;  // [C] 1: the class is evaluated
  int G, I, V, S, C;
};

// ava_eval_helper.py:266-275 for row i: the image (np.round: half to even, as rint) and the box.  Returns the `valid`
// byte; *img is the image id (-1: none) of a valid row.  _remove_invalid_boxes (per_image_evaluation.py:439-442) keeps
// a box iff y1 < y2 and x1 < x2: a NaN coordinate compares false and the row is dropped, as there.
__device__ __forceinline__ int ava_row(const float* __restrict__ boxes, int ldb, const float* __restrict__ meta, int ldm,
                                       int i, const AvaGt& gt, int* img, double* b) {
  const float fv = rintf(meta[(long)i * ldm]), fs = rintf(meta[(long)i * ldm + 1]);
  // video_idx_to_name[video_idx] raises for an index outside the list: counted, the caller refuses the result
  if (!(fv >= 0.f && fv < (float)gt.V) || !isfinite(fs)) return ROW_BADKEY;
  int m = -1;  // a second the table does not reach: an image without ground truth
  if (fs >= 0.f && fs < (float)gt.S) m = gt.lut[(long)(int)fv * gt.S + (int)fs];
  if (m == -2) return ROW_DROPPED;  // run_evaluation:216-225
  const float* r = boxes + (long)i * ldb;
  const float x1 = r[1], y1 = r[2], x2 = r[3], y2 = r[4];  // r[0] is the batch index
  if (!(x1 < x2 && y1 < y2)) return ROW_DROPPED;
  b[0] = (double)x1;  // float32 -> fp64 is exact: boxes[i].tolist()
  b[1] = (double)y1;
  b[2] = (double)x2;
  b[3] = (double)y2;
  *img = (m >= 0 && m < gt.I) ? m : -1;
  return ROW_VALID;
}

// np_box_ops.iou of one detection against one ground-truth box, in its operation order.
__device__ __forceinline__ double ava_iou(const double* b, double area1, const double* __restrict__ g) {
  const double gx1 = g[0], gy1 = g[1], gx2 = g[2], gy2 = g[3];
  const double ih = fmax(0.0, fmin(b[3], gy2) - fmax(b[1], gy1));
  const double iw = fmax(0.0, fmin(b[2], gx2) - fmax(b[0], gx1));
  const double inter = ih * iw;
  const double area2 = (gy2 - gy1) * (gx2 - gx1);
  const double uni = area1 + area2 - inter;
  return inter / uni;
}

// per_image_evaluation.py:331-339 for one detection box: for every class group of image m, g* = np.argmax of the IoU
// row (the first maximum; a NaN, which 0 / 0 gives for a degenerate pair, is numpy's maximum) and hit(class, g*) when
// IoU(g*) >= 0.5.  Groups of a class outside [0, C) or outside the whitelist have no detection and are skipped.
template <typename F>
__device__ __forceinline__ void ava_scan(const double* b, int m, const AvaGt& gt, F&& hit) {
  int g = gt.off[m], hi = gt.off[m + 1];
  if (g < 0 || hi > gt.G) return;  // a table that does not describe itself: nothing is read
  const double area1 = (b[3] - b[1]) * (b[2] - b[0]);
  while (g < hi) {
    const int c = gt.cls[g];
    int best_g = g;
    double best = ava_iou(b, area1, gt.box + (long)g * 4);
    int e = g + 1;
    for (; e < hi && gt.cls[e] == c; ++e) {
      const double v = ava_iou(b, area1, gt.box + (long)e * 4);
      if (!isnan(best) && (v > best || isnan(v))) {
        best = v;
        best_g = e;
      }
    }
    if (best >= 0.5 && c >= 0 && c < gt.C && gt.wl[c]) hit(c, best_g);
    g = e;
  }
}

// ---------------------------------------------------------------------------------------------- matching
// The reference walks an image's detections of a class in order and gives ground-truth box g to the FIRST one whose
// argmax it is (is_gt_box_detected, per_image_evaluation.py:336-343).  The order inside (image, class) is the row order
// (get_ava_eval_data appends row by row), so "first" is the smallest row index: launch 1 takes an integer minimum per
// ground-truth box, launch 2 asks every detection whether it is that minimum.  No assumption on how rows are ordered
// or grouped, and integer minima do not depend on the order of execution.
__global__ __launch_bounds__(AVA_TPB) void ava_claim_kernel(const float* __restrict__ boxes, int ldb,
                                                            const float* __restrict__ meta, int ldm, int K, AvaGt gt,
                                                            int* __restrict__ first) {
  const int i = blockIdx.x * AVA_TPB + threadIdx.x;
  if (i >= K) return;
  int m = -1;
  double b[4];
  if (ava_row(boxes, ldb, meta, ldm, i, gt, &m, b) != ROW_VALID || m < 0) return;
  ava_scan(b, m, gt, [&](int, int g) { atomicMin(&first[g], i); });
}

// Workgroup b owns rows 256 b .. 256 b + 255: it clears their tp bytes (one contiguous span), then a thread per row
// repeats launch 1's scan — the same code, so the same g* — and sets the byte of every class whose box it holds.
__global__ __launch_bounds__(AVA_TPB) void ava_label_kernel(const float* __restrict__ boxes, int ldb,
                                                            const float* __restrict__ meta, int ldm, int K, AvaGt gt,
                                                            const int* __restrict__ first,
                                                            unsigned char* __restrict__ tp,
                                                            unsigned char* __restrict__ valid) {
  const int r0 = blockIdx.x * AVA_TPB;
  const int rows = K - r0 < AVA_TPB ? K - r0 : AVA_TPB;
  const long base = (long)r0 * gt.C, span = (long)rows * gt.C;
  for (long e = threadIdx.x; e < span; e += AVA_TPB) tp[base + e] = 0;
  __syncthreads();
  const int i = r0 + threadIdx.x;
  if (i >= K) return;
  int m = -1;
  double b[4];
  const int code = ava_row(boxes, ldb, meta, ldm, i, gt, &m, b);
  valid[i] = (unsigned char)code;
  if (code != ROW_VALID || m < 0) return;
  unsigned char* row = tp + (long)i * gt.C;
  ava_scan(b, m, gt, [&](int c, int g) {
    if (first[g] == i) row[c] = 1;
  });
}

// ---------------------------------------------------------------------------------------------- average precision
// metrics.py:60-125 for one class with n ground-truth boxes: the detections in descending score order, precision at
// position r = cumTP(r) / r, precision replaced by its running maximum from the right, and
//     AP = sum over the positions where recall steps (the true positives) of (recall step) x envelope
//        = (1/n) sum_{true positives p} max_{q >= p} cumTP(q) / q.
// The maximum is attained at a true positive (cumTP / q falls along a run of false positives), so with
//     rank(i)    = #{valid j : s_j > s_i, or s_j == s_i and j >= i}   (the position, 1-based; np.argsort leaves the
//     tp_rank(i) = the same count over the true positives              order of equal scores open — here the higher
//                                                                      row index stands first)
// the envelope at true positive i is max{tp_rank(j) / rank(j) : j a true positive, rank(j) >= rank(i)}.  Workgroup
// (c, b) owns class c and candidates 256 b .. 256 b + 255 and streams the class's column through LDS in tiles of 256,
// as map_partial_kernel does; all lanes read one LDS address at a time (a broadcast).
__global__ __launch_bounds__(AVA_TPB) void ava_rank_kernel(const float* __restrict__ preds, int ld,
                                                           const unsigned char* __restrict__ tp,
                                                           const unsigned char* __restrict__ valid, int K, int C,
                                                           const unsigned char* __restrict__ wl,
                                                           int* __restrict__ rank_out, int* __restrict__ tprank_out,
                                                           int* __restrict__ refused_part) {
  __shared__ __attribute__((aligned(16))) float s_s[AVA_TPB];
  __shared__ __attribute__((aligned(16))) int s_t[AVA_TPB];
  __shared__ int s_ref[AVA_WAVES];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.y * AVA_TPB + tid;
  const bool det = i < K && wl[c] != 0 && valid[i] == ROW_VALID;  // (row i, class c) is a detection
  const float si = det ? preds[(long)i * ld + c] : NAN;
  const bool mine = det && tp[(long)i * C + c] != 0;
  const int ref = wave_sum((det && !isfinite(si)) ? 1 : 0);  // counted by its one owner; the caller refuses the result
  if (lane == 0) s_ref[wave] = ref;
  int rank = 0, tprank = 0;
  // candidates without a true positive have nothing to count (their ranks are never read): the column is not streamed
  const int n_sweep = __syncthreads_or(mine ? 1 : 0) ? K : 0;
  for (int j0 = 0; j0 < n_sweep; j0 += AVA_TPB) {
    const int j = j0 + tid;
    const bool dj = j < K && valid[j] == ROW_VALID;  // wl[c] != 0: the class has a true positive
    // not a detection: a NaN compares false with everything, so the tile is always walked whole
    s_s[tid] = dj ? preds[(long)j * ld + c] : NAN;
    s_t[tid] = (dj && tp[(long)j * C + c] != 0) ? 1 : 0;
    __syncthreads();
    if (mine) {
#pragma unroll 4
      for (int t = 0; t < AVA_TPB; t += 4) {
        const f32x4 sv = *reinterpret_cast<const f32x4*>(&s_s[t]);
        const int4 tv = *reinterpret_cast<const int4*>(&s_t[t]);
        const int te[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ahead = (sv[e] > si || (sv[e] == si && j0 + t + e >= i)) ? 1 : 0;  // itself included
          rank += ahead;
          tprank += ahead & te[e];
        }
      }
    }
    __syncthreads();
  }
  if (i < K) {  // class-major, so that the envelope pass streams a contiguous column
    rank_out[(long)c * K + i] = mine ? rank : 0;
    tprank_out[(long)c * K + i] = mine ? tprank : 0;
  }
  if (tid == 0) {  // s_ref: written before the vote's barrier
    int r = 0;
    for (int w = 0; w < AVA_WAVES; ++w) r += s_ref[w];
    refused_part[(long)c * gridDim.y + blockIdx.y] = r;
  }
}

// For every true positive, the largest tp_rank / rank among the true positives at or after it.  Fractions compare by an
// exact int64 cross-multiplication (both factors < 2^24); equal fractions divide to the same double, so which of them
// is kept does not matter.  One fp64 division per true positive; xor butterfly, then wavefronts in order.
__global__ __launch_bounds__(AVA_TPB) void ava_envelope_kernel(const int* __restrict__ rank_in,
                                                               const int* __restrict__ tprank_in, int K,
                                                               double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) int s_r[AVA_TPB];
  __shared__ __attribute__((aligned(16))) int s_t[AVA_TPB];
  __shared__ double s_sum[AVA_WAVES];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.y * AVA_TPB + tid;
  const int* rk = rank_in + (long)c * K;
  const int* tr = tprank_in + (long)c * K;
  const int ri = i < K ? rk[i] : 0;
  const bool mine = ri > 0;
  long bt = i < K ? tr[i] : 0, br = ri;  // itself: "at or after"
  const int n_sweep = __syncthreads_or(mine ? 1 : 0) ? K : 0;
  for (int j0 = 0; j0 < n_sweep; j0 += AVA_TPB) {
    const int j = j0 + tid;
    s_r[tid] = j < K ? rk[j] : 0;  // 0: not a true positive, never >= ri
    s_t[tid] = j < K ? tr[j] : 0;
    __syncthreads();
    if (mine) {
#pragma unroll 4
      for (int t = 0; t < AVA_TPB; t += 4) {
        const int4 rv = *reinterpret_cast<const int4*>(&s_r[t]);
        const int4 tv = *reinterpret_cast<const int4*>(&s_t[t]);
        const int re[4] = {rv.x, rv.y, rv.z, rv.w}, te[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (re[e] >= ri && (long)te[e] * br > bt * (long)re[e]) {
            bt = te[e];
            br = re[e];
          }
        }
      }
    }
    __syncthreads();
  }
  double term = mine ? (double)bt / (double)br : 0.0;
  term = wave_sum(term);
  if (lane == 0) s_sum[wave] = term;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int w = 0; w < AVA_WAVES; ++w) tot += s_sum[w];
    part[(long)c * gridDim.y + blockIdx.y] = tot;
  }
}

// ONE workgroup: thread c adds class c's partials in block order and divides by num_gt[c]; thread 0 adds the classes in
// index order (object_detection_evaluation.py:777-815: a class without ground truth is left out of np.nanmean; the mean
// over no class is NaN there and here).  out = {mAP, classes counted, refused scores, rows whose video index is outside
// the table}; ap[c] = -1 for a class left out.
__global__ __launch_bounds__(AVA_TPB) void ava_finish_kernel(const double* __restrict__ part,
                                                             const int* __restrict__ refused_part,
                                                             const unsigned char* __restrict__ valid, int K, int C,
                                                             int nblk, const int* __restrict__ num_gt,
                                                             double* __restrict__ out, double* __restrict__ ap) {
  __shared__ double s_ap[AVA_TPB];
  __shared__ long s_ref[AVA_TPB];
  double sum = 0.0;  // thread 0's
  long refused = 0;
  int classes = 0;
  for (int c0 = 0; c0 < C; c0 += AVA_TPB) {
    const int c = c0 + threadIdx.x;
    double a = -1.0;
    long r = 0;
    if (c < C) {
      double tot = 0.0;
      for (int b = 0; b < nblk; ++b) {
        tot += part[(long)c * nblk + b];
        r += refused_part[(long)c * nblk + b];
      }
      if (num_gt[c] > 0) a = tot / (double)num_gt[c];
      if (ap != nullptr) ap[c] = a;
    }
    s_ap[threadIdx.x] = a;
    s_ref[threadIdx.x] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = C - c0 < AVA_TPB ? C - c0 : AVA_TPB;
      for (int t = 0; t < n; ++t) {
        if (s_ap[t] >= 0.0) {
          sum += s_ap[t];
          classes += 1;
        }
        refused += s_ref[t];
      }
    }
    __syncthreads();
  }
  long bad = 0;
  for (int i = threadIdx.x; i < K; i += AVA_TPB) bad += valid[i] == ROW_BADKEY ? 1 : 0;
  s_ref[threadIdx.x] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    bad = 0;
    for (int t = 0; t < AVA_TPB; ++t) bad += s_ref[t];
    out[0] = classes > 0 ? sum / (double)classes : (double)NAN;
    out[1] = (double)classes;
    out[2] = (double)refused;
    out[3] = (double)bad;
  }
}

// The one workspace: {partial sums fp64 [C][nblk]} {rank, tp_rank int32 [C][K] each} {first int32 [G]} {refused int32
// [C][nblk]}; every part starts on 8 bytes.
struct AvaWs {
  long part, rank, tprank, first, refused, bytes;
  int nblk;
};
long up8(long n) { return (n + 7) / 8 * 8; }
bool ava_ws(int K, int C, int G, AvaWs* w) {
  if (K <= 0 || C <= 0 || G < 0) return false;
  const long kc = (long)K * C;
  const long nblk = ((long)K + AVA_TPB - 1) / AVA_TPB;
  if (kc >= (1L << 31) || nblk > 65535) return false;
  w->nblk = (int)nblk;
  w->part = 0;
  w->rank = (long)C * nblk * 8;
  w->tprank = w->rank + up8(kc * 4);
  w->first = w->tprank + up8(kc * 4);
  w->refused = w->first + up8((long)G * 4);
  w->bytes = w->refused + up8((long)C * nblk * 4);
  return true;
}
bool off4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }
bool off8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; }
}  // namespace

extern "C" long sf_ava_ws_bytes(int K, int C, int G) {
  AvaWs w;
  return ava_ws(K, C, G, &w) ? w.bytes : 0;
}

extern "C" int sf_ava_match(const float* boxes, int ldb, const float* metadata, int ldm, int K, int C,
                            const double* gt_box, const int* gt_cls, const int* gt_off, int G, int I, const int* lut,
                            int V, int S, const unsigned char* whitelist, void* ws, unsigned char* tp,
                            unsigned char* valid, void* stream) {
  AvaWs w;
  if (!boxes || !metadata || !gt_off || !lut || !whitelist || !ws || !tp || !valid) return SF_EINVAL;
  if (G > 0 && (!gt_box || !gt_cls)) return SF_EINVAL;
  if (ldb < 5 || ldm < 2 || I < 0 || V <= 0 || S <= 0 || (long)V * S >= (1L << 31) || !ava_ws(K, C, G, &w))
    return SF_EINVAL;
  if (off4(boxes) || off4(metadata) || off8(gt_box) || off4(gt_cls) || off4(gt_off) || off4(lut) || off8(ws))
    return SF_EALIGN;
  const AvaGt gt = {gt_box, gt_cls, gt_off, lut, whitelist, G, I, V, S, C};
  int* first = reinterpret_cast<int*>(static_cast<char*>(ws) + w.first);
  // every byte 0x7f: 2 139 062 143, above any row index (K C < 2^31)
  if (G > 0 && hipMemsetAsync(first, 0x7f, (size_t)G * 4, (hipStream_t)stream) != hipSuccess) return SF_ELAUNCH;
  hipLaunchKernelGGL(ava_claim_kernel, dim3(w.nblk), dim3(AVA_TPB), 0, (hipStream_t)stream, boxes, ldb, metadata, ldm,
                     K, gt, first);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ava_label_kernel, dim3(w.nblk), dim3(AVA_TPB), 0, (hipStream_t)stream, boxes, ldb, metadata, ldm,
                     K, gt, (const int*)first, tp, valid);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_ava_ap(const float* preds, int ld, const unsigned char* tp, const unsigned char* valid, int K, int C,
                         const unsigned char* whitelist, const int* num_gt, int G, void* ws, double* out, double* ap,
                         void* stream) {
  AvaWs w;
  if (!preds || !tp || !valid || !whitelist || !num_gt || !ws || !out) return SF_EINVAL;
  if (!ava_ws(K, C, G, &w) || ld < C) return SF_EINVAL;
  if (off4(preds) || off4(num_gt) || off8(ws) || off8(out) || off8(ap)) return SF_EALIGN;
  char* base = static_cast<char*>(ws);
  double* part = reinterpret_cast<double*>(base + w.part);
  int* rank = reinterpret_cast<int*>(base + w.rank);
  int* tprank = reinterpret_cast<int*>(base + w.tprank);
  int* refused = reinterpret_cast<int*>(base + w.refused);
  hipLaunchKernelGGL(ava_rank_kernel, dim3(C, w.nblk), dim3(AVA_TPB), 0, (hipStream_t)stream, preds, ld, tp, valid, K,
                     C, whitelist, rank, tprank, refused);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ava_envelope_kernel, dim3(C, w.nblk), dim3(AVA_TPB), 0, (hipStream_t)stream, (const int*)rank,
                     (const int*)tprank, K, part);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ava_finish_kernel, dim3(1), dim3(AVA_TPB), 0, (hipStream_t)stream, (const double*)part,
                     (const int*)refused, valid, K, C, w.nblk, num_gt, out, ap);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
