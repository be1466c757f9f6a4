// eval_metrics.hip — the loop between epochs (reference tools/train_net.py:166-251 eval_epoch, utils/meters.py:557-714
// ValMeter and get_map) without the host: the top-k errors of an evaluation batch as a StatsRing row (sf_topk_errors),
// ValMeter.update_predictions as an append to a device store (sf_rows_append), and mean average precision of the
// stored rows (sf_map).  Nothing here reads anything back: the meter copies once per LOG_PERIOD and once per epoch.
#include "common.h"
#include "stats_row.h"

#include <math.h>

namespace {
// ---------------------------------------------------------------------------------------------- top-k errors
// metrics.topks_correct for k = 1 and k = k_hi plus the two percentages (train_net.py:227-232) of one batch.  ONE
// workgroup, a wavefront per row as in ce_topk_kernel (step_tail.hip) — the sizes are the same N = 2..64 rows of
// K = 27..700 — but one sweep per row: the eval head returns probabilities, there is no loss and no gradient.
__global__ __launch_bounds__(CE_TPB) void topk_errors_kernel(const float* __restrict__ preds, int ld,
                                                             const long* __restrict__ labels, int N, int K, int k_hi,
                                                             float* __restrict__ ring, int* __restrict__ counter,
                                                             int cap) {
  __shared__ int s_cnt[CE_WAVES][4];  // top-1 hits, top-k_hi hits, rows with a non-finite value, bad labels
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int hit1 = 0, hitk = 0, nonfinite = 0, bad = 0;
  for (int r = wave; r < N; r += CE_WAVES) {
    const float* x = preds + (long)r * ld;
    const long l = labels[r];
    const bool ok = l >= 0 && l < K;  // a label outside [0, K): wrong for every k, counted, never a read
    const float xl = ok ? x[l] : 0.f;
    int rank = 0, nf = 0;
    for (int j = lane; j < K; j += 64) {
      const float v = x[j];
      nf |= !isfinite(v);
      rank += beats_label(v, xl, j, l);
    }
    rank = wave_sum(rank);
    nf = wave_sum(nf) != 0;
    if (ok) {
      if (!nf) {  // a row with a NaN or an Inf is wrong for every k
        hit1 += rank < 1;
        hitk += rank < k_hi;
      }
    } else {
      bad += 1;
    }
    nonfinite += nf;
  }
  if (lane == 0) {
    s_cnt[wave][0] = hit1;
    s_cnt[wave][1] = hitk;
    s_cnt[wave][2] = nonfinite;
    s_cnt[wave][3] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c[4] = {0, 0, 0, 0};
    for (int w = 0; w < CE_WAVES; ++w) {
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] += s_cnt[w][i];
    }
    const int step = counter[0];
    const int slot = ((step % cap) + cap) % cap;
    float* row = ring + (long)slot * RING_ROW;
    const float n = (float)N;
    row[0] = 0.f;
    row[1] = topk_error_pct(c[0], n);  // train_net.py:230-232, in float32 as there
    row[2] = topk_error_pct(c[1], n);
    row[3] = c[2] != 0 ? 1.f : 0.f;
    row[4] = n;
    row[5] = (float)c[3];
    row[6] = KIND_EVAL;
    row[7] = 0.f;
    counter[0] = step + 1;  // the only writer: a plain store
  }
}

// ---------------------------------------------------------------------------------------------- row store
// all_preds.append / all_labels.append (utils/meters.py:623-632) as a copy to row `cursor[0]` of two [cap][K] stores.
// ONE workgroup, because the cursor lives in device memory: every thread reads it, the barrier stands between the last
// read and the one store that advances it.  A batch is at most ~1e5 floats.  Rows that would pass `cap` are not written
// and are added to cursor[1].
__global__ __launch_bounds__(CE_TPB) void rows_append_kernel(const float* __restrict__ preds, int ldp,
                                                             const float* __restrict__ labels, int ldl, int N, int K,
                                                             float* __restrict__ store_preds,
                                                             float* __restrict__ store_labels, int* __restrict__ cursor,
                                                             int cap) {
  const int cur = cursor[0];
  __syncthreads();
  // a cursor outside [0, cap] (nobody but this kernel and the meter's reset writes it): nothing is stored
  const int room = (cur >= 0 && cur <= cap) ? cap - cur : 0;
  const int rows = N < room ? N : room;
  const long total = (long)rows * K;
  for (long e = threadIdx.x; e < total; e += CE_TPB) {
    const long r = e / K;
    const int j = (int)(e - r * K);
    const long dst = ((long)cur + r) * K + j;
    store_preds[dst] = preds[r * ldp + j];
    store_labels[dst] = labels[r * ldl + j];
  }
  if (threadIdx.x == 0) {
    if (rows > 0) cursor[0] = cur + rows;
    if (rows < N) cursor[1] += N - rows;
  }
}

// ---------------------------------------------------------------------------------------------- mAP
// get_map (utils/meters.py:690-714) = the mean over the classes with a positive of sklearn's average_precision_score,
// which for one class with scores s, labels y and P positives is
//     AP = (1/P) sum_{i : y_i = 1} TP(s_i) / CNT(s_i),   TP(t) = #{j : s_j >= t, y_j = 1},   CNT(t) = #{j : s_j >= t}
// (tied scores are one threshold there and every positive of a tie group contributes the group's precision: the same
// sum).  No sort: workgroup (c, b) owns class c and candidates i = 256 b .. 256 b + 255, streams the class's column
// through LDS in tiles of 256 (the matrix is a few MB: L2) and every thread with y_i = 1 counts over the tile — all lanes
// read the same LDS address (a broadcast), 16 bytes at a time.  The counts are integers; the only floating point is one
// fp64 division per positive and the sums, folded in a fixed order (xor butterfly, wavefronts in order, then blocks in
// order and classes in order in map_finish_kernel): equal bits run to run, no float atomics.  Scores compare as floats,
// so -0.0 ties +0.0.  An element with a NaN / Inf score or a label other than 0 or 1 is counted (by its one owner)
// and the caller refuses the result.
constexpr int MAP_TPB = 256;
constexpr int MAP_WAVES = MAP_TPB / 64;
constexpr int MAP_PART = 3;  // doubles per (class, block): sum of precisions, positives, refused elements

__global__ __launch_bounds__(MAP_TPB) void map_partial_kernel(const float* __restrict__ scores, int lds,
                                                              const float* __restrict__ labels, int ldl, int N,
                                                              double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float s_s[MAP_TPB];
  __shared__ __attribute__((aligned(16))) float s_y[MAP_TPB];
  __shared__ double s_sum[MAP_WAVES];
  __shared__ int s_cnt[MAP_WAVES][2];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.y * MAP_TPB + tid;
  float si = 0.f, yi = 0.f;
  if (i < N) {
    si = scores[(long)i * lds + c];
    yi = labels[(long)i * ldl + c];
  }
  const int refused = (i < N && (!isfinite(si) || (yi != 0.f && yi != 1.f))) ? 1 : 0;
  const bool mine = i < N && yi == 1.f;
  int cnt = 0, tp = 0;
  // a block of candidates without a positive has nothing to count: it leaves its (0, 0, refused) partial without
  // streaming the column.  The vote is the same in every thread, so the barriers of the loop stay matched.
  const int n_sweep = __syncthreads_or(mine ? 1 : 0) ? N : 0;
  for (int j0 = 0; j0 < n_sweep; j0 += MAP_TPB) {
    const int j = j0 + tid;
    // past the end: a NaN score compares false with everything, so the tile is always walked whole
    s_s[tid] = j < N ? scores[(long)j * lds + c] : NAN;
    s_y[tid] = j < N ? labels[(long)j * ldl + c] : 0.f;
    __syncthreads();
    if (mine) {
#pragma unroll 4
      for (int t = 0; t < MAP_TPB; t += 4) {
        const f32x4 sv = *reinterpret_cast<const f32x4*>(&s_s[t]);
        const f32x4 yv = *reinterpret_cast<const f32x4*>(&s_y[t]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ge = sv[e] >= si ? 1 : 0;
          cnt += ge;
          tp += (ge && yv[e] == 1.f) ? 1 : 0;
        }
      }
    }
    __syncthreads();
  }
  // a positive with a NaN score counts nothing, itself included: no division by zero (the result is refused anyway)
  double term = (mine && cnt > 0) ? (double)tp / (double)cnt : 0.0;
  term = wave_sum(term);
  const int pos = wave_sum(mine ? 1 : 0);
  const int ref = wave_sum(refused);
  if (lane == 0) {
    s_sum[wave] = term;
    s_cnt[wave][0] = pos;
    s_cnt[wave][1] = ref;
  }
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    int p = 0, r = 0;
    for (int w = 0; w < MAP_WAVES; ++w) {
      tot += s_sum[w];
      p += s_cnt[w][0];
      r += s_cnt[w][1];
    }
    double* o = part + ((long)c * gridDim.y + blockIdx.y) * MAP_PART;
    o[0] = tot;
    o[1] = (double)p;
    o[2] = (double)r;
  }
}

// ONE workgroup: thread c adds class c's partials in block order and divides by P; thread 0 then adds the classes in
// index order, 256 at a time through LDS.  out = {mAP (0 when no class has a positive, as get_map returns then), classes
// with a positive, refused elements}; ap[c] = -1 for a class left out.
__global__ __launch_bounds__(MAP_TPB) void map_finish_kernel(const double* __restrict__ part, int C, int nblk,
                                                             double* __restrict__ out, double* __restrict__ ap) {
  __shared__ double s_ap[MAP_TPB];
  __shared__ double s_ref[MAP_TPB];
  double sum = 0.0, refused = 0.0;  // thread 0's
  int classes = 0;
  for (int c0 = 0; c0 < C; c0 += MAP_TPB) {
    const int c = c0 + threadIdx.x;
    double a = -1.0, r = 0.0;
    if (c < C) {
      double tot = 0.0, p = 0.0;
      const double* row = part + (long)c * nblk * MAP_PART;
      for (int b = 0; b < nblk; ++b) {
        tot += row[b * MAP_PART];
        p += row[b * MAP_PART + 1];
        r += row[b * MAP_PART + 2];
      }
      if (p > 0.0) a = tot / p;
      if (ap != nullptr) ap[c] = a;
    }
    s_ap[threadIdx.x] = a;
    s_ref[threadIdx.x] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = C - c0 < MAP_TPB ? C - c0 : MAP_TPB;
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
  if (threadIdx.x == 0) {
    out[0] = classes > 0 ? sum / (double)classes : 0.0;
    out[1] = (double)classes;
    out[2] = refused;
  }
}

long map_blocks(int N) { return ((long)N + MAP_TPB - 1) / MAP_TPB; }
}  // namespace

extern "C" int sf_topk_errors(const float* preds, int ld, const long* labels, int N, int K, int k_hi, float* ring,
                              int* counter, int cap, void* stream) {
  if (!preds || !labels || !ring || !counter) return SF_EINVAL;
  if (N <= 0 || K <= 0 || ld < K || cap <= 0 || k_hi < 1 || k_hi > K) return SF_EINVAL;
  hipLaunchKernelGGL(topk_errors_kernel, dim3(1), dim3(CE_TPB), 0, (hipStream_t)stream, preds, ld, labels, N, K, k_hi,
                     ring, counter, cap);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_rows_append(const float* preds, int ldp, const float* labels, int ldl, int N, int K,
                              float* store_preds, float* store_labels, int* cursor, int cap, void* stream) {
  if (!preds || !labels || !store_preds || !store_labels || !cursor) return SF_EINVAL;
  if (N <= 0 || K <= 0 || ldp < K || ldl < K || cap <= 0) return SF_EINVAL;
  hipLaunchKernelGGL(rows_append_kernel, dim3(1), dim3(CE_TPB), 0, (hipStream_t)stream, preds, ldp, labels, ldl, N, K,
                     store_preds, store_labels, cursor, cap);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" long sf_map_ws_bytes(int N, int C) {
  if (N <= 0 || C <= 0 || map_blocks(N) > 65535) return 0;
  return map_blocks(N) * C * MAP_PART * (long)sizeof(double);
}

extern "C" int sf_map(const float* scores, int lds, const float* labels, int ldl, int N, int C, void* ws, double* out,
                      double* ap, void* stream) {
  if (!scores || !labels || !ws || !out) return SF_EINVAL;
  if (N <= 0 || C <= 0 || lds < C || ldl < C || sf_map_ws_bytes(N, C) == 0) return SF_EINVAL;
  if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ap)) & 7)
    return SF_EALIGN;
  const int nblk = (int)map_blocks(N);
  hipLaunchKernelGGL(map_partial_kernel, dim3(C, nblk), dim3(MAP_TPB), 0, (hipStream_t)stream, scores, lds, labels,
                     ldl, N, (double*)ws);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(map_finish_kernel, dim3(1), dim3(MAP_TPB), 0, (hipStream_t)stream, (const double*)ws, C, nblk, out,
                     ap);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
