// class_report.hip — evaluation class by class, without the host: the confusion matrix and the per-class top-1 / top-k
// hits of a batch of predictions added to caller-owned int64 counters (sf_confusion_update), and precision / recall /
// F1 / per-class accuracy with their macro means from those counters (sf_class_report).  The reference has no code for
// this (its result tables are typed by hand); the contract is include/sfhip.h's, restated in tests/_class_report_ref.py.
//
// The rule of a row is sf_topk_errors' (eval_metrics.hip, beats_label in stats_row.h): class j stands in front of class
// c iff x[j] > x[c], or x[j] == x[c] and j < c.  Values compare as floats, so -0.0 ties +0.0 and the lower index wins a
// tie.  The PREDICTED class is the one nothing stands in front of (the largest value, the lowest index among equals);
// the label is within the top k iff fewer than k classes stand in front of it — so "predicted == label" and "top-1 hit"
// are one statement.  A row with a label outside [0, K) is refused (counted in refused[0], its scores never read); a
// row with a valid label and a NaN or an infinity anywhere is refused (refused[1]) — sf_topk_errors counts both kinds
// as wrong for every k.  A refused row adds to nothing else.  Hence for every input
//     sum(conf) = N - refused[0] - refused[1],  trace(conf) = sum(hits[:, 0]) = sf_topk_errors' top-1 hits,
//     sum(hits[:, 1]) = its top-k_hi hits,  row sums of conf = support,  column sums = predicted counts.
// Only integer adds: the result does not depend on the order of execution.  No float atomics.
// sf_class_weights turns the same counters into fp32 class weights for the weighted losses of step_tail.hip (balanced or
// effective-number), in one launch and without a host read.
#include "common.h"
#include "stats_row.h"

#include <math.h>

namespace {
constexpr int CONF_TPB = 256;
constexpr int CONF_WAVES = CONF_TPB / 64;
constexpr int CONF_MAX_BLOCKS = 1024;
// One workgroup may hold the CU's whole LDS, 160 KiB (MI355X_MICROARCH.md, "Occupancy"); 512 bytes are left as the
// other kernels of the library leave them.  The small route privatises K*K + 2K + 2 uint32 counters there.
constexpr int CONF_LDS_BYTES = 160 * 1024 - 512;
constexpr long conf_counters(long K) { return K * K + 2 * K + 2; }
constexpr int conf_small_kmax() {
  int k = 1;
  while (conf_counters(k + 1) * (long)sizeof(unsigned) <= CONF_LDS_BYTES) ++k;
  return k;
}
constexpr int CONF_SMALL_KMAX = conf_small_kmax();
static_assert(CONF_SMALL_KMAX == 201, "K = 201: 40 805 counters = 163 220 B; K = 202 needs 164 840 B");

typedef unsigned long long u64;

// What one sweep over (a part of) a row leaves: the largest value with its lowest index, the number of classes in front
// of the label, and whether a value was not finite.
struct RowScan {
  float best;
  int arg;
  int rank;
  int nf;
};
__device__ __forceinline__ RowScan scan_init() { return RowScan{-INFINITY, 0, 0, 0}; }
// indices arrive in ascending order, so `>` keeps the lowest index of equal values; every finite value is > -inf, so
// `arg` of a finite row is the index of a value that was read
__device__ __forceinline__ void scan_one(RowScan& s, float v, int j, float xl, long l) {
  s.nf |= !isfinite(v);
  s.rank += beats_label(v, xl, j, l);
  if (v > s.best) {
    s.best = v;
    s.arg = j;
  }
}

// ---------------------------------------------------------------------------------------------- small K
// One thread per row; the counters of the workgroup's rows live in LDS (uint32: a workgroup sees fewer than 2^32 rows),
// and the non-zero ones go to global memory once, with one 64-bit integer atomic each.  VEC: every row starts on 16
// bytes (pointer aligned, ld % 4 == 0): 16-byte loads and a scalar tail; otherwise 4-byte loads.
template <bool VEC>
__global__ __launch_bounds__(CONF_TPB) void confusion_small_kernel(const float* __restrict__ preds, int ld,
                                                                   const long* __restrict__ labels, int N, int K,
                                                                   int k_hi, u64* __restrict__ conf,
                                                                   u64* __restrict__ hits, u64* __restrict__ refused) {
  extern __shared__ unsigned s_cnt[];
  const int KK = K * K, n_hits = 2 * K;  // K <= CONF_SMALL_KMAX: no overflow
  const int total = KK + n_hits + 2;
  for (int i = threadIdx.x; i < total; i += CONF_TPB) s_cnt[i] = 0u;
  __syncthreads();
  for (long r = (long)blockIdx.x * CONF_TPB + threadIdx.x; r < N; r += (long)gridDim.x * CONF_TPB) {
    const long l = labels[r];
    if (l < 0 || l >= K) {  // never a read of the row
      atomicAdd(&s_cnt[KK + n_hits], 1u);
      continue;
    }
    const float* x = preds + r * ld;
    const float xl = x[l];
    RowScan s = scan_init();
    int j = 0;
    if (VEC) {
      for (; j + 3 < K; j += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) scan_one(s, v[e], j + e, xl, l);
      }
    }
    for (; j < K; ++j) scan_one(s, x[j], j, xl, l);
    if (s.nf) {
      atomicAdd(&s_cnt[KK + n_hits + 1], 1u);
      continue;
    }
    atomicAdd(&s_cnt[(int)l * K + s.arg], 1u);
    if (s.rank < 1) atomicAdd(&s_cnt[KK + 2 * (int)l], 1u);
    if (s.rank < k_hi) atomicAdd(&s_cnt[KK + 2 * (int)l + 1], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += CONF_TPB) {
    const unsigned c = s_cnt[i];
    if (c == 0u) continue;
    u64* dst = i < KK ? conf + i : (i < KK + n_hits ? hits + (i - KK) : refused + (i - KK - n_hits));
    atomicAdd(dst, (u64)c);
  }
}

// ---------------------------------------------------------------------------------------------- large K
// One wavefront per row: every lane sweeps its share in ascending order, the butterfly keeps the larger value and of
// equal values the lower index; lane 0 adds one counter of conf and at most two of hits.  VEC as above.
template <bool VEC>
__global__ __launch_bounds__(CONF_TPB) void confusion_wave_kernel(const float* __restrict__ preds, int ld,
                                                                  const long* __restrict__ labels, int N, int K,
                                                                  int k_hi, u64* __restrict__ conf,
                                                                  u64* __restrict__ hits, u64* __restrict__ refused) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long r = (long)blockIdx.x * CONF_WAVES + wave; r < N; r += (long)gridDim.x * CONF_WAVES) {
    const long l = labels[r];  // the same in every lane: the branches below are taken by whole wavefronts
    if (l < 0 || l >= K) {
      if (lane == 0) atomicAdd(refused, (u64)1);
      continue;
    }
    const float* x = preds + r * ld;
    const float xl = x[l];
    RowScan s = scan_init();
    if (VEC) {
      const int kv = K & ~3;
      for (int j = 4 * lane; j < kv; j += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) scan_one(s, v[e], j + e, xl, l);
      }
      if (kv + lane < K) scan_one(s, x[kv + lane], kv + lane, xl, l);
    } else {
      for (int j = lane; j < K; j += 64) scan_one(s, x[j], j, xl, l);
    }
    const int rank = wave_sum(s.rank);
    const int nf = wave_sum(s.nf);
    float best = s.best;
    int arg = s.arg;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oa = __shfl_xor(arg, o, 64);
      if (ov > best || (ov == best && oa < arg)) {
        best = ov;
        arg = oa;
      }
    }
    if (lane == 0) {
      if (nf != 0) {
        atomicAdd(refused + 1, (u64)1);
      } else {
        atomicAdd(conf + l * K + arg, (u64)1);
        if (rank < 1) atomicAdd(hits + 2 * l, (u64)1);
        if (rank < k_hi) atomicAdd(hits + 2 * l + 1, (u64)1);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- the report
constexpr int REP_TPB = 1024;
constexpr int REP_WAVES = REP_TPB / 64;
constexpr int REP_KMAX = 1024;

__device__ __forceinline__ long wave_sum_i64(long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (long)__shfl_xor((long long)v, o, 64);
  return v;
}

// ONE workgroup.  Row sums (support) a wavefront per row, column sums (predicted counts) a thread per column: both
// read along rows.  Thread c then makes class c's five ratios, each ONE fp64 division of exact integers (0 for a zero
// denominator); thread 0 adds the classes in index order.
__global__ __launch_bounds__(REP_TPB) void class_report_kernel(const long* __restrict__ conf,
                                                               const long* __restrict__ hits, int K,
                                                               double* __restrict__ out,
                                                               double* __restrict__ per_class) {
  __shared__ long s_sup[REP_KMAX];
  __shared__ long s_col[REP_KMAX];
  __shared__ long s_tp[REP_KMAX];
  __shared__ double s_p[REP_KMAX];
  __shared__ double s_r[REP_KMAX];
  __shared__ double s_f[REP_KMAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < K; r += REP_WAVES) {
    const long* row = conf + (long)r * K;
    long s = 0;
    for (int j = lane; j < K; j += 64) s += row[j];
    s = wave_sum_i64(s);
    if (lane == 0) s_sup[r] = s;
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < K) {
    long col = 0;
    for (int j = 0; j < K; ++j) col += conf[(long)j * K + c];
    const long tp = conf[(long)c * K + c], sup = s_sup[c];
    const long fp = col - tp, fn = sup - tp;
    const double p = tp + fp > 0 ? (double)tp / (double)(tp + fp) : 0.0;
    const double r = sup > 0 ? (double)tp / (double)sup : 0.0;
    const double f = 2 * tp + fp + fn > 0 ? (double)(2 * tp) / (double)(2 * tp + fp + fn) : 0.0;
    double* o = per_class + (long)c * 6;
    o[0] = (double)sup;
    o[1] = p;
    o[2] = r;
    o[3] = f;
    o[4] = sup > 0 ? (double)hits[2 * c] / (double)sup : 0.0;
    o[5] = sup > 0 ? (double)hits[2 * c + 1] / (double)sup : 0.0;
    s_col[c] = col;
    s_tp[c] = tp;
    s_p[c] = p;
    s_r[c] = r;
    s_f[c] = f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long samples = 0, correct = 0, with_support = 0, never = 0;
    double sp = 0.0, sr = 0.0, sf = 0.0;
    for (int k = 0; k < K; ++k) {
      samples += s_sup[k];
      correct += s_tp[k];
      never += s_col[k] == 0 ? 1 : 0;
      if (s_sup[k] > 0) {
        with_support += 1;
        sp += s_p[k];
        sr += s_r[k];
        sf += s_f[k];
      }
    }
    const double n = (double)with_support;
    out[0] = (double)samples;
    out[1] = samples > 0 ? (double)correct / (double)samples : 0.0;
    out[2] = with_support > 0 ? sr / n : 0.0;
    out[3] = with_support > 0 ? sp / n : 0.0;
    out[4] = with_support > 0 ? sr / n : 0.0;
    out[5] = with_support > 0 ? sf / n : 0.0;
    out[6] = n;
    out[7] = (double)never;
  }
}

// ---------------------------------------------------------------------------------------------- class weights
// ONE workgroup.  Support = row sums of conf (a wavefront per row, as above); thread 0 counts the samples S and the
// classes with support K+ in class order; thread c then makes class c's weight, 0 for a class without support.
//   balanced:  S / (K+ * support[c]) — ONE fp64 division of exact integers, rounded once to fp32.
//   effective: e[c] = (1 - beta) / (1 - beta^support[c]) in fp64, times K+ / sum(e) (the sum in class order).
__global__ __launch_bounds__(REP_TPB) void class_weights_kernel(const long* __restrict__ conf, int K, int scheme,
                                                                double beta, float* __restrict__ w) {
  __shared__ long s_sup[REP_KMAX];
  __shared__ double s_e[REP_KMAX];
  __shared__ long s_tot[2];  // S, K+
  __shared__ double s_scale;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < K; r += REP_WAVES) {
    const long* row = conf + (long)r * K;
    long s = 0;
    for (int j = lane; j < K; j += 64) s += row[j];
    s = wave_sum_i64(s);
    if (lane == 0) s_sup[r] = s;
  }
  __syncthreads();
  const int c = threadIdx.x;
  const long sup = c < K ? s_sup[c] : 0;
  if (scheme == SF_WEIGHTS_EFFECTIVE && c < K) s_e[c] = sup > 0 ? (1.0 - beta) / (1.0 - pow(beta, (double)sup)) : 0.0;
  __syncthreads();
  if (threadIdx.x == 0) {
    long samples = 0, with_support = 0;
    double se = 0.0;
    for (int k = 0; k < K; ++k) {
      samples += s_sup[k] > 0 ? s_sup[k] : 0;
      with_support += s_sup[k] > 0 ? 1 : 0;
      if (scheme == SF_WEIGHTS_EFFECTIVE) se += s_e[k];
    }
    s_tot[0] = samples;
    s_tot[1] = with_support;
    s_scale = se > 0.0 ? (double)with_support / se : 0.0;
  }
  __syncthreads();
  if (c < K) {
    float v = 0.f;
    if (sup > 0) {
      v = scheme == SF_WEIGHTS_EFFECTIVE ? (float)(s_e[c] * s_scale)
                                         : (float)((double)s_tot[0] / (double)(s_tot[1] * sup));
    }
    w[c] = v;
  }
}

template <bool VEC>
int launch_confusion(const float* preds, int ld, const long* labels, int N, int K, int k_hi, u64* conf, u64* hits,
                     u64* refused, hipStream_t s) {
  if (K <= CONF_SMALL_KMAX) {
    const size_t lds = (size_t)conf_counters(K) * sizeof(unsigned);
    static SfLdsAttr at;
    if (lds > 64 * 1024 &&
        !sf_ensure_dyn_lds(at, reinterpret_cast<const void*>(confusion_small_kernel<VEC>), CONF_LDS_BYTES))
      return SF_ELAUNCH;
    const long blocks = ((long)N + CONF_TPB - 1) / CONF_TPB;
    hipLaunchKernelGGL(confusion_small_kernel<VEC>, dim3((unsigned)(blocks < CONF_MAX_BLOCKS ? blocks : CONF_MAX_BLOCKS)),
                       dim3(CONF_TPB), lds, s, preds, ld, labels, N, K, k_hi, conf, hits, refused);
  } else {
    const long blocks = ((long)N + CONF_WAVES - 1) / CONF_WAVES;
    hipLaunchKernelGGL(confusion_wave_kernel<VEC>, dim3((unsigned)(blocks < CONF_MAX_BLOCKS ? blocks : CONF_MAX_BLOCKS)),
                       dim3(CONF_TPB), 0, s, preds, ld, labels, N, K, k_hi, conf, hits, refused);
  }
  SF_CHECK_LAUNCH();
  return SF_OK;
}
}  // namespace

extern "C" int sf_confusion_small_kmax(void) { return CONF_SMALL_KMAX; }

extern "C" int sf_confusion_update(const float* preds, int ld, const long* labels, int N, int K, int k_hi, long* conf,
                                   long* hits, long* refused, void* stream) {
  if (!preds || !labels || !conf || !hits || !refused) return SF_EINVAL;
  if (N <= 0 || K <= 0 || ld < K || k_hi < 1 || k_hi > K) return SF_EINVAL;
  if (reinterpret_cast<uintptr_t>(preds) & 3) return SF_EALIGN;
  if ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(conf) | reinterpret_cast<uintptr_t>(hits) |
       reinterpret_cast<uintptr_t>(refused)) & 7)
    return SF_EALIGN;
  u64* c = reinterpret_cast<u64*>(conf);
  u64* h = reinterpret_cast<u64*>(hits);
  u64* f = reinterpret_cast<u64*>(refused);
  if (sf_aligned16(preds) && ld % 4 == 0 && K >= 4)
    return launch_confusion<true>(preds, ld, labels, N, K, k_hi, c, h, f, (hipStream_t)stream);
  return launch_confusion<false>(preds, ld, labels, N, K, k_hi, c, h, f, (hipStream_t)stream);
}

extern "C" int sf_class_report(const long* conf, const long* hits, int K, double* out, double* per_class, void* stream) {
  if (!conf || !hits || !out || !per_class) return SF_EINVAL;
  if (K <= 0 || K > REP_KMAX) return SF_EINVAL;
  if ((reinterpret_cast<uintptr_t>(conf) | reinterpret_cast<uintptr_t>(hits) | reinterpret_cast<uintptr_t>(out) |
       reinterpret_cast<uintptr_t>(per_class)) & 7)
    return SF_EALIGN;
  hipLaunchKernelGGL(class_report_kernel, dim3(1), dim3(REP_TPB), 0, (hipStream_t)stream, conf, hits, K, out, per_class);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_class_weights(const long* conf, int K, int scheme, const double* beta, float* w, void* stream) {
  if (!conf || !w) return SF_EINVAL;
  if (K <= 0 || K > REP_KMAX) return SF_EINVAL;
  if (scheme != SF_WEIGHTS_BALANCED && scheme != SF_WEIGHTS_EFFECTIVE) return SF_EINVAL;
  double b = 0.0;
  if (scheme == SF_WEIGHTS_EFFECTIVE) {  // beta is read here, on the host, before the launch
    if (!beta || !(*beta > 0.0 && *beta < 1.0)) return SF_EINVAL;
    b = *beta;
  }
  if ((reinterpret_cast<uintptr_t>(conf) & 7) || (reinterpret_cast<uintptr_t>(w) & 3)) return SF_EALIGN;
  hipLaunchKernelGGL(class_weights_kernel, dim3(1), dim3(REP_TPB), 0, (hipStream_t)stream, conf, K, scheme, b, w);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
