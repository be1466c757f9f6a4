// step_tail.hip — what follows the backward pass in tools/train_net.py:67-157: the loss with its gradient and the
// meter's top-k counts in one launch (sf_ce_topk; sf_bce for the multi-label and detection losses; sf_ce_topk_w and
// sf_bce_w are the same launches with class weights read from device memory), torch.optim.SGD over
// every parameter of every group in one launch (sf_sgd_step), torch.optim.Adam in two (sf_adam_step: the step counts,
// then the update), torch.optim.AdamW the same way (sf_adamw_step: the same kernel body with the decay decoupled) and SGD
// behind a per-tensor trust ratio (sf_lars_sgd_step: sf_sgd_step's body reading {r, wd_t} per tensor from the array
// lars.hip::sf_lars_ratios leaves in device memory).  Nothing here needs the host: the statistics go to a ring in device memory that the meter drains once
// per LOG_PERIOD, the hyper-parameters are read from device memory (the LR schedule is a 4-byte write a replayed graph
// sees) and a non-finite loss switches the update off through a flag the loss kernel leaves.
#include "chunk_table.h"
#include "common.h"
#include "mix_row.h"
#include "stats_row.h"

#include <math.h>

#include <cmath>

namespace {
// ---------------------------------------------------------------------------------------------- loss + top-k
// ONE workgroup: the real sizes are N = 2..64 rows of K = 27..700 logits (45k floats at most, read from L2 after the
// first pass), so a second workgroup would only add a hand-over.  A wavefront owns rows w, w + 16, ...; a row is three
// lane-strided sweeps (max + rank of the label, sum of exp, gradient).  exp / log / the sums run in fp64: at these sizes
// that is free and every stored float is the rounded exact value.  Order of every sum is fixed (lane stride, xor
// butterfly, rows in order per wavefront, wavefronts in order): equal bits run to run, no atomics.
// WEIGHTED (sf_ce_topk_w): F.cross_entropy(weight = wgt): row r counts wgt[labels[r]] times and the divisor is W, the sum
// of those weights over the rows with a valid label, instead of N.  W comes first, in the same launch: thread t adds
// the weights of rows t, t + 1024, ..., xor butterfly, wavefronts in order, one barrier — every thread then holds the
// same W.  The row's factor is w * (1 / W) and the mean tot * (1 / W): with every weight 1.0f and every label valid
// these are the unweighted 1 / N and tot * (1 / N) bit for bit.  W == 0 (every present class has weight 0; torch
// returns NaN), or a W that is not finite: the loss is NaN, the flag 1 and dlogits all zeros.
// MIX (sf_ce_mix): the target of row r is t = (1 - eps) (lam onehot(a) + (1 - lam) onehot(b)) + eps / K with a the row's
// label, b its partner's and lam from the row's mix row — two labels, one weight and one scalar instead of an N x K
// tensor.  The loss needs sum_j t_j x_j = (1 - eps) (lam x_a + (1 - lam) x_b) + (eps / K) sum_j x_j: the sum of the row
// rides in the exp sweep.  The hits are counted against the dominant label (a when lam >= 0.5, else b).  At eps = 0
// and lam = 1 the products are by one and the added terms exact zeros (finite logits): sf_ce_topk's bits.
__device__ __forceinline__ double ce_weight_total(const long* __restrict__ labels, const float* __restrict__ wgt, int N,
                                                  int K) {
  __shared__ double s_w[CE_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double ws = 0.0;
  for (int r = threadIdx.x; r < N; r += CE_TPB) {
    const long l = labels[r];
    if (l >= 0 && l < K) ws += (double)wgt[l];
  }
  ws = wave_sum(ws);
  if (lane == 0) s_w[wave] = ws;
  __syncthreads();
  double wtot = 0.0;
  for (int w = 0; w < CE_WAVES; ++w) wtot += s_w[w];
  return wtot;
}

template <bool WEIGHTED, bool MIX = false>
__device__ __forceinline__ void ce_topk_body(const float* __restrict__ logits, int ld, const long* __restrict__ labels,
                                             const float* __restrict__ wgt, int N, int K, int k_hi,
                                             float* __restrict__ dlogits, float* __restrict__ ring,
                                             int* __restrict__ counter, int cap, float* __restrict__ loss_out,
                                             const long* __restrict__ mix = nullptr, float smoothing = 0.f) {
  static_assert(!(WEIGHTED && MIX), "class weights and soft targets divide differently: not offered together");
  __shared__ double s_loss[CE_WAVES];
  __shared__ int s_cnt[CE_WAVES][4];  // top-1 hits, top-k_hi hits, rows with a non-finite logit, bad labels
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double wtot = WEIGHTED ? ce_weight_total(labels, wgt, N, K) : (double)N;
  const bool w_ok = !WEIGHTED || (wtot > 0.0 && isfinite(wtot));
  const double inv_n = 1.0 / wtot;  // WEIGHTED: 1 / W
  const double keep = MIX ? 1.0 - (double)smoothing : 1.0;         // 1 - eps
  const double uni = MIX ? (double)smoothing / (double)K : 0.0;    // eps / K
  double loss = 0.0;
  int hit1 = 0, hitk = 0, nonfinite = 0, bad = 0;
  for (int r = wave; r < N; r += CE_WAVES) {
    const float* x = logits + (long)r * ld;
    float* dx = dlogits + (long)r * K;
    long l = labels[r];
    bool ok = l >= 0 && l < K;  // a label outside [0, K): no loss, no gradient, never a read
    long la = l, lb = l;        // MIX: the row's own label and its partner's
    double lam = 1.0, xa = 0.0, xb = 0.0;
    if (MIX) {
      long p = r;
      if (mix != nullptr) {  // the host entry checked its copy; a device row that differs is a bad row, never a read
        const long* mr = mix + (long)r * MIX_ROW;
        const bool pair = mix_pair_ok(mr, N);
        ok = ok && pair;
        if (pair) {
          p = mr[0];
          lam = (double)mix_lambda(mr[2]);
        }
      }
      lb = labels[p];
      ok = ok && lb >= 0 && lb < K;
      l = lam >= 0.5 ? la : lb;  // the dominant label: what the hits are counted against
      if (ok) {
        xa = (double)x[la];
        xb = (double)x[lb];
      }
    }
    const float xl = ok ? x[l] : 0.f;
    const double wr = (WEIGHTED && ok) ? (double)wgt[l] : 1.0;
    const double fac = WEIGHTED ? wr * inv_n : inv_n;
    const bool grad = WEIGHTED ? (ok && w_ok) : ok;
    float m = -INFINITY;
    int rank = 0, nf = 0;
    for (int j = lane; j < K; j += 64) {
      const float v = x[j];
      m = fmaxf(m, v);
      nf |= !isfinite(v);
      rank += beats_label(v, xl, j, l);  // ties go to the lower index
    }
    m = wave_max(m);
    rank = wave_sum(rank);
    nf = wave_sum(nf) != 0;
    double s = 0.0, sx = 0.0;
    if (MIX) {
      for (int j = lane; j < K; j += 64) {
        s += exp((double)x[j] - (double)m);
        sx += (double)x[j];
      }
    } else {
      for (int j = lane; j < K; j += 64) s += exp((double)x[j] - (double)m);  // NaN / Inf propagate from here
    }
    s = wave_sum(s);
    if (MIX) sx = wave_sum(sx);
    const double inv_s = 1.0 / s;
    if (MIX) {
      const double lam_b = 1.0 - lam;
      for (int j = lane; j < K; j += 64) {
        const double p = exp((double)x[j] - (double)m) * inv_s;
        const double t = keep * (lam * (j == la ? 1.0 : 0.0) + lam_b * (j == lb ? 1.0 : 0.0)) + uni;
        dx[j] = grad ? (float)((p - t) * fac) : 0.f;
      }
    } else {
      for (int j = lane; j < K; j += 64) {
        const double p = exp((double)x[j] - (double)m) * inv_s;
        dx[j] = grad ? (float)((p - (j == l ? 1.0 : 0.0)) * fac) : 0.f;
      }
    }
    if (ok) {
      if (WEIGHTED)
        loss += wr * (log(s) + (double)m - (double)xl);
      else if (MIX)
        loss += log(s) + (double)m - (keep * (lam * xa + (1.0 - lam) * xb) + uni * sx);
      else
        loss += log(s) + (double)m - (double)xl;
      if (!nf) {  // a row with a NaN or an Inf is wrong for every k
        hit1 += rank < 1;
        hitk += rank < k_hi;
      }
    } else {
      bad += 1;
    }
    // WEIGHTED: a row that is left out (torch's ignore_index) is left out whole — what it holds does not reach the flag
    nonfinite += (WEIGHTED && !ok) ? 0 : nf;
  }
  if (lane == 0) {
    s_loss[wave] = loss;
    s_cnt[wave][0] = hit1;
    s_cnt[wave][1] = hitk;
    s_cnt[wave][2] = nonfinite;
    s_cnt[wave][3] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    int c[4] = {0, 0, 0, 0};
    for (int w = 0; w < CE_WAVES; ++w) {
      tot += s_loss[w];
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] += s_cnt[w][i];
    }
    const float mean = (!WEIGHTED || w_ok) ? (float)(tot * inv_n) : NAN;
    const float flag = (c[2] != 0 || !isfinite(mean)) ? 1.f : 0.f;
    const int step = counter[0];
    const int slot = ((step % cap) + cap) % cap;
    float* row = ring + (long)slot * RING_ROW;
    const float n = (float)N;
    row[0] = mean;
    row[1] = topk_error_pct(c[0], n);  // train_net.py:123-125, in float32 as there
    row[2] = topk_error_pct(c[1], n);
    row[3] = flag;
    row[4] = n;
    row[5] = (float)c[3];
    row[6] = 0.f;
    row[7] = 0.f;
    loss_out[0] = mean;
    loss_out[1] = flag;
    counter[0] = step + 1;  // the only writer: a plain store
  }
}

__global__ __launch_bounds__(CE_TPB) void ce_topk_kernel(const float* __restrict__ logits, int ld,
                                                         const long* __restrict__ labels, int N, int K, int k_hi,
                                                         float* __restrict__ dlogits, float* __restrict__ ring,
                                                         int* __restrict__ counter, int cap,
                                                         float* __restrict__ loss_out) {
  ce_topk_body<false>(logits, ld, labels, nullptr, N, K, k_hi, dlogits, ring, counter, cap, loss_out);
}

__global__ __launch_bounds__(CE_TPB) void ce_topk_w_kernel(const float* __restrict__ logits, int ld,
                                                           const long* __restrict__ labels,
                                                           const float* __restrict__ wgt, int N, int K, int k_hi,
                                                           float* __restrict__ dlogits, float* __restrict__ ring,
                                                           int* __restrict__ counter, int cap,
                                                           float* __restrict__ loss_out) {
  ce_topk_body<true>(logits, ld, labels, wgt, N, K, k_hi, dlogits, ring, counter, cap, loss_out);
}

__global__ __launch_bounds__(CE_TPB) void ce_mix_kernel(const float* __restrict__ logits, int ld,
                                                        const long* __restrict__ labels, const long* __restrict__ mix,
                                                        int N, int K, int k_hi, float smoothing,
                                                        float* __restrict__ dlogits, float* __restrict__ ring,
                                                        int* __restrict__ counter, int cap,
                                                        float* __restrict__ loss_out) {
  ce_topk_body<false, true>(logits, ld, labels, nullptr, N, K, k_hi, dlogits, ring, counter, cap, loss_out, mix,
                            smoothing);
}

// ---------------------------------------------------------------------------------------------- BCE
// nn.BCELoss / nn.BCEWithLogitsLoss (mean) with the gradient, a ring row and the flag.  ONE workgroup as above: the real
// sizes are boxes x 80 (AVA) or clips x 157 (Charades), ~1e4 elements.  Thread i owns elements i, i + 1024, ... of the
// flattened [N][K]; log / exp / log1p and the sums in fp64, fixed order (thread stride, xor butterfly, wavefronts in
// order): equal bits run to run, no atomics.
// WEIGHTED (sf_bce_w): nn.BCELoss(weight = wgt[K]) / nn.BCEWithLogitsLoss(weight = wgt[K], pos_weight = pos[K]); either
// vector may be null (= all ones).  Element (r, j) counts wgt[j] times and the divisor stays N * K, as in torch.  With
// logits and p = pos[j]:  loss = (1 - y) x + (1 + (p - 1) y) softplus(-x), written as the unweighted loss plus
// (p - 1) y softplus(-x), and the gradient as (sigmoid - y) + (p - 1) y (sigmoid - 1): at p = 1 the added terms are
// exact zeros, and a weight of 1 is a multiply by one — all-ones vectors give sf_bce's bits.
template <bool WEIGHTED>
__device__ __forceinline__ void bce_body(const float* __restrict__ x, int ldx, const float* __restrict__ y, int ldy,
                                         const float* __restrict__ wgt, const float* __restrict__ pos, int N, int K,
                                         int from_logits, float* __restrict__ dx, float* __restrict__ ring,
                                         int* __restrict__ counter, int cap, float* __restrict__ loss_out) {
  __shared__ double s_loss[CE_WAVES];
  __shared__ int s_cnt[CE_WAVES][2];  // elements with a NaN / Inf input, elements outside [0, 1]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long total = (long)N * K;
  const double inv = 1.0 / (double)total;
  double loss = 0.0;
  int nonfinite = 0, bad = 0;
  for (long e = threadIdx.x; e < total; e += CE_TPB) {
    const long r = e / K;
    const int j = (int)(e - r * K);
    const float xf = x[r * ldx + j], yf = y[r * ldy + j];
    const double xv = (double)xf, yv = (double)yf;
    const bool nf = !isfinite(xf) || !isfinite(yf);
    const double wj = (WEIGHTED && wgt != nullptr) ? (double)wgt[j] : 1.0;
    const double winv = WEIGHTED ? wj * inv : inv;
    double l, d;
    if (from_logits) {
      const double t = exp(-fabs(xv));  // in (0, 1]: no overflow at any x; log1p keeps it where 1 + t == 1
      l = fmax(xv, 0.0) - xv * yv + log1p(t);
      if (!WEIGHTED) {
        d = ((xv >= 0.0 ? 1.0 / (1.0 + t) : t / (1.0 + t)) - yv) * inv;
      } else {
        const double sig = xv >= 0.0 ? 1.0 / (1.0 + t) : t / (1.0 + t);
        d = sig - yv;
        if (pos != nullptr) {
          const double py = ((double)pos[j] - 1.0) * yv;
          l += py * (fmax(-xv, 0.0) + log1p(t));
          d += py * (sig - 1.0);
        }
        d *= winv;
      }
    } else if (nf || (xf >= 0.f && xf <= 1.f && yf >= 0.f && yf <= 1.f)) {
      // torch's binary_cross_entropy: both logs clamped at -100, the gradient's denominator at 1e-12
      l = -(yv * fmax(log(xv), -100.0) + (1.0 - yv) * fmax(log(1.0 - xv), -100.0));
      double den = xv * (1.0 - xv);
      den = den < 1e-12 ? 1e-12 : den;  // (a NaN stays one)
      d = (xv - yv) / den * winv;
    } else {  // where torch asserts on the device: no loss, no gradient; the divisor stays N * K
      l = 0.0;
      d = 0.0;
      bad += 1;
    }
    if (nf) {  // fmax drops a NaN: say it outright
      l = (double)NAN;
      nonfinite += 1;
    }
    if (WEIGHTED)
      loss += wj * l;
    else
      loss += l;
    dx[e] = (float)d;
  }
  loss = wave_sum(loss);
  nonfinite = wave_sum(nonfinite);
  bad = wave_sum(bad);
  if (lane == 0) {
    s_loss[wave] = loss;
    s_cnt[wave][0] = nonfinite;
    s_cnt[wave][1] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    int c[2] = {0, 0};
    for (int w = 0; w < CE_WAVES; ++w) {
      tot += s_loss[w];
      c[0] += s_cnt[w][0];
      c[1] += s_cnt[w][1];
    }
    const float mean = (float)(tot * inv);
    const float flag = (c[0] != 0 || !isfinite(mean)) ? 1.f : 0.f;
    const int step = counter[0];
    const int slot = ((step % cap) + cap) % cap;
    float* row = ring + (long)slot * RING_ROW;
    row[0] = mean;
    row[1] = 0.f;
    row[2] = 0.f;
    row[3] = flag;
    row[4] = (float)N;
    row[5] = (float)c[1];
    row[6] = KIND_BCE;
    row[7] = 0.f;
    loss_out[0] = mean;
    loss_out[1] = flag;
    counter[0] = step + 1;  // the only writer: a plain store
  }
}

__global__ __launch_bounds__(CE_TPB) void bce_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ y,
                                                     int ldy, int N, int K, int from_logits, float* __restrict__ dx,
                                                     float* __restrict__ ring, int* __restrict__ counter, int cap,
                                                     float* __restrict__ loss_out) {
  bce_body<false>(x, ldx, y, ldy, nullptr, nullptr, N, K, from_logits, dx, ring, counter, cap, loss_out);
}

__global__ __launch_bounds__(CE_TPB) void bce_w_kernel(const float* __restrict__ x, int ldx,
                                                       const float* __restrict__ y, int ldy,
                                                       const float* __restrict__ wgt, const float* __restrict__ pos,
                                                       int N, int K, int from_logits, float* __restrict__ dx,
                                                       float* __restrict__ ring, int* __restrict__ counter, int cap,
                                                       float* __restrict__ loss_out) {
  bce_body<true>(x, ldx, y, ldy, wgt, pos, N, K, from_logits, dx, ring, counter, cap, loss_out);
}

// ---------------------------------------------------------------------------------------------- SGD
constexpr int TAB_ROW = 6;  // parameter, gradient, momentum buffer (0: none), numel, group, first step
constexpr int HYP_ROW = 5;  // lr, weight_decay, momentum, dampening, nesterov

struct Hyper {
  float lr, wd, mom, keep;  // keep = 1 - dampening
  bool nesterov;
};

// torch/optim/sgd.py::_single_tensor_sgd for one element; returns the new parameter, *b the new momentum buffer.
// LARS (sf_lars_sgd_step): h.wd is the TENSOR's weight decay and the decayed gradient is scaled by the tensor's trust
// ratio r, one fp32 multiply; r == 1 is a multiply by one: sf_sgd_step's bits.
template <bool LARS>
__device__ __forceinline__ float sgd1(float p, float g, float* b, const Hyper& h, bool has_buf, bool first, float r) {
  if (h.wd != 0.f) g = fmaf(h.wd, p, g);
  if (LARS) g *= r;
  if (has_buf) {
    const float nb = first ? g : fmaf(h.mom, *b, h.keep * g);
    *b = nb;
    g = h.nesterov ? fmaf(h.mom, nb, g) : nb;
  }
  return fmaf(-h.lr, g, p);
}

template <bool LARS>
__device__ __forceinline__ void sgd_step_body(const long* __restrict__ table, const long* __restrict__ chunks,
                                              const float* __restrict__ hyper, const float* __restrict__ ratios,
                                              const float* __restrict__ guard, int n_tensors, int n_groups,
                                              int zero_grad) {
  if (guard != nullptr && guard[0] != 0.f) return;  // the step's loss was not finite (or NaN itself): no update
  Chunk c;
  if (!chunk_resolve(table, chunks, n_tensors, TAB_ROW, 3, &c)) return;
  const long* row = c.row;
  const long ti = c.ti, start = c.start, grp = row[4];
  if (row[0] == 0 || row[1] == 0 || grp < 0 || grp >= n_groups) return;
  const float* hy = hyper + grp * HYP_ROW;
  Hyper h;
  h.lr = hy[0];
  h.wd = hy[1];
  h.mom = hy[2];
  h.keep = 1.f - hy[3];
  h.nesterov = hy[4] != 0.f;
  float r = 1.f;
  if (LARS) {  // {r, wd_t} of this TENSOR, as sf_lars_ratios left them; the group's weight decay is not applied again
    r = ratios[2 * ti];
    h.wd = ratios[2 * ti + 1];
  }
  const bool has_buf = row[2] != 0 && h.mom != 0.f;
  const bool first = row[5] != 0;
  float* p = as_global(row[0]) + start;
  float* g = as_global(row[1]) + start;
  float* b = as_global(has_buf ? row[2] : row[0]) + start;  // never dereferenced without has_buf
  const int len = c.len;
  const unsigned long bits = (unsigned long)p | (unsigned long)g | (unsigned long)b;
  if ((bits & 15) == 0) {
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += CHUNK_TPB) {
      f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
      const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
      f32x4 bv = {0.f, 0.f, 0.f, 0.f};
      if (has_buf && !first) bv = reinterpret_cast<f32x4*>(b)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float be = bv[e];
        pv[e] = sgd1<LARS>(pv[e], gv[e], &be, h, has_buf, first, r);
        bv[e] = be;
      }
      reinterpret_cast<f32x4*>(p)[i] = pv;
      if (has_buf) reinterpret_cast<f32x4*>(b)[i] = bv;
      if (zero_grad) reinterpret_cast<f32x4*>(g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int i = (n4 << 2) + threadIdx.x;  // up to three elements left
    if (i < len) {
      float be = (has_buf && !first) ? b[i] : 0.f;
      p[i] = sgd1<LARS>(p[i], g[i], &be, h, has_buf, first, r);
      if (has_buf) b[i] = be;
      if (zero_grad) g[i] = 0.f;
    }
  } else {
    for (int i = threadIdx.x; i < len; i += CHUNK_TPB) {
      float be = (has_buf && !first) ? b[i] : 0.f;
      p[i] = sgd1<LARS>(p[i], g[i], &be, h, has_buf, first, r);
      if (has_buf) b[i] = be;
      if (zero_grad) g[i] = 0.f;
    }
  }
}

__global__ __launch_bounds__(CHUNK_TPB) void sgd_step_kernel(const long* __restrict__ table,
                                                           const long* __restrict__ chunks,
                                                           const float* __restrict__ hyper,
                                                           const float* __restrict__ guard, int n_tensors, int n_groups,
                                                           int zero_grad) {
  sgd_step_body<false>(table, chunks, hyper, nullptr, guard, n_tensors, n_groups, zero_grad);
}

__global__ __launch_bounds__(CHUNK_TPB) void lars_sgd_step_kernel(const long* __restrict__ table,
                                                                const long* __restrict__ chunks,
                                                                const float* __restrict__ hyper,
                                                                const float* __restrict__ ratios,
                                                                const float* __restrict__ guard, int n_tensors,
                                                                int n_groups, int zero_grad) {
  sgd_step_body<true>(table, chunks, hyper, ratios, guard, n_tensors, n_groups, zero_grad);
}

bool sgd_tables_ok(const long* tab, int n_tensors, const long* chunks, int n_chunks, const float* hyper, int n_groups) {
  for (int t = 0; t < n_tensors; ++t) {
    const long* r = tab + (long)t * TAB_ROW;
    if (r[0] == 0 || r[1] == 0 || ((r[0] | r[1] | r[2]) & 3) != 0) return false;
    if (r[3] <= 0 || r[4] < 0 || r[4] >= n_groups || (r[5] != 0 && r[5] != 1)) return false;
    if (hyper[r[4] * HYP_ROW + 2] != 0.f && r[2] == 0) return false;  // momentum without a buffer
  }
  return chunks_tile(tab, TAB_ROW, 3, n_tensors, chunks, n_chunks);
}

// ---------------------------------------------------------------------------------------------- Adam
constexpr int ADAM_TAB_ROW = 7;  // parameter, gradient, exp_avg, exp_avg_sq, step (one float), numel, group
constexpr int ADAM_HYP_ROW = 5;  // lr, beta1, beta2, eps, weight_decay — fp64, what torch's Python floats are

// the step counts first, in a launch of their own: the update's chunks of one tensor all read the new value
__global__ __launch_bounds__(CHUNK_TPB) void adam_tick_kernel(const long* __restrict__ table,
                                                            const float* __restrict__ guard, int n_tensors) {
  if (guard != nullptr && guard[0] != 0.f) return;
  for (int t = threadIdx.x; t < n_tensors; t += CHUNK_TPB) {
    const long a = table[(long)t * ADAM_TAB_ROW + 4];
    if (a == 0) continue;
    float* s = as_global(a);
    s[0] += 1.f;
  }
}

struct AdamScalars {
  float w1, b2, w2, step_size, inv_bc2_sqrt, eps, wd;  // w_i = 1 - beta_i; DECOUPLED: wd holds 1 - lr * weight_decay
  int ok;
};

// torch/optim/adam.py::_single_tensor_adam (amsgrad = maximize = False) for one element; returns the new parameter.
// DECOUPLED (sf_adamw_step, torch.optim.AdamW): p *= 1 - lr * wd in front, nothing added to g.
template <bool DECOUPLED>
__device__ __forceinline__ float adam1(float p, float g, float* m, float* v, const AdamScalars& a) {
  if (DECOUPLED)
    p *= a.wd;
  else if (a.wd != 0.f)
    g = fmaf(a.wd, p, g);
  const float dm = g - *m;
  const float nm = a.w1 < 0.5f ? fmaf(a.w1, dm, *m) : g - dm * (1.f - a.w1);  // exp_avg.lerp_(grad, 1 - beta1)
  const float nv = fmaf(a.w2 * g, g, a.b2 * *v);
  *m = nm;
  *v = nv;
  const float denom = fmaf(sqrtf(nv), a.inv_bc2_sqrt, a.eps);
  return fmaf(-a.step_size, nm / denom, p);
}

template <bool DECOUPLED>
__device__ __forceinline__ void adam_step_body(const long* __restrict__ table, const long* __restrict__ chunks,
                                               const double* __restrict__ hyper, const float* __restrict__ guard,
                                               int n_tensors, int n_groups, int zero_grad) {
  __shared__ AdamScalars s_a;
  if (guard != nullptr && guard[0] != 0.f) return;  // as in sgd_step_kernel: nothing moves
  Chunk c;
  if (!chunk_resolve(table, chunks, n_tensors, ADAM_TAB_ROW, 5, &c)) return;
  const long* row = c.row;
  const long start = c.start, grp = row[6];
  if (row[0] == 0 || row[1] == 0 || row[2] == 0 || row[3] == 0 || row[4] == 0) return;
  if (grp < 0 || grp >= n_groups) return;
  if (threadIdx.x == 0) {  // the bias corrections once per workgroup, in fp64 as torch's Python floats
    const double* hy = hyper + grp * ADAM_HYP_ROW;
    const double lr = hy[0], b1 = hy[1], b2 = hy[2];
    const double t = (double)as_global(row[4])[0];
    const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
    AdamScalars a;
    a.w1 = (float)(1.0 - b1);
    a.b2 = (float)b2;
    a.w2 = (float)(1.0 - b2);
    a.step_size = (float)(lr / bc1);
    a.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    a.eps = (float)hy[3];
    a.wd = DECOUPLED ? (float)(1.0 - lr * hy[4]) : (float)hy[4];  // torch multiplies by the Python float 1 - lr * wd
    a.ok = t >= 1.0 && bc1 > 0.0 && bc2 > 0.0;  // a step count nobody advanced: leave the chunk alone
    s_a = a;
  }
  __syncthreads();
  const AdamScalars a = s_a;
  if (!a.ok) return;
  float* p = as_global(row[0]) + start;
  float* g = as_global(row[1]) + start;
  float* m = as_global(row[2]) + start;
  float* v = as_global(row[3]) + start;
  const int len = c.len;
  const unsigned long bits = (unsigned long)p | (unsigned long)g | (unsigned long)m | (unsigned long)v;
  if ((bits & 15) == 0) {
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += CHUNK_TPB) {
      f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
      const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
      f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
      f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float me = mv[e], ve = vv[e];
        pv[e] = adam1<DECOUPLED>(pv[e], gv[e], &me, &ve, a);
        mv[e] = me;
        vv[e] = ve;
      }
      reinterpret_cast<f32x4*>(p)[i] = pv;
      reinterpret_cast<f32x4*>(m)[i] = mv;
      reinterpret_cast<f32x4*>(v)[i] = vv;
      if (zero_grad) reinterpret_cast<f32x4*>(g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int i = (n4 << 2) + threadIdx.x;  // up to three elements left
    if (i < len) {
      float me = m[i], ve = v[i];
      p[i] = adam1<DECOUPLED>(p[i], g[i], &me, &ve, a);
      m[i] = me;
      v[i] = ve;
      if (zero_grad) g[i] = 0.f;
    }
  } else {
    for (int i = threadIdx.x; i < len; i += CHUNK_TPB) {
      float me = m[i], ve = v[i];
      p[i] = adam1<DECOUPLED>(p[i], g[i], &me, &ve, a);
      m[i] = me;
      v[i] = ve;
      if (zero_grad) g[i] = 0.f;
    }
  }
}

__global__ __launch_bounds__(CHUNK_TPB) void adam_step_kernel(const long* __restrict__ table,
                                                            const long* __restrict__ chunks,
                                                            const double* __restrict__ hyper,
                                                            const float* __restrict__ guard, int n_tensors,
                                                            int n_groups, int zero_grad) {
  adam_step_body<false>(table, chunks, hyper, guard, n_tensors, n_groups, zero_grad);
}

__global__ __launch_bounds__(CHUNK_TPB) void adamw_step_kernel(const long* __restrict__ table,
                                                             const long* __restrict__ chunks,
                                                             const double* __restrict__ hyper,
                                                             const float* __restrict__ guard, int n_tensors,
                                                             int n_groups, int zero_grad) {
  adam_step_body<true>(table, chunks, hyper, guard, n_tensors, n_groups, zero_grad);
}

bool adam_tables_ok(const long* tab, int n_tensors, const long* chunks, int n_chunks, const double* hyper,
                    int n_groups) {
  for (int g = 0; g < n_groups; ++g) {
    const double* h = hyper + (long)g * ADAM_HYP_ROW;
    for (int i = 0; i < ADAM_HYP_ROW; ++i)
      if (!std::isfinite(h[i])) return false;
    if (h[1] < 0.0 || h[1] >= 1.0 || h[2] < 0.0 || h[2] >= 1.0) return false;  // torch's own range: 1 - beta^t > 0
  }
  for (int t = 0; t < n_tensors; ++t) {
    const long* r = tab + (long)t * ADAM_TAB_ROW;
    for (int i = 0; i < 5; ++i)
      if (r[i] == 0 || (r[i] & 3) != 0) return false;
    if (r[5] <= 0 || r[6] < 0 || r[6] >= n_groups) return false;
  }
  return chunks_tile(tab, ADAM_TAB_ROW, 5, n_tensors, chunks, n_chunks);
}

// ---------------------------------------------------------------------------------------------- the entries' checks
bool ce_args_ok(const float* logits, int ld, const long* labels, int N, int K, int k_hi, float* dlogits, float* ring,
                int* counter, int cap, float* loss_out) {
  if (!logits || !labels || !dlogits || !ring || !counter || !loss_out) return false;
  return N > 0 && K > 0 && ld >= K && cap > 0 && k_hi >= 1 && k_hi <= K;
}

bool bce_args_ok(const float* x, int ldx, const float* y, int ldy, int N, int K, int from_logits, float* dx,
                 float* ring, int* counter, int cap, float* loss_out) {
  if (!x || !y || !dx || !ring || !counter || !loss_out) return false;
  return N > 0 && K > 0 && ldx >= K && ldy >= K && cap > 0 && (from_logits == 0 || from_logits == 1);
}

// sf_sgd_step and, with the ratios, sf_lars_sgd_step
template <bool LARS>
int sgd_entry(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
              int n_chunks, const float* hyper_host, const float* hyper, int n_groups, const float* ratios,
              const float* guard, int zero_grad, void* stream) {
  if (!tables_args_ok(table_host, table, n_tensors, chunks_host, chunks, n_chunks)) return SF_EINVAL;
  if (!hyper_host || !hyper || (LARS && !ratios)) return SF_EINVAL;
  if (n_groups <= 0 || (zero_grad != 0 && zero_grad != 1)) return SF_EINVAL;
  if (!sgd_tables_ok(table_host, n_tensors, chunks_host, n_chunks, hyper_host, n_groups)) return SF_EINVAL;
  if (LARS)
    hipLaunchKernelGGL(lars_sgd_step_kernel, dim3(n_chunks), dim3(CHUNK_TPB), 0, (hipStream_t)stream, table, chunks,
                       hyper, ratios, guard, n_tensors, n_groups, zero_grad);
  else
    hipLaunchKernelGGL(sgd_step_kernel, dim3(n_chunks), dim3(CHUNK_TPB), 0, (hipStream_t)stream, table, chunks, hyper,
                       guard, n_tensors, n_groups, zero_grad);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

// sf_adam_step and sf_adamw_step: the tick launch, then the step launch
template <bool DECOUPLED>
int adam_entry(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
               int n_chunks, const double* hyper_host, const double* hyper, int n_groups, const float* guard,
               int zero_grad, void* stream) {
  if (!tables_args_ok(table_host, table, n_tensors, chunks_host, chunks, n_chunks)) return SF_EINVAL;
  if (!hyper_host || !hyper || n_groups <= 0 || (zero_grad != 0 && zero_grad != 1)) return SF_EINVAL;
  if (!adam_tables_ok(table_host, n_tensors, chunks_host, n_chunks, hyper_host, n_groups)) return SF_EINVAL;
  hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(CHUNK_TPB), 0, (hipStream_t)stream, table, guard, n_tensors);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(DECOUPLED ? adamw_step_kernel : adam_step_kernel, dim3(n_chunks), dim3(CHUNK_TPB), 0,
                     (hipStream_t)stream, table, chunks, hyper, guard, n_tensors, n_groups, zero_grad);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
}  // namespace

extern "C" int sf_ce_topk(const float* logits, int ld, const long* labels, int N, int K, int k_hi, float* dlogits,
                          float* ring, int* counter, int cap, float* loss_out, void* stream) {
  if (!ce_args_ok(logits, ld, labels, N, K, k_hi, dlogits, ring, counter, cap, loss_out)) return SF_EINVAL;
  hipLaunchKernelGGL(ce_topk_kernel, dim3(1), dim3(CE_TPB), 0, (hipStream_t)stream, logits, ld, labels, N, K, k_hi,
                     dlogits, ring, counter, cap, loss_out);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_ce_topk_w(const float* logits, int ld, const long* labels, const float* weight, int N, int K, int k_hi,
                            float* dlogits, float* ring, int* counter, int cap, float* loss_out, void* stream) {
  if (!weight || !ce_args_ok(logits, ld, labels, N, K, k_hi, dlogits, ring, counter, cap, loss_out)) return SF_EINVAL;
  hipLaunchKernelGGL(ce_topk_w_kernel, dim3(1), dim3(CE_TPB), 0, (hipStream_t)stream, logits, ld, labels, weight, N, K,
                     k_hi, dlogits, ring, counter, cap, loss_out);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_ce_mix(const float* logits, int ld, const long* labels, const long* mix_host, const long* mix, int N,
                         int K, int k_hi, float smoothing, float* dlogits, float* ring, int* counter, int cap,
                         float* loss_out, void* stream) {
  if (!ce_args_ok(logits, ld, labels, N, K, k_hi, dlogits, ring, counter, cap, loss_out)) return SF_EINVAL;
  if (!(smoothing >= 0.f && smoothing < 1.f)) return SF_EINVAL;  // (a NaN fails both)
  if ((mix == nullptr) != (mix_host == nullptr)) return SF_EINVAL;
  if (mix_host != nullptr)
    for (int r = 0; r < N; ++r)
      if (!mix_row_ok(mix_host + (long)r * MIX_ROW, N)) return SF_EINVAL;
  hipLaunchKernelGGL(ce_mix_kernel, dim3(1), dim3(CE_TPB), 0, (hipStream_t)stream, logits, ld, labels, mix, N, K, k_hi,
                     smoothing, dlogits, ring, counter, cap, loss_out);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_sgd_chunk_elems(void) { return CHUNK_ELEMS; }

extern "C" int sf_sgd_step(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                           const long* chunks, int n_chunks, const float* hyper_host, const float* hyper, int n_groups,
                           const float* guard, int zero_grad, void* stream) {
  return sgd_entry<false>(table_host, table, n_tensors, chunks_host, chunks, n_chunks, hyper_host, hyper, n_groups,
                          nullptr, guard, zero_grad, stream);
}

extern "C" int sf_lars_sgd_step(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                                const long* chunks, int n_chunks, const float* hyper_host, const float* hyper,
                                int n_groups, const float* ratios, const float* guard, int zero_grad, void* stream) {
  return sgd_entry<true>(table_host, table, n_tensors, chunks_host, chunks, n_chunks, hyper_host, hyper, n_groups,
                         ratios, guard, zero_grad, stream);
}

extern "C" int sf_bce(const float* x, int ldx, const float* y, int ldy, int N, int K, int from_logits, float* dx,
                      float* ring, int* counter, int cap, float* loss_out, void* stream) {
  if (!bce_args_ok(x, ldx, y, ldy, N, K, from_logits, dx, ring, counter, cap, loss_out)) return SF_EINVAL;
  hipLaunchKernelGGL(bce_kernel, dim3(1), dim3(CE_TPB), 0, (hipStream_t)stream, x, ldx, y, ldy, N, K, from_logits, dx,
                     ring, counter, cap, loss_out);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_bce_w(const float* x, int ldx, const float* y, int ldy, const float* weight, const float* pos_weight,
                        int N, int K, int from_logits, float* dx, float* ring, int* counter, int cap, float* loss_out,
                        void* stream) {
  if (!bce_args_ok(x, ldx, y, ldy, N, K, from_logits, dx, ring, counter, cap, loss_out)) return SF_EINVAL;
  if (pos_weight && !from_logits) return SF_EINVAL;  // torch's BCELoss has no pos_weight
  hipLaunchKernelGGL(bce_w_kernel, dim3(1), dim3(CE_TPB), 0, (hipStream_t)stream, x, ldx, y, ldy, weight, pos_weight, N,
                     K, from_logits, dx, ring, counter, cap, loss_out);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_adam_step(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                            const long* chunks, int n_chunks, const double* hyper_host, const double* hyper,
                            int n_groups, const float* guard, int zero_grad, void* stream) {
  return adam_entry<false>(table_host, table, n_tensors, chunks_host, chunks, n_chunks, hyper_host, hyper, n_groups,
                           guard, zero_grad, stream);
}

extern "C" int sf_adamw_step(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                             const long* chunks, int n_chunks, const double* hyper_host, const double* hyper,
                             int n_groups, const float* guard, int zero_grad, void* stream) {
  return adam_entry<true>(table_host, table, n_tensors, chunks_host, chunks, n_chunks, hyper_host, hyper, n_groups,
                          guard, zero_grad, stream);
}
