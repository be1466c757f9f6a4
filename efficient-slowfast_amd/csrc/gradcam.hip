// gradcam.hip — the kernels behind slowfast/models/gradcam.py (reference wdf_visualization/gradcam_video.py):
//   sf_epilogue_bwd       backward of a conv's folded eval epilogue  y = relu?(scale[c] * z + bias[c] + res), with the
//                         nearest T-repeat of the CMDA Slow->Fast edge (custom_video_model_builder.py:120-121) as `rep`
//   sf_epilogue_bwd_act   the same with an activation code (ReLU6: mobilenetv2_helper.py:30-68) and the inverse of the
//                         channel-shuffled store of a grouped conv (shufflenet_helper.py:22-79)
//   sf_dwconv_dgrad_epi   data gradient of a depthwise conv with its folded epilogue's backward applied while dy is
//                         loaded: no dL/dz tensor is written or read (MobileNetV2's 6x-expanded depthwise, ShuffleNet's conv2)
//   sf_head_act_mean_bwd  backward of the head's eval tail  out[b,k] = mean_p act(logits[b,p,:])[k]  (head_helper.py:217-221)
//   sf_cam_weights        w[n,t,c] = mean_{h,w} G[n,t,h,w,c]                                   (gradcam_video.py:159-166)
//   sf_cam_map            cam[n,t,h,w] = max(0, 1 + sum_c w[n,t,c] * mean_t' A[n,t',h,w,c]), then (cam - min) / (max - min)
//                         per frame (gradcam_video.py:167-179); a frame whose range is zero gives zeros
// Every output element has one owner and every sum a fixed order: no atomics, bitwise reproducible.  Element indices
// are 64-bit.  All are HBM / latency bound passes; none keeps state between launches.
#include "common.h"

namespace {

constexpr int TPB = 256;

template <int V>
struct Vec;
template <>
struct Vec<4> { typedef f32x4 type; };
template <>
struct Vec<1> { typedef float type; };

template <int V>
__device__ __forceinline__ float lane(const typename Vec<V>::type& v, int e);
template <>
__device__ __forceinline__ float lane<4>(const f32x4& v, int e) { return v[e]; }
template <>
__device__ __forceinline__ float lane<1>(const float& v, int) { return v; }
template <int V>
__device__ __forceinline__ void set_lane(typename Vec<V>::type& v, int e, float x);
template <>
__device__ __forceinline__ void set_lane<4>(f32x4& v, int e, float x) { v[e] = x; }
template <>
__device__ __forceinline__ void set_lane<1>(float& v, int, float x) { v = x; }

struct EpiArgs {
  const float* dy; int dy_cs, dy_coff;
  const float* y; int y_cs, y_coff;
  int T, HW, C, rep;         // T = frames of dz (dy / y hold T * rep)
  const float* scale; int act;   // SF_ACT_NONE | SF_ACT_RELU | SF_ACT_RELU6
  int groups;                // > 1: dz channel g * (C / groups) + j reads dy / y at channel j * groups + g
  float* dz; int dz_cs, dz_coff, dz_acc;
  float* dres; int dres_cs, dres_coff, dres_acc;
  long total;                // N * T * HW * (C / V) threads
};

// the activation's gradient mask, taken from its OUTPUT (as sf_act_bwd): 0 < y, and y < 6 for ReLU6
__device__ __forceinline__ bool act_passes(float y, int act) { return y > 0.f && (act != SF_ACT_RELU6 || y < 6.f); }

// one thread per (n, t, hw, V channels) of dz: reads its rep elements of dy (and y) once, in frame order
template <int V>
__global__ __launch_bounds__(TPB) void epilogue_bwd_kernel(const EpiArgs a) {
  typedef typename Vec<V>::type vec;
  const long idx = (long)blockIdx.x * TPB + threadIdx.x;
  if (idx >= a.total) return;
  const int cv = a.C / V;
  const int c = (int)(idx % cv) * V;
  long r = idx / cv;
  const int hw = (int)(r % a.HW);
  r /= a.HW;
  const int t = (int)(r % a.T);
  const long n = r / a.T;
  const long row0 = ((n * a.T + t) * a.rep) * a.HW + hw;  // row of (n, t * rep, hw) in dy / y
  vec acc = (vec)0.f;
  for (int q = 0; q < a.rep; ++q) {
    const long row = row0 + (long)q * a.HW;
    vec g = *reinterpret_cast<const vec*>(a.dy + row * a.dy_cs + a.dy_coff + c);
    if (a.act != SF_ACT_NONE) {
      const vec yy = *reinterpret_cast<const vec*>(a.y + row * a.y_cs + a.y_coff + c);
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (!act_passes(lane<V>(yy, e), a.act)) set_lane<V>(g, e, 0.f);
    }
    if (q == 0) {
      acc = g;
      if (a.dres) {  // rep == 1 (checked by the launcher): dres row == dz row
        float* o = a.dres + row * a.dres_cs + a.dres_coff + c;
        if (a.dres_acc) *reinterpret_cast<vec*>(o) += g;
        else *reinterpret_cast<vec*>(o) = g;
      }
    } else {
      acc += g;
    }
  }
  if (a.scale) acc *= *reinterpret_cast<const vec*>(a.scale + c);
  float* o = a.dz + (((n * a.T + t) * (long)a.HW) + hw) * a.dz_cs + a.dz_coff + c;
  if (a.dz_acc) *reinterpret_cast<vec*>(o) += acc;
  else *reinterpret_cast<vec*>(o) = acc;
}

// groups > 1 (rep == 1, no dres: checked by the launcher): one thread per (row, V CONTIGUOUS dz channels), which gathers
// its dy / y elements at stride `groups` — the inverse of the shuffled store of sf_conv_fwd_grouped(shuffle = 1).  The
// threads of a row together read the row's C floats of dy (and y) exactly once.
template <int V>
__global__ __launch_bounds__(TPB) void epilogue_bwd_shuffled_kernel(const EpiArgs a) {
  typedef typename Vec<V>::type vec;
  const long idx = (long)blockIdx.x * TPB + threadIdx.x;
  if (idx >= a.total) return;
  const int cv = a.C / V;
  const int c = (int)(idx % cv) * V;
  const long row = idx / cv;
  const int cg = a.C / a.groups;
  const float* dyr = a.dy + row * a.dy_cs + a.dy_coff;
  const float* yr = a.act != SF_ACT_NONE ? a.y + row * a.y_cs + a.y_coff : nullptr;
  vec acc = (vec)0.f;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const int cz = c + e;
    const int g = cz / cg, j = cz - g * cg;
    const int src = j * a.groups + g;
    float v = dyr[src];
    if (yr && !act_passes(yr[src], a.act)) v = 0.f;
    set_lane<V>(acc, e, v);
  }
  if (a.scale) acc *= *reinterpret_cast<const vec*>(a.scale + c);
  float* o = a.dz + row * a.dz_cs + a.dz_coff + c;
  if (a.dz_acc) *reinterpret_cast<vec*>(o) += acc;
  else *reinterpret_cast<vec*>(o) = acc;
}

struct DwEpiArgs {
  sf_conv_desc d;            // Ti/Hi/Wi: dx's dims, To/Ho/Wo: dy's dims, cin_pad: the packed weight's pitch
  const float* dy; int dy_cs, dy_coff;
  const float* y; int y_cs, y_coff;
  const float* w; const float* scale; int act;
  float* dx; int dx_cs, dx_coff;
  int C, accumulate;
};

// dx[n,ti,hi,wi,c] (=|+=) scale[c] * sum_taps w[tap][c] * dy[pos] * m(y[pos]): the transposed gather of
// dwconv_dgrad_vec4_kernel (backward.hip) with the epilogue's mask applied to dy as it is loaded.  One thread per
// (dx position, V channels), taps in (kt, kh, kw) order.  I: the position arithmetic's integer type (32-bit where the
// thread count fits, 64-bit otherwise); element offsets are 64-bit either way.
template <int V, typename I>
__global__ __launch_bounds__(TPB) void dwconv_dgrad_epi_kernel(const DwEpiArgs a, I total) {
  typedef typename Vec<V>::type vec;
  const I idx = (I)blockIdx.x * TPB + threadIdx.x;
  if (idx >= total) return;
  const sf_conv_desc& d = a.d;
  const I cv = (I)(a.C / V);
  const I rin = idx / cv;
  const int c = (int)(idx - rin * cv) * V;
  const I q1 = rin / (I)d.Wi;
  const int wi = (int)(rin - q1 * (I)d.Wi);
  const I q2 = q1 / (I)d.Hi;
  const int hi = (int)(q1 - q2 * (I)d.Hi);
  const I n = q2 / (I)d.Ti;
  const int ti = (int)(q2 - n * (I)d.Ti);
  vec acc = (vec)0.f;
  int tap = 0;
  for (int kt = 0; kt < d.kT; ++kt) {
    const int nt = ti + d.pT - kt * d.dT;
    for (int kh = 0; kh < d.kH; ++kh) {
      const int nh = hi + d.pH - kh * d.dH;
      for (int kw = 0; kw < d.kW; ++kw, ++tap) {
        const int nw = wi + d.pW - kw * d.dW;
        if (nt < 0 || nh < 0 || nw < 0 || (nt % d.sT) || (nh % d.sH) || (nw % d.sW)) continue;
        const int to = nt / d.sT, ho = nh / d.sH, wo = nw / d.sW;
        if (to >= d.To || ho >= d.Ho || wo >= d.Wo) continue;
        const long ro = (((long)n * d.To + to) * d.Ho + ho) * d.Wo + wo;
        vec g = *reinterpret_cast<const vec*>(a.dy + ro * a.dy_cs + a.dy_coff + c);
        if (a.act != SF_ACT_NONE) {
          const vec yy = *reinterpret_cast<const vec*>(a.y + ro * a.y_cs + a.y_coff + c);
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (!act_passes(lane<V>(yy, e), a.act)) set_lane<V>(g, e, 0.f);
        }
        acc += g * *reinterpret_cast<const vec*>(a.w + (long)tap * d.cin_pad + c);
      }
    }
  }
  if (a.scale) acc *= *reinterpret_cast<const vec*>(a.scale + c);
  float* o = a.dx + (long)rin * a.dx_cs + a.dx_coff + c;
  if (a.accumulate) *reinterpret_cast<vec*>(o) += acc;
  else *reinterpret_cast<vec*>(o) = acc;
}

// fixed-order tree over the workgroup's TPB values; every thread gets the result
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const float o = red[threadIdx.x + s];
      red[threadIdx.x] = MAX ? fmaxf(red[threadIdx.x], o) : red[threadIdx.x] + o;
    }
    __syncthreads();
  }
  const float out = red[0];
  __syncthreads();
  return out;
}

// one workgroup per (b, p) row of the logits
__global__ __launch_bounds__(TPB) void head_act_mean_bwd_kernel(const float* __restrict__ logits,
                                                                const float* __restrict__ dout, int P, int K, int act,
                                                                float* __restrict__ dl, int accumulate) {
  __shared__ float red[TPB];
  const long row = blockIdx.x;
  const long b = row / P;
  const float* l = logits + row * K;
  const float* g = dout + b * K;
  float* o = dl + row * K;
  const float invP = 1.f / (float)P;
  float mx = 0.f, sum = 1.f, dot = 0.f;
  if (act == SF_ACT_SOFTMAX) {
    float m = -3.0e38f;
    for (int k = threadIdx.x; k < K; k += TPB) m = fmaxf(m, l[k]);
    mx = block_reduce<true>(m, red);
    float part = 0.f, pd = 0.f;
    for (int k = threadIdx.x; k < K; k += TPB) {
      const float e = expf(l[k] - mx);
      part += e;
      pd = fmaf(g[k], e, pd);
    }
    sum = block_reduce<false>(part, red);
    dot = block_reduce<false>(pd, red) / sum;  // sum_j dout[j] * s[j]
  }
  for (int k = threadIdx.x; k < K; k += TPB) {
    const float v = l[k];
    float d;
    if (act == SF_ACT_SOFTMAX) {
      d = expf(v - mx) / sum * (g[k] - dot);
    } else if (act == SF_ACT_SIGMOID) {
      const float s = 1.f / (1.f + expf(-v));
      d = s * (1.f - s) * g[k];
    } else if (act == SF_ACT_RELU) {
      d = v > 0.f ? g[k] : 0.f;
    } else {
      d = g[k];
    }
    d *= invP;
    o[k] = accumulate ? o[k] + d : d;
  }
}

// grid (N * T, channel blocks of cbw): thread = (position lane, channel); partial sums over the lane's positions in
// position order, then the lanes' partials in lane order
__global__ __launch_bounds__(TPB) void cam_weights_kernel(const float* __restrict__ g, int cs, int coff, int HW, int C,
                                                          int cbw, float* __restrict__ w) {
  __shared__ float red[TPB];
  const int lanes = TPB / cbw;
  const int ci = threadIdx.x % cbw, pl = threadIdx.x / cbw;
  const int c = blockIdx.y * cbw + ci;
  const long nt = blockIdx.x;
  float acc = 0.f;
  if (c < C) {
    const float* src = g + nt * HW * cs + coff + c;
    for (int p = pl; p < HW; p += lanes) acc += src[(long)p * cs];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (pl == 0 && c < C) {
    float s = red[ci];
    for (int q = 1; q < lanes; ++q) s += red[q * cbw + ci];
    w[nt * C + c] = s / (float)HW;
  }
}

// abar[n, hw, c] = (sum_t A[n, t, hw, c]) / T, frames in order
__global__ __launch_bounds__(TPB) void cam_abar_kernel(const float* __restrict__ a, int cs, int coff, int T, int HW,
                                                       int C, float* __restrict__ abar, long total) {
  const long idx = (long)blockIdx.x * TPB + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  long r = idx / C;
  const int hw = (int)(r % HW);
  const long n = r / HW;
  const float* src = a + ((n * T) * HW + hw) * cs + coff + c;
  float acc = src[0];
  for (int t = 1; t < T; ++t) acc += src[(long)t * HW * cs];
  abar[idx] = acc / (float)T;
}

// one workgroup per (n, t) frame: map (channels in order, fused multiply-adds), frame min / max, normalise.  The
// normalisation is invariant under the map's constant: max(0, 1 + s) - 1 = max(-1, s), so it is taken of u = max(-1, s)
// with s summed from 0 — where the maps are nearly flat (s of order 1e-3: deep targets), rounding 1 + s to fp32 first
// would cost the normalised map 2^-24 / range.  `raw` is the map itself, summed onto the 1.  A thread re-reads only the
// positions it wrote itself.
__global__ __launch_bounds__(TPB) void cam_map_kernel(const float* __restrict__ abar, const float* __restrict__ w, int T,
                                                      int HW, int C, float* __restrict__ raw, float* __restrict__ cam) {
  __shared__ float red[TPB];
  const long nt = blockIdx.x;
  const long n = nt / T;
  const float* wv = w + nt * C;
  const float* ab = abar + n * HW * C;
  float* o = cam + nt * HW;
  float lo = 3.0e38f, hi = -1.f;  // u >= -1
  for (int p = threadIdx.x; p < HW; p += TPB) {
    const float* ap = ab + (long)p * C;
    float one = 1.f, u = 0.f;
    for (int c = 0; c < C; ++c) {
      one = fmaf(wv[c], ap[c], one);
      u = fmaf(wv[c], ap[c], u);
    }
    u = fmaxf(u, -1.f);
    o[p] = u;
    if (raw) raw[nt * HW + p] = fmaxf(one, 0.f);
    lo = fminf(lo, u);
    hi = fmaxf(hi, u);
  }
  hi = block_reduce<true>(hi, red);
  lo = -block_reduce<true>(-lo, red);
  const float range = hi - lo;
  for (int p = threadIdx.x; p < HW; p += TPB) o[p] = range > 0.f ? (o[p] - lo) / range : 0.f;
}

bool slice_ok(int cs, int coff, int C) { return coff >= 0 && C <= cs && coff <= cs - C; }
bool grid_ok(long blocks) { return blocks > 0 && blocks <= 0xffffffffL / TPB; }  // grid x block stays below 2^32 threads

}  // namespace

static int epilogue_bwd_impl(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff, int N, int T,
                             int H, int W, int C, int rep, const float* scale, int act, int groups, float* dz, int dz_cs,
                             int dz_coff, int dz_accumulate, float* dres, int dres_cs, int dres_coff,
                             int dres_accumulate, void* stream) {
  if (!dy || !dz || N <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || rep <= 0 || groups <= 0) return SF_EINVAL;
  if (act != SF_ACT_NONE && act != SF_ACT_RELU && act != SF_ACT_RELU6) return SF_EINVAL;
  const bool masked = act != SF_ACT_NONE;
  if (masked && !y) return SF_EINVAL;
  if (dres && rep != 1) return SF_EINVAL;
  if (groups > 1 && (rep != 1 || dres || C % groups != 0)) return SF_EINVAL;
  if (!slice_ok(dy_cs, dy_coff, C) || !slice_ok(dz_cs, dz_coff, C)) return SF_EINVAL;
  if (masked && !slice_ok(y_cs, y_coff, C)) return SF_EINVAL;
  if (dres && !slice_ok(dres_cs, dres_coff, C)) return SF_EINVAL;
  bool vec4 = C % 4 == 0 && dy_cs % 4 == 0 && dy_coff % 4 == 0 && dz_cs % 4 == 0 && dz_coff % 4 == 0 &&
              sf_aligned16(dy) && sf_aligned16(dz) && (!scale || sf_aligned16(scale));
  if (masked) vec4 = vec4 && y_cs % 4 == 0 && y_coff % 4 == 0 && sf_aligned16(y);
  if (dres) vec4 = vec4 && dres_cs % 4 == 0 && dres_coff % 4 == 0 && sf_aligned16(dres);
  EpiArgs a;
  a.dy = dy; a.dy_cs = dy_cs; a.dy_coff = dy_coff;
  a.y = masked ? y : nullptr; a.y_cs = y_cs; a.y_coff = y_coff;
  a.T = T; a.HW = H * W; a.C = C; a.rep = rep;
  a.scale = scale; a.act = act; a.groups = groups;
  a.dz = dz; a.dz_cs = dz_cs; a.dz_coff = dz_coff; a.dz_acc = dz_accumulate ? 1 : 0;
  a.dres = dres; a.dres_cs = dres_cs; a.dres_coff = dres_coff; a.dres_acc = dres_accumulate ? 1 : 0;
  if ((long)H * W > 0x7fffffffL) return SF_EINVAL;
  a.total = (long)N * T * H * W * (C / (vec4 ? 4 : 1));
  const long blocks = (a.total + TPB - 1) / TPB;
  if (!grid_ok(blocks)) return SF_EINVAL;
  if (groups > 1) {
    if (vec4) {
      hipLaunchKernelGGL(epilogue_bwd_shuffled_kernel<4>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, a);
    } else {
      hipLaunchKernelGGL(epilogue_bwd_shuffled_kernel<1>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, a);
    }
  } else if (vec4) {
    hipLaunchKernelGGL(epilogue_bwd_kernel<4>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(epilogue_bwd_kernel<1>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, a);
  }
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_epilogue_bwd(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff, int N,
                               int T, int H, int W, int C, int rep, const float* scale, int relu, float* dz, int dz_cs,
                               int dz_coff, int dz_accumulate, float* dres, int dres_cs, int dres_coff,
                               int dres_accumulate, void* stream) {
  return epilogue_bwd_impl(dy, dy_cs, dy_coff, y, y_cs, y_coff, N, T, H, W, C, rep, scale,
                           relu ? SF_ACT_RELU : SF_ACT_NONE, 1, dz, dz_cs, dz_coff, dz_accumulate, dres, dres_cs,
                           dres_coff, dres_accumulate, stream);
}

extern "C" int sf_epilogue_bwd_act(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff, int N,
                                   int T, int H, int W, int C, int rep, const float* scale, int act, int groups,
                                   float* dz, int dz_cs, int dz_coff, int dz_accumulate, float* dres, int dres_cs,
                                   int dres_coff, int dres_accumulate, void* stream) {
  return epilogue_bwd_impl(dy, dy_cs, dy_coff, y, y_cs, y_coff, N, T, H, W, C, rep, scale, act, groups, dz, dz_cs,
                           dz_coff, dz_accumulate, dres, dres_cs, dres_coff, dres_accumulate, stream);
}

static int dw_out_dim(int i, int k, int s, int p, int dl) { return (i + 2 * p - dl * (k - 1) - 1) / s + 1; }

extern "C" int sf_dwconv_dgrad_epi(const sf_conv_desc* d, const float* dy, int dy_cs, int dy_coff, const float* y,
                                   int y_cs, int y_coff, const float* w_packed, const float* scale, int act, float* dx,
                                   int dx_cs, int dx_coff, int C, int accumulate, void* stream) {
  if (!d || !dy || !w_packed || !dx || C <= 0) return SF_EINVAL;
  if (act != SF_ACT_NONE && act != SF_ACT_RELU && act != SF_ACT_RELU6) return SF_EINVAL;
  const bool masked = act != SF_ACT_NONE;
  if (masked && !y) return SF_EINVAL;
  if (d->N <= 0 || d->Ti <= 0 || d->Hi <= 0 || d->Wi <= 0 || d->To <= 0 || d->Ho <= 0 || d->Wo <= 0) return SF_EINVAL;
  if (d->kT <= 0 || d->kH <= 0 || d->kW <= 0 || d->sT <= 0 || d->sH <= 0 || d->sW <= 0 || d->pT < 0 || d->pH < 0 ||
      d->pW < 0 || d->dT <= 0 || d->dH <= 0 || d->dW <= 0 || d->cin_pad < C)
    return SF_EINVAL;
  // dy's dims are the forward conv's output dims: every row the gather can reach lies inside dy and y
  if ((long)d->Ti + 2 * d->pT < (long)d->dT * (d->kT - 1) + 1 || (long)d->Hi + 2 * d->pH < (long)d->dH * (d->kH - 1) + 1 ||
      (long)d->Wi + 2 * d->pW < (long)d->dW * (d->kW - 1) + 1)
    return SF_EINVAL;
  if (d->To != dw_out_dim(d->Ti, d->kT, d->sT, d->pT, d->dT) || d->Ho != dw_out_dim(d->Hi, d->kH, d->sH, d->pH, d->dH) ||
      d->Wo != dw_out_dim(d->Wi, d->kW, d->sW, d->pW, d->dW))
    return SF_EINVAL;
  if (!slice_ok(dy_cs, dy_coff, C) || !slice_ok(dx_cs, dx_coff, C)) return SF_EINVAL;
  if (masked && !slice_ok(y_cs, y_coff, C)) return SF_EINVAL;
  bool vec4 = C % 4 == 0 && dy_cs % 4 == 0 && dy_coff % 4 == 0 && dx_cs % 4 == 0 && dx_coff % 4 == 0 &&
              d->cin_pad % 4 == 0 && sf_aligned16(dy) && sf_aligned16(dx) && sf_aligned16(w_packed) &&
              (!scale || sf_aligned16(scale));
  if (masked) vec4 = vec4 && y_cs % 4 == 0 && y_coff % 4 == 0 && sf_aligned16(y);
  DwEpiArgs a;
  a.d = *d;
  a.dy = dy; a.dy_cs = dy_cs; a.dy_coff = dy_coff;
  a.y = masked ? y : nullptr; a.y_cs = y_cs; a.y_coff = y_coff;
  a.w = w_packed; a.scale = scale; a.act = act;
  a.dx = dx; a.dx_cs = dx_cs; a.dx_coff = dx_coff;
  a.C = C; a.accumulate = accumulate ? 1 : 0;
  const long total = (long)d->N * d->Ti * d->Hi * d->Wi * (C / (vec4 ? 4 : 1));
  const long blocks = (total + TPB - 1) / TPB;
  if (!grid_ok(blocks)) return SF_EINVAL;
  const bool small = total <= 0x7fffffffL - TPB;  // the thread index fits 32 bits: 32-bit position arithmetic
  hipStream_t s = (hipStream_t)stream;
  if (vec4 && small) {
    hipLaunchKernelGGL((dwconv_dgrad_epi_kernel<4, unsigned>), dim3((unsigned)blocks), dim3(TPB), 0, s, a, (unsigned)total);
  } else if (vec4) {
    hipLaunchKernelGGL((dwconv_dgrad_epi_kernel<4, long>), dim3((unsigned)blocks), dim3(TPB), 0, s, a, total);
  } else if (small) {
    hipLaunchKernelGGL((dwconv_dgrad_epi_kernel<1, unsigned>), dim3((unsigned)blocks), dim3(TPB), 0, s, a, (unsigned)total);
  } else {
    hipLaunchKernelGGL((dwconv_dgrad_epi_kernel<1, long>), dim3((unsigned)blocks), dim3(TPB), 0, s, a, total);
  }
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_head_act_mean_bwd(const float* logits, const float* dout, int B, int P, int K, int act, float* dl,
                                    int accumulate, void* stream) {
  if (!logits || !dout || !dl || B <= 0 || P <= 0 || K <= 0) return SF_EINVAL;
  if (act != SF_ACT_NONE && act != SF_ACT_RELU && act != SF_ACT_SIGMOID && act != SF_ACT_SOFTMAX) return SF_EINVAL;
  const long rows = (long)B * P;
  if (!grid_ok(rows)) return SF_EINVAL;
  hipLaunchKernelGGL(head_act_mean_bwd_kernel, dim3((unsigned)rows), dim3(TPB), 0, (hipStream_t)stream, logits, dout,
                     P, K, act, dl, accumulate ? 1 : 0);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_cam_weights(const float* g, int g_cs, int g_coff, int N, int T, int H, int W, int C, float* w,
                              void* stream) {
  if (!g || !w || N <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0) return SF_EINVAL;
  if (!slice_ok(g_cs, g_coff, C) || (long)H * W > 0x7fffffffL) return SF_EINVAL;
  const int cbw = C <= 8 ? 8 : C <= 16 ? 16 : C <= 32 ? 32 : 64;
  const long frames = (long)N * T;
  const int cblocks = (C + cbw - 1) / cbw;
  if (!grid_ok(frames) || cblocks > 65535) return SF_EINVAL;
  hipLaunchKernelGGL(cam_weights_kernel, dim3((unsigned)frames, (unsigned)cblocks), dim3(TPB), 0, (hipStream_t)stream,
                     g, g_cs, g_coff, H * W, C, cbw, w);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" long sf_cam_map_ws_floats(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  return (long)N * H * W * C;
}

extern "C" int sf_cam_map(const float* a, int a_cs, int a_coff, const float* w, int N, int T, int H, int W, int C,
                          float* ws, float* raw, float* cam, void* stream) {
  if (!a || !w || !ws || !cam || N <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0) return SF_EINVAL;
  if (!slice_ok(a_cs, a_coff, C) || (long)H * W > 0x7fffffffL) return SF_EINVAL;
  const long total = (long)N * H * W * C;
  const long blocks = (total + TPB - 1) / TPB;
  const long frames = (long)N * T;
  if (!grid_ok(blocks) || !grid_ok(frames)) return SF_EINVAL;
  hipLaunchKernelGGL(cam_abar_kernel, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, a, a_cs, a_coff, T,
                     H * W, C, ws, total);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(cam_map_kernel, dim3((unsigned)frames), dim3(TPB), 0, (hipStream_t)stream, ws, w, T, H * W, C, raw,
                     cam);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
