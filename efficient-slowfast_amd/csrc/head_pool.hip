// head_pool.hip — the fully-convolutional classification head's average pool (ResNetBasicHead, reference
// head_helper.py:174-179 builds nn.AvgPool3d(pool_size, stride=1); :203-207 applies it per pathway and concatenates):
//   out[n, to, ho, wo, c] = 1/|k| * sum over the (kT, kH, kW) window of x        sf_avgpool_win_fwd
//   dx[n, t, h, w, c]    (+)= 1/|k| * sum of dy over the windows that hold (t,h,w)  sf_avgpool_win_bwd
// Stride 1, no padding, To = T - kT + 1 (H, W likewise).  With the driver-monitoring YAMLs' spatial strides res5 is
// crop/16 wide under a crop//32 window, so To x Ho x Wo = 1 x 5 x 5 at crop 112 (1 x 3 x 3 at crop 64) instead of 1.
//
// Forward: one workgroup per (n, to, block of channels).  It sums the window's kT frames into an [H*W][channels] plane
// in LDS — the only pass over x — and box-filters that plane into the pathway's channel slice of the concat buffer.
// Backward: a gather, one thread per (n, h, w, 4 channels); when To == 1 the sum over the windows does not depend on
// t, so it is formed once and stored to all T frames.  Both add in a fixed order and own their outputs: no atomics,
// bitwise reproducible.  Element indices are 64-bit.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int PLANE_FLOATS = 8192;  // 32 KB of LDS per workgroup
constexpr int MIN_BLOCK_C = 32;     // channel blocks are not cut below 128 contiguous bytes per position
constexpr long WANT_WGS = 1024;     // four workgroups per CU before the channel blocks stop shrinking

template <int V>
struct Vec;
template <>
struct Vec<4> { typedef f32x4 type; };
template <>
struct Vec<1> { typedef float type; };

// grid: N * To * nblk workgroups.  bc: channels per block (a multiple of V, H * W * bc <= PLANE_FLOATS).
template <int V>
__global__ __launch_bounds__(TPB) void avgpool_win_fwd_kernel(const sf_pool_desc d, const float* __restrict__ x,
                                                              float* __restrict__ out, int bc, int nblk, float inv) {
  typedef typename Vec<V>::type vec;
  __shared__ __attribute__((aligned(16))) float plane[PLANE_FLOATS];
  const int blk = blockIdx.x % nblk;
  const long nt = blockIdx.x / nblk;  // n * To + to
  const int to = (int)(nt % d.To);
  const long n = nt / d.To;
  const int c0 = blk * bc;
  const int cc = min(bc, d.C - c0);  // this block's channels (a multiple of V)
  const int cv = cc / V;
  const int HW = d.Hi * d.Wi;
  const long fstep = (long)HW * d.in_cs;  // one frame of x
  const float* xb = x + (n * d.Ti + to) * fstep + d.in_coff + c0;
  for (int i = threadIdx.x; i < HW * cv; i += TPB) {
    const int pos = i / cv, c = (i - pos * cv) * V;
    const float* s = xb + (long)pos * d.in_cs + c;
    vec acc = *reinterpret_cast<const vec*>(s);
    for (int kt = 1; kt < d.kT; ++kt) acc += *reinterpret_cast<const vec*>(s + kt * fstep);
    *reinterpret_cast<vec*>(plane + pos * cc + c) = acc;
  }
  __syncthreads();
  const int OHW = d.Ho * d.Wo;
  float* ob = out + nt * OHW * d.out_cs + d.out_coff + c0;
  for (int i = threadIdx.x; i < OHW * cv; i += TPB) {
    const int pos = i / cv, c = (i - pos * cv) * V;
    const int ho = pos / d.Wo, wo = pos - ho * d.Wo;
    const float* p = plane + (ho * d.Wi + wo) * cc + c;
    vec acc = *reinterpret_cast<const vec*>(p);
    for (int kh = 0; kh < d.kH; ++kh)
      for (int kw = (kh == 0 ? 1 : 0); kw < d.kW; ++kw) acc += *reinterpret_cast<const vec*>(p + (kh * d.Wi + kw) * cc);
    *reinterpret_cast<vec*>(ob + (long)pos * d.out_cs + c) = acc * inv;
  }
}

// total = N * TT * H * W * (C / V) threads, TT = 1 when the frames share one sum (To == 1: `frames` = T stores per
// thread), else TT = T and frames = 1.
template <int V>
__global__ __launch_bounds__(TPB) void avgpool_win_bwd_kernel(const sf_pool_desc d, const float* __restrict__ dy,
                                                              int dy_cs, int dy_coff, float* __restrict__ dx,
                                                              int dx_cs, int dx_coff, int TT, int frames, float inv,
                                                              int overwrite, long total) {
  typedef typename Vec<V>::type vec;
  const long idx = (long)blockIdx.x * TPB + threadIdx.x;
  if (idx >= total) return;
  const int cv = d.C / V;
  const int c = (int)(idx % cv) * V;
  long r = idx / cv;
  const int w = (int)(r % d.Wi);
  r /= d.Wi;
  const int h = (int)(r % d.Hi);
  r /= d.Hi;
  const int t = (int)(r % TT);
  const long n = r / TT;
  const int to0 = max(0, t - d.kT + 1), to1 = min(d.To - 1, t);
  const int ho0 = max(0, h - d.kH + 1), ho1 = min(d.Ho - 1, h);
  const int wo0 = max(0, w - d.kW + 1), wo1 = min(d.Wo - 1, w);
  vec acc = (vec)0.f;
  for (int to = to0; to <= to1; ++to)
    for (int ho = ho0; ho <= ho1; ++ho)
      for (int wo = wo0; wo <= wo1; ++wo)
        acc += *reinterpret_cast<const vec*>(dy + (((n * d.To + to) * d.Ho + ho) * d.Wo + wo) * dy_cs + dy_coff + c);
  acc *= inv;
  const long fstep = (long)d.Hi * d.Wi * dx_cs;
  float* o = dx + (((n * d.Ti + t) * d.Hi + h) * d.Wi + w) * dx_cs + dx_coff + c;
  if (overwrite) {
    for (int f = 0; f < frames; ++f) *reinterpret_cast<vec*>(o + f * fstep) = acc;
  } else {
    for (int f = 0; f < frames; ++f) *reinterpret_cast<vec*>(o + f * fstep) += acc;
  }
}

// stride 1, no padding, an averaging window no larger than the input, output extents that follow from it
bool win_desc_ok(const sf_pool_desc* d) {
  if (!d || d->N <= 0 || d->Ti <= 0 || d->Hi <= 0 || d->Wi <= 0 || d->C <= 0) return false;
  if (d->kT <= 0 || d->kH <= 0 || d->kW <= 0 || d->kT > d->Ti || d->kH > d->Hi || d->kW > d->Wi) return false;
  if (d->sT != 1 || d->sH != 1 || d->sW != 1 || d->pT != 0 || d->pH != 0 || d->pW != 0 || !d->is_avg) return false;
  return d->To == d->Ti - d->kT + 1 && d->Ho == d->Hi - d->kH + 1 && d->Wo == d->Wi - d->kW + 1;
}

bool slice_ok(int cs, int coff, int C) { return coff >= 0 && C <= cs && coff <= cs - C; }

}  // namespace

extern "C" int sf_avgpool_win_fwd(const sf_pool_desc* d, const float* x, float* out, void* stream) {
  if (!win_desc_ok(d) || !x || !out) return SF_EINVAL;
  if (!slice_ok(d->in_cs, d->in_coff, d->C) || !slice_ok(d->out_cs, d->out_coff, d->C)) return SF_EINVAL;
  const bool vec4 = d->C % 4 == 0 && d->in_cs % 4 == 0 && d->in_coff % 4 == 0 && d->out_cs % 4 == 0 &&
                    d->out_coff % 4 == 0 && sf_aligned16(x) && sf_aligned16(out);
  const int V = vec4 ? 4 : 1;
  const long HW = (long)d->Hi * d->Wi;
  // a plane that leaves no room for one vector of channels per position (H * W > 2048 with float4): the generic kernel
  if (HW * V > PLANE_FLOATS) return sf_pool_fwd(d, x, out, stream);
  const long nt = (long)d->N * d->To;
  int bc = (int)(PLANE_FLOATS / HW) / V * V;
  if (bc > d->C) bc = d->C;
  while (bc > MIN_BLOCK_C && nt * ((d->C + bc - 1) / bc) < WANT_WGS) bc = ((bc + 1) / 2 + V - 1) / V * V;
  const int nblk = (d->C + bc - 1) / bc;
  if (nt * nblk > 0xffffffffL / TPB) return SF_EINVAL;  // grid x block stays below 2^32 threads
  const float inv = 1.f / (float)(d->kT * d->kH * d->kW);
  const dim3 grid((unsigned)(nt * nblk));
  if (vec4) {
    hipLaunchKernelGGL(avgpool_win_fwd_kernel<4>, grid, dim3(TPB), 0, (hipStream_t)stream, *d, x, out, bc, nblk, inv);
  } else {
    hipLaunchKernelGGL(avgpool_win_fwd_kernel<1>, grid, dim3(TPB), 0, (hipStream_t)stream, *d, x, out, bc, nblk, inv);
  }
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_avgpool_win_bwd(const sf_pool_desc* d, const float* dy, int dy_cs, int dy_coff, float* dx, int dx_cs,
                                  int dx_coff, int overwrite, void* stream) {
  if (!win_desc_ok(d) || !dy || !dx) return SF_EINVAL;
  if (!slice_ok(dy_cs, dy_coff, d->C) || !slice_ok(dx_cs, dx_coff, d->C)) return SF_EINVAL;
  const bool vec4 = d->C % 4 == 0 && dy_cs % 4 == 0 && dy_coff % 4 == 0 && dx_cs % 4 == 0 && dx_coff % 4 == 0 &&
                    sf_aligned16(dy) && sf_aligned16(dx);
  const int TT = d->To == 1 ? 1 : d->Ti, frames = d->To == 1 ? d->Ti : 1;
  const long total = (long)d->N * TT * d->Hi * d->Wi * (d->C / (vec4 ? 4 : 1));
  if ((total + TPB - 1) / TPB > 0xffffffffL / TPB) return SF_EINVAL;  // grid x block stays below 2^32 threads
  const float inv = 1.f / (float)(d->kT * d->kH * d->kW);
  const dim3 grid((unsigned)((total + TPB - 1) / TPB));
  if (vec4) {
    hipLaunchKernelGGL(avgpool_win_bwd_kernel<4>, grid, dim3(TPB), 0, (hipStream_t)stream, *d, dy, dy_cs, dy_coff, dx,
                       dx_cs, dx_coff, TT, frames, inv, overwrite, total);
  } else {
    hipLaunchKernelGGL(avgpool_win_bwd_kernel<1>, grid, dim3(TPB), 0, (hipStream_t)stream, *d, dy, dy_cs, dy_coff, dx,
                       dx_cs, dx_coff, TT, frames, inv, overwrite, total);
  }
  SF_CHECK_LAUNCH();
  return SF_OK;
}
