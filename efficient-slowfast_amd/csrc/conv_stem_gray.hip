// conv_stem_gray.hip — the stem convolution of a ONE-channel (grayscale) clip: forward, weight gradient, layout (gfx950).
//
// Reference: stem_helper.py:157-164 (nn.Conv3d(1, Cout, [kT,7,7], stride [1,2,2], padding [kT//2,3,3]) of
// ResNetBasicStem) on the clips of the fork's driver-monitoring configs (DATA.INPUT_CHANNEL_NUM [1] / [1, 1]).
// Through the RGB stem trick (conv_stem.hip) such a clip would be padded to 4 channels: a tap row of 7 pixels becomes
// 28 floats padded to 32 of which 7 are real.  Here the clip stays at one float per pixel,
//   x [N][T][H + 2 pH][Wp], zero H/W borders (the conv's padding; Wp as engine.stem_geometry),
// and a direct VALU conv runs only the kT x 7 x 7 real taps (the f32 MFMA has the vector rate on this part, so a
// matrix form with K padded to 8 would buy nothing).  The weights are read in the parameter's own layout
// [Cout][1][kT][7][7]: nothing is packed or cached.
//
// Forward: one workgroup per (clip, output frame, band of BH output rows).  The kT x (2 BH + 5) input rows of the band
// and the weights (transposed to [tap][Cout]) sit in LDS; a thread owns a PAIR of neighbouring output positions x 8
// output channels: per (kt, kh) it reads 9 input floats (two 16-byte reads + one) and 7 x 8 weights (broadcast 16-byte
// reads) for 112 FMAs.  Scale / bias / ReLU, then 16-byte stores into the NDHWC slice.
// Weight gradient: the same bands; dz's band is staged too, a thread owns one tap x 8 output channels and walks the
// band's positions (1 input float + 8 dz floats -> 8 FMAs), summing over the frames its workgroup owns in registers.
// Every workgroup writes its partial dW to the workspace; a second kernel adds the partials in workgroup order —
// no atomics, so two runs are bitwise equal.
#include "common.h"

namespace {

constexpr int KH = 7, KW = 7, SH = 2, SW = 2, CB = 8, TPB = 256;
constexpr int LDS_SMALL = 64 * 1024, LDS_MAX = 128 * 1024;  // two workgroups per CU where a band fits the former

struct Stem1Args {
  const float* x; const float* w; const float* scale; const float* bias; const float* dz;
  float* out;
  int N, T, Hp, Wp, Cout, kT, pT, To, Ho, Wo, cs, coff, act;
  int BH, RB, LP, NP, nbands, tparts, vec;
};

// rows [2 h0, 2 h0 + RB) of the kT frames around output frame t -> xs [kT][RB][LP]; zero outside the frame range, the
// padded frame and the row pitch
__device__ __forceinline__ void stage_rows(const Stem1Args& q, float* xs, int n, int t, int h0) {
  const int per = q.RB * q.LP;
  for (int kt = 0; kt < q.kT; ++kt) {
    const int ti = t + kt - q.pT;
    const bool ok = (unsigned)ti < (unsigned)q.T;
    const float* src = q.x + ((long)n * q.T + (ok ? ti : 0)) * q.Hp * q.Wp;
    for (int e = threadIdx.x; e < per; e += TPB) {
      const int r = e / q.LP, c = e - r * q.LP;
      const int row = h0 * SH + r;
      xs[kt * per + e] = (ok && row < q.Hp && c < q.Wp) ? src[(long)row * q.Wp + c] : 0.f;
    }
  }
}

__global__ __launch_bounds__(TPB) void stem1_fwd_kernel(const Stem1Args q) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const xs = lds;                         // [kT][RB][LP], LP % 4 == 0
  float* const ws = lds + q.kT * q.RB * q.LP;    // [kT * 49][Cout]
  int b = blockIdx.x;
  const int band = b % q.nbands;
  b /= q.nbands;
  const int t = b % q.To, n = b / q.To;
  const int h0 = band * q.BH;
  const int K = q.kT * KH * KW;
  for (int e = threadIdx.x; e < K * q.Cout; e += TPB) {
    const int co = e / K, k = e - co * K;
    ws[k * q.Cout + co] = q.w[e];
  }
  stage_rows(q, xs, n, t, h0);
  __syncthreads();
  const bool relu = q.act == SF_ACT_RELU || q.act == SF_ACT_RELU6;
  const float hi = q.act == SF_ACT_RELU6 ? 6.f : 3.0e38f;
  const int items = (q.Cout / CB) * q.BH * q.NP;
  for (int it = threadIdx.x; it < items; it += TPB) {
    const int p = it % q.NP;
    const int r = it / q.NP;
    const int hl = r % q.BH, cb = r / q.BH;
    const int ho = h0 + hl;
    if (ho >= q.Ho) continue;
    float a0[CB], a1[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) a0[c] = a1[c] = 0.f;
    for (int kt = 0; kt < q.kT; ++kt) {
      for (int kh = 0; kh < KH; ++kh) {
        const float* xp = xs + (kt * q.RB + hl * SH + kh) * q.LP + 2 * SW * p;
        const f32x4 xa = *reinterpret_cast<const f32x4*>(xp);
        const f32x4 xb = *reinterpret_cast<const f32x4*>(xp + 4);
        const float xr[9] = {xa[0], xa[1], xa[2], xa[3], xb[0], xb[1], xb[2], xb[3], xp[8]};
        const float* wp = ws + (kt * KH + kh) * KW * q.Cout + cb * CB;
#pragma unroll
        for (int kw = 0; kw < KW; ++kw) {
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp + kw * q.Cout);
          const f32x4 w1 = *reinterpret_cast<const f32x4*>(wp + kw * q.Cout + 4);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            a0[c] = fmaf(xr[kw], w0[c], a0[c]);
            a0[4 + c] = fmaf(xr[kw], w1[c], a0[4 + c]);
            a1[c] = fmaf(xr[kw + SW], w0[c], a1[c]);
            a1[4 + c] = fmaf(xr[kw + SW], w1[c], a1[4 + c]);
          }
        }
      }
    }
    const int co0 = cb * CB;
    float sc[CB], bi[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      sc[c] = q.scale ? q.scale[co0 + c] : 1.f;
      bi[c] = q.bias ? q.bias[co0 + c] : 0.f;
    }
    const long row0 = (((long)n * q.To + t) * q.Ho + ho) * q.Wo;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int wo = 2 * p + j;
      if (wo >= q.Wo) continue;
      float v[CB];
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        v[c] = (j ? a1[c] : a0[c]) * sc[c] + bi[c];
        if (relu) v[c] = fminf(fmaxf(v[c], 0.f), hi);
      }
      float* o = q.out + (row0 + wo) * q.cs + q.coff + co0;
      if (q.vec) {
        *reinterpret_cast<f32x4*>(o) = (f32x4){v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(o + 4) = (f32x4){v[4], v[5], v[6], v[7]};
      } else {
#pragma unroll
        for (int c = 0; c < CB; ++c) o[c] = v[c];
      }
    }
  }
}

// workgroup = (clip, band, part of the output frames); partial dW [Cout][kT*49] per workgroup
template <int SLOTS>
__global__ __launch_bounds__(TPB) void stem1_wgrad_kernel(const Stem1Args q, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const xs = lds;                         // [kT][RB][LP]
  float* const gs = lds + q.kT * q.RB * q.LP;    // [BH * Wo][Cout]: dz of the band (zero past the last output row)
  int b = blockIdx.x;
  const int tz = b % q.tparts;
  b /= q.tparts;
  const int band = b % q.nbands, n = b / q.nbands;
  const int h0 = band * q.BH;
  const int K = q.kT * KH * KW;
  const int items = K * (q.Cout / CB);
  const int tper = (q.To + q.tparts - 1) / q.tparts;
  const int t0 = tz * tper, t1 = min(q.To, t0 + tper);
  const int npos = q.BH * q.Wo;

  float acc[SLOTS][CB];
  int xoff[SLOTS], goff[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[s][c] = 0.f;
    const int it = min(threadIdx.x + s * TPB, items - 1);  // item = (channel block, tap)
    const int tap = it % K, cb = it / K;
    const int kt = tap / (KH * KW), kh = (tap / KW) % KH, kw = tap % KW;
    xoff[s] = (kt * q.RB + kh) * q.LP + kw;
    goff[s] = cb * CB;
  }
  for (int t = t0; t < t1; ++t) {
    __syncthreads();  // the step before may still read xs / gs
    stage_rows(q, xs, n, t, h0);
    const long grow0 = (((long)n * q.To + t) * q.Ho + h0) * q.Wo;
    const int nvalid = min(q.BH, q.Ho - h0) * q.Wo;
    for (int e = threadIdx.x; e < npos * q.Cout; e += TPB) {
      const int pos = e / q.Cout, co = e - pos * q.Cout;
      gs[e] = pos < nvalid ? q.dz[(grow0 + pos) * q.cs + q.coff + co] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      if (threadIdx.x + s * TPB >= items) continue;
      for (int hl = 0; hl < q.BH; ++hl) {
        const float* xrow = xs + xoff[s] + hl * SH * q.LP;
        const float* grow = gs + hl * q.Wo * q.Cout + goff[s];
        for (int wo = 0; wo < q.Wo; ++wo) {
          const float xv = xrow[wo * SW];
          const f32x4 g0 = *reinterpret_cast<const f32x4*>(grow + wo * q.Cout);
          const f32x4 g1 = *reinterpret_cast<const f32x4*>(grow + wo * q.Cout + 4);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            acc[s][c] = fmaf(xv, g0[c], acc[s][c]);
            acc[s][4 + c] = fmaf(xv, g1[c], acc[s][4 + c]);
          }
        }
      }
    }
  }
  float* dst = part + (long)blockIdx.x * K * q.Cout;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int it = threadIdx.x + s * TPB;
    if (it >= items) continue;
    const int tap = it % K, cb = it / K;
#pragma unroll
    for (int c = 0; c < CB; ++c) dst[(cb * CB + c) * K + tap] = acc[s][c];
  }
}

// dW[e] (+)= sum of the workgroups' partials, in workgroup order
__global__ void stem1_wgrad_reduce_kernel(const float* __restrict__ part, int nparts, int KC, float* __restrict__ dw,
                                          int accumulate) {
  const int e = blockIdx.x * TPB + threadIdx.x;
  if (e >= KC) return;
  float s = 0.f;
  for (int g = 0; g < nparts; ++g) s += part[(long)g * KC + e];
  dw[e] = accumulate ? dw[e] + s : s;
}

__global__ void ncthw1_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int ph, int pw,
                                   int Wp, long total) {
  const long idx = (long)blockIdx.x * TPB + threadIdx.x;
  if (idx >= total) return;
  const int Hp = H + 2 * ph;
  const int xp = (int)(idx % Wp);
  const long r = idx / Wp;
  const int yp = (int)(r % Hp);
  const long f = r / Hp;  // frame (n, t): [N, 1, T, H, W] is [N * T] frames
  const int y = yp - ph, x = xp - pw;
  dst[idx] = (y >= 0 && y < H && x >= 0 && x < W) ? src[(f * H + y) * W + x] : 0.f;
}

// Geometry shared by the forward and the weight gradient.  false: not this file's shape.
bool stem1_plan(Stem1Args& q, int N, int T, int Hp, int Wp, int Cout, int kT, int pT, bool wgrad) {
  if (N <= 0 || T <= 0 || Hp < KH || Wp < KW || pT < 0 || kT < 1 || kT > 5) return false;
  if (Cout != 8 && Cout != 16 && Cout != 64) return false;
  q.N = N; q.T = T; q.Hp = Hp; q.Wp = Wp; q.Cout = Cout; q.kT = kT; q.pT = pT;
  q.To = T + 2 * pT - kT + 1;
  q.Ho = (Hp - KH) / SH + 1;
  q.Wo = (Wp - KW) / SW + 1;
  if (q.To <= 0) return false;
  q.NP = (q.Wo + 1) / 2;
  q.LP = (max(Wp, 2 * SW * q.NP + 5) + 3) / 4 * 4;  // a pair reads floats [4 p, 4 p + 9) of its row
  const int K = kT * KH * KW;
  if (wgrad && K * (Cout / CB) > 8 * TPB) return false;
  int bh = 8;
  if (!wgrad)
    while (bh > 2 && (long)N * q.To * sf_cdiv(q.Ho, bh) < 512) bh >>= 1;  // short grids: more, smaller bands
  const int bh0 = bh;
  bool fits = false;
  for (int limit = LDS_SMALL; !fits && limit <= LDS_MAX; limit += LDS_MAX - LDS_SMALL)
    for (bh = bh0; bh >= 1 && !fits; bh >>= 1) {
      const int rb = (bh - 1) * SH + KH;
      const long fl = (long)kT * rb * q.LP + (wgrad ? (long)bh * q.Wo * Cout : (long)K * Cout);
      fits = fl * (long)sizeof(float) <= limit;
      if (fits) break;
    }
  if (!fits) return false;
  q.BH = bh;
  q.RB = (bh - 1) * SH + KH;
  q.nbands = sf_cdiv(q.Ho, bh);
  q.tparts = 1;
  if (wgrad) {
    const long base = (long)N * q.nbands;
    q.tparts = (int)min((long)q.To, max(1L, (512 + base - 1) / base));
    const int tper = (q.To + q.tparts - 1) / q.tparts;
    q.tparts = (q.To + tper - 1) / tper;  // no empty part
  }
  return true;
}

size_t stem1_lds(const Stem1Args& q, bool wgrad) {
  return ((size_t)q.kT * q.RB * q.LP +
          (wgrad ? (size_t)q.BH * q.Wo * q.Cout : (size_t)q.kT * KH * KW * q.Cout)) * sizeof(float);
}

}  // namespace

extern "C" int sf_stem1_accepts(int Hp, int Wp, int Cout, int kT) {
  Stem1Args q;
  return stem1_plan(q, 1, kT, Hp, Wp, Cout, kT, kT / 2, false) && stem1_plan(q, 1, kT, Hp, Wp, Cout, kT, kT / 2, true)
             ? 1 : 0;
}

extern "C" int sf_stem1_fwd(const float* x, int N, int T, int Hp, int Wp, const float* w, int Cout, int kT, int pT,
                            const float* scale, const float* bias, int act, float* out, int out_cs, int out_coff,
                            void* stream) {
  if (!x || !w || !out || out_coff < 0 || out_coff + Cout > out_cs) return SF_EINVAL;
  if (act != SF_ACT_NONE && act != SF_ACT_RELU && act != SF_ACT_RELU6) return SF_EINVAL;
  Stem1Args q;
  if (!stem1_plan(q, N, T, Hp, Wp, Cout, kT, pT, false)) return SF_ENOTTAKEN;
  q.x = x; q.w = w; q.scale = scale; q.bias = bias; q.dz = nullptr; q.out = out;
  q.cs = out_cs; q.coff = out_coff; q.act = act;
  q.vec = (out_cs % 4 == 0 && out_coff % 4 == 0 && sf_aligned16(out)) ? 1 : 0;
  const long grid = (long)N * q.To * q.nbands;
  if (grid > 0x7fffffffL) return SF_EINVAL;
  static SfLdsAttr at;
  if (!sf_ensure_dyn_lds(at, reinterpret_cast<const void*>(stem1_fwd_kernel), LDS_MAX)) return SF_ELAUNCH;
  hipLaunchKernelGGL(stem1_fwd_kernel, dim3((unsigned)grid), dim3(TPB), stem1_lds(q, false), (hipStream_t)stream, q);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" long sf_stem1_wgrad_ws_floats(int N, int T, int Hp, int Wp, int Cout, int kT, int pT) {
  Stem1Args q;
  if (!stem1_plan(q, N, T, Hp, Wp, Cout, kT, pT, true)) return 0;
  return (long)N * q.nbands * q.tparts * kT * KH * KW * Cout;
}

extern "C" int sf_stem1_wgrad(const float* x, int N, int T, int Hp, int Wp, const float* dz, int dz_cs, int dz_coff,
                              int Cout, int kT, int pT, float* dw, int accumulate, float* ws, void* stream) {
  if (!x || !dz || !dw || !ws || dz_coff < 0 || dz_coff + Cout > dz_cs) return SF_EINVAL;
  Stem1Args q;
  if (!stem1_plan(q, N, T, Hp, Wp, Cout, kT, pT, true)) return SF_ENOTTAKEN;
  q.x = x; q.w = nullptr; q.scale = nullptr; q.bias = nullptr; q.dz = dz; q.out = nullptr;
  q.cs = dz_cs; q.coff = dz_coff; q.act = 0; q.vec = 0;
  const long grid = (long)N * q.nbands * q.tparts;
  if (grid > 0x7fffffffL) return SF_EINVAL;
  const int KC = kT * KH * KW * Cout;
  const int items = KC / CB;
  const size_t lds = stem1_lds(q, true);
  static SfLdsAttr at1, at2, at8;
  if (!sf_ensure_dyn_lds(at1, reinterpret_cast<const void*>(stem1_wgrad_kernel<1>), LDS_MAX) ||
      !sf_ensure_dyn_lds(at2, reinterpret_cast<const void*>(stem1_wgrad_kernel<2>), LDS_MAX) ||
      !sf_ensure_dyn_lds(at8, reinterpret_cast<const void*>(stem1_wgrad_kernel<8>), LDS_MAX))
    return SF_ELAUNCH;
  if (items <= TPB)
    hipLaunchKernelGGL(stem1_wgrad_kernel<1>, dim3((unsigned)grid), dim3(TPB), lds, (hipStream_t)stream, q, ws);
  else if (items <= 2 * TPB)
    hipLaunchKernelGGL(stem1_wgrad_kernel<2>, dim3((unsigned)grid), dim3(TPB), lds, (hipStream_t)stream, q, ws);
  else
    hipLaunchKernelGGL(stem1_wgrad_kernel<8>, dim3((unsigned)grid), dim3(TPB), lds, (hipStream_t)stream, q, ws);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(stem1_wgrad_reduce_kernel, dim3(sf_cdiv(KC, TPB)), dim3(TPB), 0, (hipStream_t)stream, ws,
                     (int)grid, KC, dw, accumulate);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_ncthw1_pack(const float* src, float* dst, int N, int T, int H, int W, int ph, int pw, int Wp,
                              void* stream) {
  if (!src || !dst || N <= 0 || T <= 0 || H <= 0 || W <= 0 || ph < 0 || pw < 0 || Wp < W + 2 * pw) return SF_EINVAL;
  const long total = (long)N * T * (H + 2 * ph) * Wp;
  hipLaunchKernelGGL(ncthw1_pack_kernel, dim3(sf_cdiv(total, TPB)), dim3(TPB), 0, (hipStream_t)stream, src, dst, H, W,
                     ph, pw, Wp, total);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
