// clip_sample.h — the pixel arithmetic of the input step, one copy for every file that resamples decoded frames
// (input_prologue.hip: per-clip, view and batch kernels; stream.hip: the streaming demo's frame ring), so that they
// cannot drift apart: a frame pushed into the ring holds the bits sf_clip_prologue writes for it.
#pragma once
#include "common.h"

struct NormArgs {
  float m[3], s[3];
};

__device__ __forceinline__ float norm1(unsigned char u, float m, float s) {
  return __fdiv_rn(__fdiv_rn((float)u, 255.f) - m, s);  // tensor/255 - mean, then /std (datasets/utils.py:306-314)
}

// torch upsample_bilinear (align_corners=False): src = scale*(dst+0.5)-0.5 clamped at 0; i0 = min(int(src), n-1);
// lambda = src - i0 clamped to [0,1]; i1 = i0 + (i0 < n-1).
__device__ __forceinline__ void src_index(float scale, int dst, int n, int* i0, int* i1, float* l0, float* l1) {
  float r = scale * ((float)dst + 0.5f) - 0.5f;
  if (r < 0.f) r = 0.f;
  int a = (int)r;
  if (a > n - 1) a = n - 1;
  float l = r - (float)a;
  l = fminf(fmaxf(l, 0.f), 1.f);
  *i0 = a;
  *i1 = a + (a < n - 1 ? 1 : 0);
  *l1 = l;
  *l0 = 1.f - l;
}

// The value of the scaled frame at (ys, xs), taken from the decoded frame `fr`: the three normalised channels in
// source order.  Shared by every kernel of the input step (so they write the same bits).
__device__ __forceinline__ void sample_rgb(const unsigned char* __restrict__ fr, int H, int W, int new_h, int new_w,
                                           int ys, int xs, const NormArgs& nm, float v[3]) {
  if (new_h == H && new_w == W) {
    const unsigned char* p = fr + ((long)ys * W + xs) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = norm1(p[c], nm.m[c], nm.s[c]);
  } else {
    int ya, yb, xa, xb;
    float ly0, ly1, lx0, lx1;
    src_index((float)H / (float)new_h, ys, H, &ya, &yb, &ly0, &ly1);
    src_index((float)W / (float)new_w, xs, W, &xa, &xb, &lx0, &lx1);
    const unsigned char* p00 = fr + ((long)ya * W + xa) * 3;
    const unsigned char* p01 = fr + ((long)ya * W + xb) * 3;
    const unsigned char* p10 = fr + ((long)yb * W + xa) * 3;
    const unsigned char* p11 = fr + ((long)yb * W + xb) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = norm1(p00[c], nm.m[c], nm.s[c]), b = norm1(p01[c], nm.m[c], nm.s[c]);
      const float d = norm1(p10[c], nm.m[c], nm.s[c]), e = norm1(p11[c], nm.m[c], nm.s[c]);
      v[c] = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * d + lx1 * e);
    }
  }
}
