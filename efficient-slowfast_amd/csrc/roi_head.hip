// roi_head.hip — the spatio-temporal action-detection head (ResNetRoIHead, reference head_helper.py:11-130):
//   s{p}_tpool  AvgPool3d([T,1,1], stride 1) + squeeze(2)       sf_roi_tpool_fwd
//   s{p}_roi    ROIAlign(R, 1/scale_factor, sampling_ratio 0)    } sf_roi_align_max_fwd (one kernel, per-(box, channel)
//   s{p}_spool  MaxPool2d(R, stride 1)                            }  winner byte kept for the backward)
//   backward of the three                                          sf_roi_align_max_bwd (gather form, no atomics)
//   backward of the head's sigmoid                                 sf_sigmoid_bwd
//
// RoIAlign semantics (detectron2 ROIAlign as the reference calls it, restated from its definition):
//   offset = aligned ? 0.5 : 0;  start = coord * scale - offset;  roi = end - start (legacy: max(roi, 1));
//   bin = roi / R;  grid = ceil(roi / R) per dimension (sampling_ratio 0);  count = max(gh * gw, 1);
//   sample (iy, ix) of bin (ph, pw): y = start_h + ph * bin_h + (iy + 0.5) * bin_h / gh (x likewise);
//   bilinear: y < -1 | y > H | x < -1 | x > W -> 0; negative coordinates clamp to 0; floor(y) >= H-1 -> both rows H-1;
//   bin value = sum of samples / count.  The max-pool keeps the FIRST maximal bin in row-major order (strict >).
//
// Safety: a box whose batch index does not truncate into [0, N) reads nothing and yields zeros; NaN coordinates make
// every sample invalid; every row / column index is clamped into the map before it is used.  The sampling grid is
// capped at ROI_GRID_MAX per bin and dimension (a bin wider than 64 feature cells: far outside any frame).
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int ROI_GRID_MAX = 64;

// ---------------------------------------------------------------- temporal average pool
template <int V>
__global__ __launch_bounds__(TPB) void roi_tpool_fwd_kernel(const float* __restrict__ x, int cs, int coff, int T,
                                                            int HW, int C, float* __restrict__ out, long total) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x;  // over N * HW * C / V
  if (i >= total) return;
  const int cv = C / V;
  const int c = (int)(i % cv) * V;
  const long p = i / cv;  // n * HW + hw
  const long n = p / HW, hw = p - n * HW;
  const float* src = x + ((n * T) * HW + hw) * cs + coff + c;
  const long tstep = (long)HW * cs;
  if constexpr (V == 4) {
    f32x4 s = *reinterpret_cast<const f32x4*>(src);
    for (int t = 1; t < T; ++t) s += *reinterpret_cast<const f32x4*>(src + t * tstep);
    *reinterpret_cast<f32x4*>(out + p * C + c) = s / (float)T;
  } else {
    float s = src[0];
    for (int t = 1; t < T; ++t) s += src[t * tstep];
    out[p * C + c] = s / (float)T;
  }
}

// ---------------------------------------------------------------- RoI geometry
struct RoiGeom {
  float sh, sw, bh, bw, inv_count;
  int gh, gw;
};

__device__ __forceinline__ int roi_grid(float roi, int R) {
  const float g = ceilf(roi / (float)R);
  return g > 0.f ? (int)fminf(g, (float)ROI_GRID_MAX) : 0;  // NaN / non-positive extents: no samples
}

__device__ __forceinline__ RoiGeom roi_geom(const float* b, int R, float scale, int aligned) {
  const float off = aligned ? 0.5f : 0.f;
  RoiGeom g;
  g.sw = b[1] * scale - off;
  g.sh = b[2] * scale - off;
  float rw = b[3] * scale - off - g.sw;
  float rh = b[4] * scale - off - g.sh;
  if (!aligned) {
    rw = fmaxf(rw, 1.f);
    rh = fmaxf(rh, 1.f);
  }
  g.bh = rh / (float)R;
  g.bw = rw / (float)R;
  g.gh = roi_grid(rh, R);
  g.gw = roi_grid(rw, R);
  g.inv_count = 1.f / (float)max(g.gh * g.gw, 1);
  return g;
}

// batch index as detectron2 reads it (truncation), -1 when it does not land in [0, N)
__device__ __forceinline__ int roi_batch(float bf, int N) {
  return (bf > -1.f && bf < (float)N) ? (int)bf : -1;
}

// One coordinate of a bilinear sample: lo / hi cell and the weight of hi; false when the sample contributes 0.
__device__ __forceinline__ bool roi_axis(float y, int H, int& lo, int& hi, float& l) {
  if (!(y >= -1.f && y <= (float)H)) return false;  // also NaN
  if (y <= 0.f) y = 0.f;
  lo = min((int)y, H - 1);
  if (lo >= H - 1) {
    hi = lo = H - 1;
    y = (float)lo;
  } else {
    hi = lo + 1;
  }
  l = y - (float)lo;
  return true;
}

// ---------------------------------------------------------------- fused RoIAlign + MaxPool2d(R) forward
// grid (K, ceil(C / TPB)): thread = (box, channel); 64 lanes of a wave read 64 consecutive channels of one cell.
__global__ __launch_bounds__(TPB) void roi_align_max_fwd_kernel(const float* __restrict__ x, int N, int H, int W,
                                                                int C, const float* __restrict__ boxes, int R,
                                                                float scale, int aligned, float* __restrict__ out,
                                                                int out_cs, int out_coff,
                                                                unsigned char* __restrict__ arg) {
  const int c = blockIdx.y * TPB + threadIdx.x;
  const int k = blockIdx.x;
  if (c >= C) return;
  const float* b = boxes + 5L * k;
  const int n = roi_batch(b[0], N);
  float best = 0.f;
  int bi = 0;
  if (n >= 0) {
    const RoiGeom g = roi_geom(b, R, scale, aligned);
    const float* xn = x + (long)n * H * W * C + c;
    for (int ph = 0; ph < R; ++ph) {
      for (int pw = 0; pw < R; ++pw) {
        float acc = 0.f;
        for (int iy = 0; iy < g.gh; ++iy) {
          const float y = g.sh + ph * g.bh + (iy + .5f) * g.bh / (float)g.gh;
          int y0, y1;
          float ly;
          if (!roi_axis(y, H, y0, y1, ly)) continue;
          const float hy = 1.f - ly;
          for (int ix = 0; ix < g.gw; ++ix) {
            const float xx = g.sw + pw * g.bw + (ix + .5f) * g.bw / (float)g.gw;
            int x0, x1;
            float lx;
            if (!roi_axis(xx, W, x0, x1, lx)) continue;
            const float hx = 1.f - lx;
            const float v00 = xn[((long)y0 * W + x0) * C], v01 = xn[((long)y0 * W + x1) * C];
            const float v10 = xn[((long)y1 * W + x0) * C], v11 = xn[((long)y1 * W + x1) * C];
            acc += hy * hx * v00 + hy * lx * v01 + ly * hx * v10 + ly * lx * v11;
          }
        }
        const float v = acc * g.inv_count;
        const int bin = ph * R + pw;
        if (bin == 0 || v > best || v != v) {  // torch's max-pool: first maximum, NaN wins
          best = v;
          bi = bin;
        }
      }
    }
  }
  out[(long)k * out_cs + out_coff + c] = best;
  arg[(long)k * C + c] = (unsigned char)bi;
}

// Sum over the samples of one bin of the weights that land on cell `h` along one axis (the bilinear weight
// factorises: w(h, w) = Wy(h) * Wx(w), and a sample is valid iff both of its coordinates are).
__device__ __forceinline__ float roi_axis_weight(float start, float bin, int grid, int p, int H, int h) {
  float s = 0.f;
  for (int i = 0; i < grid; ++i) {
    const float y = start + p * bin + (i + .5f) * bin / (float)grid;
    int lo, hi;
    float l;
    if (!roi_axis(y, H, lo, hi, l)) continue;
    s += (h == lo ? 1.f - l : 0.f) + (h == hi ? l : 0.f);
  }
  return s;
}

// ---------------------------------------------------------------- backward (gather form)
// dx[n, t, h, w, c] (+)= (1/T) * sum_{boxes k of clip n, in index order} dy[k, c] * Wy(h) Wx(w) / count
// over the samples of the winning bin arg[k, c].  Every output element is owned by one thread, so the result is
// bitwise reproducible.  grid (N * H * W, ceil(C / TPB)).
__global__ __launch_bounds__(TPB) void roi_align_max_bwd_kernel(const float* __restrict__ dy, int dy_cs, int dy_coff,
                                                                const unsigned char* __restrict__ arg,
                                                                const float* __restrict__ boxes, int K, int N, int T,
                                                                int H, int W, int C, int R, float scale, int aligned,
                                                                float* __restrict__ dx, int dx_cs, int dx_coff,
                                                                int accumulate) {
  const int c = blockIdx.y * TPB + threadIdx.x;
  const int p = blockIdx.x;  // (n * H + h) * W + w
  if (c >= C) return;
  const int w = p % W, h = (p / W) % H, n = p / (W * H);
  const float hf = (float)h, wf = (float)w;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) {
    const float* b = boxes + 5L * k;
    if (roi_batch(b[0], N) != n) continue;
    const RoiGeom g = roi_geom(b, R, scale, aligned);
    // cells any sample of this box can touch (conservative by one cell each side)
    const float y_lo = floorf(fmaxf(g.sh, 0.f)) - 1.f, y_hi = floorf(fmaxf(g.sh + g.bh * R, 0.f)) + 2.f;
    const float x_lo = floorf(fmaxf(g.sw, 0.f)) - 1.f, x_hi = floorf(fmaxf(g.sw + g.bw * R, 0.f)) + 2.f;
    if (!(hf >= y_lo && hf <= y_hi && wf >= x_lo && wf <= x_hi)) continue;
    const int bin = arg[(long)k * C + c];
    const int ph = bin / R, pw = bin - (bin / R) * R;
    const float wy = roi_axis_weight(g.sh, g.bh, g.gh, ph, H, h);
    if (wy == 0.f) continue;
    const float wx = roi_axis_weight(g.sw, g.bw, g.gw, pw, W, w);
    acc += dy[(long)k * dy_cs + dy_coff + c] * (wy * wx * g.inv_count);
  }
  const float v = acc / (float)T;
  float* d = dx + ((long)n * T * H * W + (long)h * W + w) * dx_cs + dx_coff + c;
  const long tstep = (long)H * W * dx_cs;
  if (accumulate) {
    for (int t = 0; t < T; ++t) d[t * tstep] += v;
  } else {
    for (int t = 0; t < T; ++t) d[t * tstep] = v;
  }
}

__global__ __launch_bounds__(TPB) void sigmoid_bwd_kernel(const float* y, const float* dy, float* dx, long n,
                                                          int accumulate) {
  const long i = (long)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const float s = y[i];
  const float g = dy[i] * (s * (1.f - s));
  dx[i] = accumulate ? dx[i] + g : g;
}

}  // namespace

extern "C" int sf_roi_tpool_fwd(const float* x, int cs, int coff, int N, int T, int H, int W, int C, float* out,
                                void* stream) {
  if (!x || !out || N <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || coff < 0 || coff + C > cs) return SF_EINVAL;
  const int HW = H * W;
  if (C % 4 == 0 && cs % 4 == 0 && coff % 4 == 0 && sf_aligned16(x) && sf_aligned16(out)) {
    const long total = (long)N * HW * (C / 4);
    hipLaunchKernelGGL(roi_tpool_fwd_kernel<4>, dim3(sf_cdiv(total, TPB)), dim3(TPB), 0, (hipStream_t)stream, x, cs,
                       coff, T, HW, C, out, total);
  } else {
    const long total = (long)N * HW * C;
    hipLaunchKernelGGL(roi_tpool_fwd_kernel<1>, dim3(sf_cdiv(total, TPB)), dim3(TPB), 0, (hipStream_t)stream, x, cs,
                       coff, T, HW, C, out, total);
  }
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_roi_align_max_fwd(const float* x, int N, int H, int W, int C, const float* boxes, int K, int R,
                                    float spatial_scale, int aligned, float* out, int out_cs, int out_coff,
                                    unsigned char* arg, void* stream) {
  if (!x || N <= 0 || H <= 0 || W <= 0 || C <= 0 || K < 0 || R <= 0 || R * R > 256) return SF_EINVAL;
  if (K == 0) return SF_OK;
  if (!boxes || !out || !arg || out_coff < 0 || out_coff + C > out_cs) return SF_EINVAL;
  hipLaunchKernelGGL(roi_align_max_fwd_kernel, dim3(K, sf_cdiv(C, TPB)), dim3(TPB), 0, (hipStream_t)stream, x, N, H,
                     W, C, boxes, R, spatial_scale, aligned, out, out_cs, out_coff, arg);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_roi_align_max_bwd(const float* dy, int dy_cs, int dy_coff, const unsigned char* arg,
                                    const float* boxes, int K, int N, int T, int H, int W, int C, int R,
                                    float spatial_scale, int aligned, float* dx, int dx_cs, int dx_coff,
                                    int accumulate, void* stream) {
  if (!dx || N <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || K < 0 || R <= 0 || R * R > 256) return SF_EINVAL;
  if (dx_coff < 0 || dx_coff + C > dx_cs || (long)N * H * W > 0x7fffffffL) return SF_EINVAL;
  if (K > 0 && (!dy || !arg || !boxes || dy_coff < 0 || dy_coff + C > dy_cs)) return SF_EINVAL;
  if (K == 0 && accumulate) return SF_OK;  // nothing to add
  // K == 0 and overwrite: the kernel writes the zeros (no box matches any clip)
  hipLaunchKernelGGL(roi_align_max_bwd_kernel, dim3(N * H * W, sf_cdiv(C, TPB)), dim3(TPB), 0, (hipStream_t)stream,
                     dy, dy_cs, dy_coff, arg, boxes, K, N, T, H, W, C, R, spatial_scale, aligned, dx, dx_cs, dx_coff,
                     accumulate);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_sigmoid_bwd(const float* y, const float* dy, float* dx, long n, int accumulate, void* stream) {
  if (n < 0 || (n > 0 && (!y || !dy || !dx))) return SF_EINVAL;
  if (n == 0) return SF_OK;
  hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3(sf_cdiv(n, TPB)), dim3(TPB), 0, (hipStream_t)stream, y, dy, dx, n,
                     accumulate);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
