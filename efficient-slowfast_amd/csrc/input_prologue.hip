// input_prologue.hip — the per-clip input step as ONE pass.
//
// Reference (CPU, per clip, datasets/kinetics.py:230-248): uint8 THWC frames -> tensor_normalize -> permute ->
// spatial_sampling (bilinear short-side scale, crop, horizontal flip) -> pack_pathway_output (slow = frames at
// linspace indices).  That is four full-size float tensors per clip on the host and a 4x larger H2D copy.
// Here the decoded uint8 clip is read once per pathway and the result lands directly in the stem's input layout
// (NDHWC, channels padded to 4, zero H/W borders, row pitch Wp): each thread owns one destination pixel, pulls
// its (up to 4) source taps, normalises them and writes one aligned 16-byte store.  HBM-bound: 3 B read per tap,
// 16 B written per pixel.
#include "clip_sample.h"  // NormArgs, norm1, src_index, sample_rgb: shared with stream.hip
#include "mix_row.h"

namespace {
constexpr int TPB = 256;

// One-channel frame: one normalised value.
__device__ __forceinline__ float sample_gray(const unsigned char* __restrict__ fr, int H, int W, int new_h, int new_w,
                                             int ys, int xs, float mean, float stdv) {
  if (new_h == H && new_w == W) return norm1(fr[(long)ys * W + xs], mean, stdv);
  int ya, yb, xa, xb;
  float ly0, ly1, lx0, lx1;
  src_index((float)H / (float)new_h, ys, H, &ya, &yb, &ly0, &ly1);
  src_index((float)W / (float)new_w, xs, W, &xa, &xb, &lx0, &lx1);
  const float a = norm1(fr[(long)ya * W + xa], mean, stdv), b = norm1(fr[(long)ya * W + xb], mean, stdv);
  const float d = norm1(fr[(long)yb * W + xa], mean, stdv), e = norm1(fr[(long)yb * W + xb], mean, stdv);
  return ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * d + lx1 * e);
}

__global__ void clip_prologue_kernel(const unsigned char* __restrict__ clip, int T, int H, int W, int new_h,
                                     int new_w, int y0, int x0, int crop, int flip, int reverse, NormArgs nm,
                                     const int* __restrict__ frame_idx, int n_frames, float* __restrict__ dst, int ph,
                                     int pw, int Wp, long total) {
  const long idx = (long)blockIdx.x * TPB + threadIdx.x;
  if (idx >= total) return;
  const int Hp = crop + 2 * ph;
  const int xp = (int)(idx % Wp);
  long r = idx / Wp;
  const int yp = (int)(r % Hp);
  const int f = (int)(r / Hp);
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  const int yy = yp - ph, xx = xp - pw;
  if (yy >= 0 && yy < crop && xx >= 0 && xx < crop) {
    const int t = frame_idx ? frame_idx[f] : f;
    const int ys = y0 + yy;                            // row in the scaled image
    const int xs = x0 + (flip ? crop - 1 - xx : xx);   // column in the scaled image (flip is applied after the crop)
    float v[3];
    sample_rgb(clip + (long)t * H * W * 3, H, W, new_h, new_w, ys, xs, nm, v);
    if (reverse) {  // DATA.REVERSE_INPUT_CHANNEL: frames[[2, 1, 0]]
      o[0] = v[2]; o[1] = v[1]; o[2] = v[0];
    } else {
      o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
  }
  *reinterpret_cast<f32x4*>(dst + idx * 4) = o;
}
// One-channel (grayscale) clip, uint8 [T,H,W]: the same arithmetic, one float per destination pixel — the one-channel
// stem layout of conv_stem_gray.hip ([n_frames][crop + 2 ph][Wp], zero borders).
__global__ void clip_prologue_gray_kernel(const unsigned char* __restrict__ clip, int T, int H, int W, int new_h,
                                          int new_w, int y0, int x0, int crop, int flip, float mean, float stdv,
                                          const int* __restrict__ frame_idx, int n_frames, float* __restrict__ dst,
                                          int ph, int pw, int Wp, long total) {
  const long idx = (long)blockIdx.x * TPB + threadIdx.x;
  if (idx >= total) return;
  const int Hp = crop + 2 * ph;
  const int xp = (int)(idx % Wp);
  long r = idx / Wp;
  const int yp = (int)(r % Hp);
  const int f = (int)(r / Hp);
  float o = 0.f;
  const int yy = yp - ph, xx = xp - pw;
  if (yy >= 0 && yy < crop && xx >= 0 && xx < crop) {
    const int t = min(max(frame_idx ? frame_idx[f] : f, 0), T - 1);
    const int ys = y0 + yy;
    const int xs = x0 + (flip ? crop - 1 - xx : xx);
    o = sample_gray(clip + (long)t * H * W, H, W, new_h, new_w, ys, xs, mean, stdv);
  }
  dst[idx] = o;
}

// ---- all views of one decoded video, both pathways, in ONE launch (tools/test_net.py's protocol: TEST.NUM_ENSEMBLE_VIEWS
// x TEST.NUM_SPATIAL_CROPS views per video).  The grid is (pixels of one padded frame, Fast frame, view): the view's
// table row, the frame's index and the "is this Fast frame also a Slow frame" search are uniform per workgroup (scalar
// loads), a thread owns one destination pixel of one Fast frame, computes it once with the per-clip kernels' arithmetic
// and stores it to the Fast buffer and — when slow_idx names the frame — to the Slow buffer too.  Every element of both
// buffers has exactly one owner (slow_idx holds distinct frames), consecutive threads write consecutive 16-byte chunks.
constexpr int VIEW_ROW = 5;  // new_h, new_w, y0, x0, flip

struct ViewGeo {
  int new_h, new_w, y0, x0, flip, ok;
};

__device__ __forceinline__ ViewGeo view_row(const int* __restrict__ views, int v, int crop) {
  const int* r = views + (long)v * VIEW_ROW;
  ViewGeo g = {r[0], r[1], r[2], r[3], r[4], 0};
  // the host entry checked its copy of the table; a row that differs on the device yields zeros, never a wild read
  g.ok = g.new_h > 0 && g.new_w > 0 && g.y0 >= 0 && g.x0 >= 0 && g.y0 + crop <= g.new_h && g.x0 + crop <= g.new_w;
  return g;
}

__global__ void clip_views_kernel(const unsigned char* __restrict__ video, int T, int H, int W,
                                  const int* __restrict__ views, const int* __restrict__ frame_idx,
                                  const int* __restrict__ slow_idx, int n_fast, int n_slow, int crop, int reverse,
                                  NormArgs nm, float* __restrict__ fast, float* __restrict__ slow, int ph, int pw, int Wp,
                                  int plane) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= plane) return;
  const int f = blockIdx.y, v = blockIdx.z;
  const ViewGeo g = view_row(views, v, crop);
  const int yp = p / Wp, xp = p - yp * Wp;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  const int yy = yp - ph, xx = xp - pw;
  if (g.ok && yy >= 0 && yy < crop && xx >= 0 && xx < crop) {
    const int t = min(max(frame_idx[(long)v * n_fast + f], 0), T - 1);
    const int ys = g.y0 + yy;
    const int xs = g.x0 + (g.flip ? crop - 1 - xx : xx);
    float c[3];
    sample_rgb(video + (long)t * H * W * 3, H, W, g.new_h, g.new_w, ys, xs, nm, c);
    if (reverse) {
      o[0] = c[2]; o[1] = c[1]; o[2] = c[0];
    } else {
      o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    }
  }
  *reinterpret_cast<f32x4*>(fast + (((long)v * n_fast + f) * plane + p) * 4) = o;
  for (int j = 0; j < n_slow; ++j)  // n_slow <= n_fast / alpha entries, wave-uniform
    if (slow_idx[j] == f) *reinterpret_cast<f32x4*>(slow + (((long)v * n_slow + j) * plane + p) * 4) = o;
}

// One-channel video: VEC = 4 pixels of one row per thread (one 16-byte store; needs Wp % 4 == 0 and 16-byte aligned
// buffers) or VEC = 1 (any pitch).  `plane` counts threads' units: Hp * Wp / VEC.
template <int VEC>
__global__ void clip_views_gray_kernel(const unsigned char* __restrict__ video, int T, int H, int W,
                                       const int* __restrict__ views, const int* __restrict__ frame_idx,
                                       const int* __restrict__ slow_idx, int n_fast, int n_slow, int crop, float mean,
                                       float stdv, float* __restrict__ fast, float* __restrict__ slow, int ph, int pw,
                                       int Wp, int plane) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= plane) return;
  const int f = blockIdx.y, v = blockIdx.z;
  const ViewGeo g = view_row(views, v, crop);
  const int wq = Wp / VEC;
  const int yp = p / wq, xp0 = (p - yp * wq) * VEC;
  const int yy = yp - ph;
  float o[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) o[i] = 0.f;
  if (g.ok && yy >= 0 && yy < crop) {
    const int t = min(max(frame_idx[(long)v * n_fast + f], 0), T - 1);
    const unsigned char* fr = video + (long)t * H * W;
    const int ys = g.y0 + yy;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const int xx = xp0 + i - pw;
      if (xx >= 0 && xx < crop)
        o[i] = sample_gray(fr, H, W, g.new_h, g.new_w, ys, g.x0 + (g.flip ? crop - 1 - xx : xx), mean, stdv);
    }
  }
  const long fo = (((long)v * n_fast + f) * plane + p) * VEC;
  if constexpr (VEC == 4) {
    const f32x4 q = {o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(fast + fo) = q;
    for (int j = 0; j < n_slow; ++j)
      if (slow_idx[j] == f) *reinterpret_cast<f32x4*>(slow + (((long)v * n_slow + j) * plane + p) * VEC) = q;
  } else {
    fast[fo] = o[0];
    for (int j = 0; j < n_slow; ++j)
      if (slow_idx[j] == f) slow[((long)v * n_slow + j) * plane + p] = o[0];
  }
}

// Host-side check of the view table's host copy: rows [V][5], then frame indices [V][n_fast], then n_slow Slow indices.
bool view_table_ok(const int* tab, int T, int V, int n_fast, int n_slow, int crop) {
  for (int v = 0; v < V; ++v) {
    const int* r = tab + (long)v * VIEW_ROW;
    if (r[0] <= 0 || r[1] <= 0 || r[2] < 0 || r[3] < 0 || (long)r[2] + crop > r[0] || (long)r[3] + crop > r[1])
      return false;
  }
  const int* fi = tab + (long)V * VIEW_ROW;
  for (long i = 0; i < (long)V * n_fast; ++i)
    if (fi[i] < 0 || fi[i] >= T) return false;
  const int* si = fi + (long)V * n_fast;
  for (int j = 0; j < n_slow; ++j)
    if (si[j] < 0 || si[j] >= n_fast || (j > 0 && si[j] <= si[j - 1])) return false;  // distinct: one owner per Slow frame
  return true;
}

// Shared argument checks of the two entries; on success *plane = (crop + 2 ph) * Wp.
bool clip_views_args_ok(const void* video, int T, int H, int W, const int* table_host, const int* table, int V, int n_fast,
                        int n_slow, int crop, const float* fast, const float* slow, int ph, int pw, int Wp, long* plane) {
  if (!video || !table_host || !table || !fast || T <= 0 || H <= 0 || W <= 0 || V <= 0 || n_fast <= 0 || crop <= 0 ||
      ph < 0 || pw < 0)
    return false;
  if (n_slow < 0 || n_slow > n_fast || (slow == nullptr) != (n_slow == 0)) return false;
  if (V > 65535 || n_fast > 65535 || Wp < crop + 2 * pw) return false;
  *plane = (long)(crop + 2 * ph) * Wp;
  if (*plane > 0x7fffffffL / 4) return false;
  return view_table_ok(table_host, T, V, n_fast, n_slow, crop);
}

// ---- all B clips of one TRAINING batch, both pathways, in ONE launch (datasets/kinetics.py:142-165, :186-189, :230-248
// per sample; the loader's collate step stacks B of them).  Unlike the views of one video the B decoded spans are
// separate allocations of their own T_i x H_i x W_i, so the table row carries the clip's device address and extents
// beside its scale / crop / flip.  The grid is (pixels of one padded frame, Fast frame, clip); everything else is
// clip_views_kernel: the row, the frame index and the Slow search are uniform per workgroup, a thread owns one
// destination pixel of one Fast frame, computes it once with sample_rgb / sample_gray and stores it to the Fast buffer
// and — when slow_idx names the frame — to the Slow buffer.
constexpr int BATCH_ROW = 9;  // clip address, T, H, W, new_h, new_w, y0, x0, flip (int64 each)

struct ClipGeo {
  const unsigned char* clip;
  int T, H, W, new_h, new_w, y0, x0, flip, ok;
};

// One row's check, shared by the host entry (its copy of the table) and the kernel (the device copy): a row that
// fails yields zeros on the device, never a read.  Extents must fit an int: the pixel arithmetic is 32-bit per frame.
__host__ __device__ __forceinline__ bool batch_row_ok(const long* r, int crop) {
  const long lim = 0x7fffffffL;
  return r[0] != 0 && r[1] > 0 && r[1] <= lim && r[2] > 0 && r[2] <= lim && r[3] > 0 && r[3] <= lim && r[4] > 0 &&
         r[4] <= lim && r[5] > 0 && r[5] <= lim && r[6] >= 0 && r[6] <= lim && r[7] >= 0 && r[7] <= lim && r[6] + crop <= r[4] && r[7] + crop <= r[5];
}

__device__ __forceinline__ ClipGeo batch_row(const long* __restrict__ tab, int b, int crop) {
  const long* r = tab + (long)b * BATCH_ROW;
  ClipGeo g;
  // the address names global memory (a hipMalloc'ed span): say so, or every tap becomes a flat load
  g.clip = (const unsigned char*)(const __attribute__((address_space(1))) unsigned char*)(unsigned long)r[0];
  g.T = (int)r[1]; g.H = (int)r[2]; g.W = (int)r[3];
  g.new_h = (int)r[4]; g.new_w = (int)r[5]; g.y0 = (int)r[6]; g.x0 = (int)r[7];
  g.flip = r[8] != 0;
  g.ok = batch_row_ok(r, crop);
  return g;
}

__global__ void clip_batch_kernel(const long* __restrict__ tab, const long* __restrict__ frame_idx,
                                  const long* __restrict__ slow_idx, int n_fast, int n_slow, int crop, int reverse,
                                  NormArgs nm, float* __restrict__ fast, float* __restrict__ slow, int ph, int pw, int Wp,
                                  int plane) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= plane) return;
  const int f = blockIdx.y, b = blockIdx.z;
  const ClipGeo g = batch_row(tab, b, crop);
  const int yp = p / Wp, xp = p - yp * Wp;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  const int yy = yp - ph, xx = xp - pw;
  if (g.ok && yy >= 0 && yy < crop && xx >= 0 && xx < crop) {
    const long ft = frame_idx[(long)b * n_fast + f];
    const int t = ft < 0 ? 0 : (ft > g.T - 1 ? g.T - 1 : (int)ft);  // clamped into [0, T_i)
    const int ys = g.y0 + yy;
    const int xs = g.x0 + (g.flip ? crop - 1 - xx : xx);
    float c[3];
    sample_rgb(g.clip + (long)t * g.H * g.W * 3, g.H, g.W, g.new_h, g.new_w, ys, xs, nm, c);
    if (reverse) {
      o[0] = c[2]; o[1] = c[1]; o[2] = c[0];
    } else {
      o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    }
  }
  *reinterpret_cast<f32x4*>(fast + (((long)b * n_fast + f) * plane + p) * 4) = o;
  for (int j = 0; j < n_slow; ++j)  // n_slow <= n_fast / alpha entries, wave-uniform
    if (slow_idx[j] == f) *reinterpret_cast<f32x4*>(slow + (((long)b * n_slow + j) * plane + p) * 4) = o;
}

// One-channel clips: VEC as in clip_views_gray_kernel; `plane` counts threads' units: Hp * Wp / VEC.
template <int VEC>
__global__ void clip_batch_gray_kernel(const long* __restrict__ tab, const long* __restrict__ frame_idx,
                                       const long* __restrict__ slow_idx, int n_fast, int n_slow, int crop, float mean,
                                       float stdv, float* __restrict__ fast, float* __restrict__ slow, int ph, int pw,
                                       int Wp, int plane) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= plane) return;
  const int f = blockIdx.y, b = blockIdx.z;
  const ClipGeo g = batch_row(tab, b, crop);
  const int wq = Wp / VEC;
  const int yp = p / wq, xp0 = (p - yp * wq) * VEC;
  const int yy = yp - ph;
  float o[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) o[i] = 0.f;
  if (g.ok && yy >= 0 && yy < crop) {
    const long ft = frame_idx[(long)b * n_fast + f];
    const int t = ft < 0 ? 0 : (ft > g.T - 1 ? g.T - 1 : (int)ft);  // clamped into [0, T_i)
    const unsigned char* fr = g.clip + (long)t * g.H * g.W;
    const int ys = g.y0 + yy;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const int xx = xp0 + i - pw;
      if (xx >= 0 && xx < crop)
        o[i] = sample_gray(fr, g.H, g.W, g.new_h, g.new_w, ys, g.x0 + (g.flip ? crop - 1 - xx : xx), mean, stdv);
    }
  }
  const long fo = (((long)b * n_fast + f) * plane + p) * VEC;
  if constexpr (VEC == 4) {
    const f32x4 q = {o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(fast + fo) = q;
    for (int j = 0; j < n_slow; ++j)
      if (slow_idx[j] == f) *reinterpret_cast<f32x4*>(slow + (((long)b * n_slow + j) * plane + p) * VEC) = q;
  } else {
    fast[fo] = o[0];
    for (int j = 0; j < n_slow; ++j)
      if (slow_idx[j] == f) slow[((long)b * n_slow + j) * plane + p] = o[0];
  }
}

// ---- the same batch with mixup / CutMix inside the launch (upstream datasets/mixup.py, MixUp._mix_batch on the collated
// float batch): the table carries B mix rows (mix_row.h) behind the Slow positions.  A mixed pixel is the pixel of
// clip b, of its partner p (CutMix inside the box: still one resample), or both combined (mixup: two resamples, both
// uint8 reads) — clip p through its own row and its own frame index.  Grid, ownership and stores are clip_batch_kernel's.
struct MixGeo {
  int partner, mode, y0, x0, y1, x1, ok;
  float lam;
};

__device__ __forceinline__ MixGeo mix_row(const long* __restrict__ mix, int b, int B, int crop) {
  const long* r = mix + (long)b * MIX_ROW;
  MixGeo m;
  // the host entry checked its copy of the rows; a row that differs on the device yields zeros, never a wild read
  m.ok = mix_row_ok(r, B) && mix_box_ok(r, crop);
  m.partner = m.ok ? (int)r[0] : b;
  m.mode = (int)r[1];
  m.lam = mix_lambda(r[2]);
  m.y0 = (int)r[3]; m.x0 = (int)r[4]; m.y1 = (int)r[5]; m.x1 = (int)r[6];
  return m;
}

// lam * own + (1 - lam) * other as torch computes it on float32 tensors: two rounded products and one rounded sum.
// HIP's __fmul_rn / __fadd_rn are plain operators, which the build's -ffp-contract=fast fuses into an fma whatever a
// contract pragma says: the products pass through an empty asm, so the sum only ever sees the rounded values.
__device__ __forceinline__ float mix2(float lam, float rest, float own, float other) {
  float a = __fmul_rn(lam, own), b = __fmul_rn(rest, other);
  asm("" : "+v"(a), "+v"(b));
  return __fadd_rn(a, b);
}

// the frame of clip `b` that Fast position f takes, clamped into [0, T_b)
__device__ __forceinline__ const unsigned char* batch_frame(const ClipGeo& g, const long* __restrict__ frame_idx, int b,
                                                            int n_fast, int f, int channels) {
  const long ft = frame_idx[(long)b * n_fast + f];
  const int t = ft < 0 ? 0 : (ft > g.T - 1 ? g.T - 1 : (int)ft);
  return g.clip + (long)t * g.H * g.W * channels;
}

__global__ void clip_batch_mix_kernel(const long* __restrict__ tab, const long* __restrict__ frame_idx,
                                      const long* __restrict__ slow_idx, const long* __restrict__ mix, int B, int n_fast,
                                      int n_slow, int crop, int reverse, NormArgs nm, float* __restrict__ fast,
                                      float* __restrict__ slow, int ph, int pw, int Wp, int plane) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= plane) return;
  const int f = blockIdx.y, b = blockIdx.z;
  const MixGeo mg = mix_row(mix, b, B, crop);
  const ClipGeo g = batch_row(tab, b, crop);
  const ClipGeo gp = batch_row(tab, mg.partner, crop);
  const int yp = p / Wp, xp = p - yp * Wp;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  const int yy = yp - ph, xx = xp - pw;
  if (mg.ok && g.ok && gp.ok && yy >= 0 && yy < crop && xx >= 0 && xx < crop) {
    const unsigned char* own = batch_frame(g, frame_idx, b, n_fast, f, 3);
    const unsigned char* oth = batch_frame(gp, frame_idx, mg.partner, n_fast, f, 3);
    const bool boxed = mg.mode == MIX_CUTMIX && yy >= mg.y0 && yy < mg.y1 && xx >= mg.x0 && xx < mg.x1;
    float c[3];
    if (boxed)
      sample_rgb(oth, gp.H, gp.W, gp.new_h, gp.new_w, gp.y0 + yy, gp.x0 + (gp.flip ? crop - 1 - xx : xx), nm, c);
    else
      sample_rgb(own, g.H, g.W, g.new_h, g.new_w, g.y0 + yy, g.x0 + (g.flip ? crop - 1 - xx : xx), nm, c);
    if (mg.mode == MIX_MIXUP) {  // two roundings of a product and one of the sum, never an fma: torch's x * lam + y * (1 - lam)
      float d[3];
      sample_rgb(oth, gp.H, gp.W, gp.new_h, gp.new_w, gp.y0 + yy, gp.x0 + (gp.flip ? crop - 1 - xx : xx), nm, d);
      const float rest = __fsub_rn(1.0f, mg.lam);
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = mix2(mg.lam, rest, c[k], d[k]);
    }
    if (reverse) {
      o[0] = c[2]; o[1] = c[1]; o[2] = c[0];
    } else {
      o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    }
  }
  *reinterpret_cast<f32x4*>(fast + (((long)b * n_fast + f) * plane + p) * 4) = o;
  for (int j = 0; j < n_slow; ++j)  // n_slow <= n_fast / alpha entries, wave-uniform
    if (slow_idx[j] == f) *reinterpret_cast<f32x4*>(slow + (((long)b * n_slow + j) * plane + p) * 4) = o;
}

// One-channel clips: VEC as in clip_batch_gray_kernel.
template <int VEC>
__global__ void clip_batch_mix_gray_kernel(const long* __restrict__ tab, const long* __restrict__ frame_idx,
                                           const long* __restrict__ slow_idx, const long* __restrict__ mix, int B,
                                           int n_fast, int n_slow, int crop, float mean, float stdv,
                                           float* __restrict__ fast, float* __restrict__ slow, int ph, int pw, int Wp,
                                           int plane) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= plane) return;
  const int f = blockIdx.y, b = blockIdx.z;
  const MixGeo mg = mix_row(mix, b, B, crop);
  const ClipGeo g = batch_row(tab, b, crop);
  const ClipGeo gp = batch_row(tab, mg.partner, crop);
  const int wq = Wp / VEC;
  const int yp = p / wq, xp0 = (p - yp * wq) * VEC;
  const int yy = yp - ph;
  float o[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) o[i] = 0.f;
  if (mg.ok && g.ok && gp.ok && yy >= 0 && yy < crop) {
    const unsigned char* own = batch_frame(g, frame_idx, b, n_fast, f, 1);
    const unsigned char* oth = batch_frame(gp, frame_idx, mg.partner, n_fast, f, 1);
    const bool rows = mg.mode == MIX_CUTMIX && yy >= mg.y0 && yy < mg.y1;
    const float rest = __fsub_rn(1.0f, mg.lam);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const int xx = xp0 + i - pw;
      if (xx >= 0 && xx < crop) {
        float v;
        if (rows && xx >= mg.x0 && xx < mg.x1)
          v = sample_gray(oth, gp.H, gp.W, gp.new_h, gp.new_w, gp.y0 + yy, gp.x0 + (gp.flip ? crop - 1 - xx : xx), mean,
                          stdv);
        else
          v = sample_gray(own, g.H, g.W, g.new_h, g.new_w, g.y0 + yy, g.x0 + (g.flip ? crop - 1 - xx : xx), mean, stdv);
        if (mg.mode == MIX_MIXUP) {
          const float d = sample_gray(oth, gp.H, gp.W, gp.new_h, gp.new_w, gp.y0 + yy,
                                      gp.x0 + (gp.flip ? crop - 1 - xx : xx), mean, stdv);
          v = mix2(mg.lam, rest, v, d);
        }
        o[i] = v;
      }
    }
  }
  const long fo = (((long)b * n_fast + f) * plane + p) * VEC;
  if constexpr (VEC == 4) {
    const f32x4 q = {o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(fast + fo) = q;
    for (int j = 0; j < n_slow; ++j)
      if (slow_idx[j] == f) *reinterpret_cast<f32x4*>(slow + (((long)b * n_slow + j) * plane + p) * VEC) = q;
  } else {
    fast[fo] = o[0];
    for (int j = 0; j < n_slow; ++j)
      if (slow_idx[j] == f) slow[((long)b * n_slow + j) * plane + p] = o[0];
  }
}

// Host-side check of the mix rows behind a batch table: [B][SF_MIX_ROW] after the Slow positions.
bool mix_table_ok(const long* tab, int B, int n_fast, int n_slow, int crop) {
  const long* mix = tab + (long)B * (BATCH_ROW + n_fast) + n_slow;
  for (int b = 0; b < B; ++b)
    if (!mix_row_ok(mix + (long)b * MIX_ROW, B) || !mix_box_ok(mix + (long)b * MIX_ROW, crop)) return false;
  return true;
}

// Host-side check of the batch table's host copy: rows [B][9], then frame indices [B][n_fast], then n_slow Slow positions.
bool batch_table_ok(const long* tab, int B, int n_fast, int n_slow, int crop) {
  for (int b = 0; b < B; ++b)
    if (!batch_row_ok(tab + (long)b * BATCH_ROW, crop)) return false;
  const long* fi = tab + (long)B * BATCH_ROW;
  for (int b = 0; b < B; ++b) {
    const long T = tab[(long)b * BATCH_ROW + 1];
    for (int f = 0; f < n_fast; ++f)
      if (fi[(long)b * n_fast + f] < 0 || fi[(long)b * n_fast + f] >= T) return false;
  }
  const long* si = fi + (long)B * n_fast;
  for (int j = 0; j < n_slow; ++j)
    if (si[j] < 0 || si[j] >= n_fast || (j > 0 && si[j] <= si[j - 1])) return false;  // distinct: one owner per Slow frame
  return true;
}

// Shared argument checks of the two batch entries; on success *plane = (crop + 2 ph) * Wp.
bool clip_batch_args_ok(const long* table_host, const long* table, int B, int n_fast, int n_slow, int crop,
                        const float* fast, const float* slow, int ph, int pw, int Wp, long* plane) {
  if (!table_host || !table || !fast || B <= 0 || n_fast <= 0 || crop <= 0 || ph < 0 || pw < 0) return false;
  if (n_slow < 0 || n_slow > n_fast || (slow == nullptr) != (n_slow == 0)) return false;
  if (B > 65535 || n_fast > 65535 || Wp < crop + 2 * pw) return false;
  *plane = (long)(crop + 2 * ph) * Wp;
  if (*plane > 0x7fffffffL / 4) return false;
  return batch_table_ok(table_host, B, n_fast, n_slow, crop);
}

// ---- the same batch with Jester's colour jitter inside the launch (decoder.py:456-469 -> transform.py:692-717,
// RandomColorJitter: PIL's ImageEnhance.Brightness, then Contrast, then Color, on every sampled uint8 frame before
// tensor_normalize).  The table carries B jitter rows behind the Slow positions: three float32 factors per CLIP.  The
// contrast stage blends against the frame's grey mean, a reduction over the whole decoded frame, so a first launch
// (frame_grey_means_kernel) leaves one int per (clip, Fast frame) and the clip launch reads it.  Checked against
// Pillow 12.2.0: PIL casts the factor to a C float and blends in float32, one rounded product and one rounded sum.
constexpr int JITTER_ROW = SF_JITTER_ROW;  // brightness, contrast, colour: float32 bits in the low half of an int64

struct JitGeo {
  float fb, fc, fs;
  int m, ok;  // m: the frame's grey mean (the contrast stage's other image)
};

// a factor word: the high half zero and the float finite (checked on the host copy and again on the device copy)
__host__ __device__ __forceinline__ bool jitter_row_ok(const long* r) {
  for (int i = 0; i < JITTER_ROW; ++i)
    if (r[i] < 0 || r[i] > 0xffffffffL || ((unsigned)r[i] & 0x7f800000u) == 0x7f800000u) return false;
  return true;
}

__device__ __forceinline__ JitGeo jitter_row(const long* __restrict__ jit, int b) {
  const long* r = jit + (long)b * JITTER_ROW;
  JitGeo j;
  j.ok = jitter_row_ok(r);
  j.fb = __uint_as_float((unsigned)r[0]);
  j.fc = __uint_as_float((unsigned)r[1]);
  j.fs = __uint_as_float((unsigned)r[2]);
  j.m = 0;
  return j;
}

// Image.blend(x0, x1, f) on uint8 values: fl(x0 + fl(f * (x1 - x0))), the product kept from fusing into the sum as in
// mix2.  For 0 <= f <= 1 PIL truncates, otherwise it clips to [0, 255] and truncates: one expression serves both,
// because inside [0, 1] the rounded sum cannot leave [min(x0, x1), max(x0, x1)].
__device__ __forceinline__ int blend8(float f, int x0, int x1) {
  float p = __fmul_rn(f, (float)(x1 - x0));
  asm("" : "+v"(p));
  const float t = __fadd_rn((float)x0, p);
  return (int)fminf(fmaxf(t, 0.f), 255.f);
}

// ImageEnhance.Brightness: blend against black
__device__ __forceinline__ void bright3(float fb, int c[3]) {
  if (fb > 0.f) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = blend8(fb, 0, c[k]);
  }
}

// convert("L"): ITU-R 601-2 luma in 16-bit fixed point
__device__ __forceinline__ int grey3(const int c[3]) { return (19595 * c[0] + 38470 * c[1] + 7471 * c[2] + 32768) >> 16; }

// The jitter of ONE source pixel, uint8 in and uint8 out: what every tap of the resampling reads.  A stage whose
// factor is <= 0 is skipped (transform.py:706-717).
__device__ __forceinline__ void jitter_px(const unsigned char* __restrict__ p, const JitGeo& j, unsigned char u[3]) {
  int c[3] = {p[0], p[1], p[2]};
  bright3(j.fb, c);
  if (j.fc > 0.f) {  // ImageEnhance.Contrast: blend against the frame's grey mean
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = blend8(j.fc, j.m, c[k]);
  }
  if (j.fs > 0.f) {  // ImageEnhance.Color: blend against the pixel's own grey
    const int l = grey3(c);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = blend8(j.fs, l, c[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = (unsigned char)c[k];
}

// The weighted sum of four normalised taps with the roundings sample_rgb's `ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * d +
// lx1 * e)` has in the plain kernels.  There the build's -ffp-contract=fast and the vectoriser settle them: each row is
// fma(lx0, left, fl(lx1 * right)), and the two rows meet as fl(ly0 * top) + fl(ly1 * bottom), a packed multiply and
// an add, no fma.  Around the jitter's integer arithmetic the compiler pairs the operations differently, so this
// path states that form outright (empty asm keeps the products from fusing, as in mix2); the GPU tests hold the two
// to equal bits.
__device__ __forceinline__ float bilerp_as_plain(float ly0, float ly1, float lx0, float lx1, float a, float b, float d,
                                                 float e) {
  float tb = __fmul_rn(lx1, b), te = __fmul_rn(lx1, e);
  asm("" : "+v"(tb), "+v"(te));
  float top = __fmul_rn(ly0, __fmaf_rn(lx0, a, tb)), bot = __fmul_rn(ly1, __fmaf_rn(lx0, d, te));
  asm("" : "+v"(top), "+v"(bot));
  return __fadd_rn(top, bot);
}

// sample_rgb with every tap passed through jitter_px, so a clip whose three factors are all <= 0 holds sample_rgb's
// bits.
__device__ __forceinline__ void sample_rgb_jitter(const unsigned char* __restrict__ fr, int H, int W, int new_h,
                                                  int new_w, int ys, int xs, const NormArgs& nm, const JitGeo& j,
                                                  float v[3]) {
  if (new_h == H && new_w == W) {
    unsigned char p[3];
    jitter_px(fr + ((long)ys * W + xs) * 3, j, p);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = norm1(p[c], nm.m[c], nm.s[c]);
  } else {
    int ya, yb, xa, xb;
    float ly0, ly1, lx0, lx1;
    src_index((float)H / (float)new_h, ys, H, &ya, &yb, &ly0, &ly1);
    src_index((float)W / (float)new_w, xs, W, &xa, &xb, &lx0, &lx1);
    unsigned char p00[3], p01[3], p10[3], p11[3];
    jitter_px(fr + ((long)ya * W + xa) * 3, j, p00);
    jitter_px(fr + ((long)ya * W + xb) * 3, j, p01);
    jitter_px(fr + ((long)yb * W + xa) * 3, j, p10);
    jitter_px(fr + ((long)yb * W + xb) * 3, j, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = norm1(p00[c], nm.m[c], nm.s[c]), b = norm1(p01[c], nm.m[c], nm.s[c]);
      const float d = norm1(p10[c], nm.m[c], nm.s[c]), e = norm1(p11[c], nm.m[c], nm.s[c]);
      v[c] = bilerp_as_plain(ly0, ly1, lx0, lx1, a, b, d, e);
    }
  }
}

// The grey mean of every (clip, Fast frame) after the clip's brightness stage: int(ImageStat.Stat(L).mean[0] + 0.5) =
// (2 S + n) / (2 n) for the sum S of the n = H * W grey values.  One workgroup per frame (grid n_fast x B: 256 for a
// batch of 8 x 32, one per CU), each thread sums pixels in an integer register, the wavefronts meet in LDS and thread 0
// owns the output element: no atomics.  The frame starts at any byte, so the first (address % 4) pixels and the last
// (< 4) go one by one and the rest as aligned 12-byte groups of four pixels.
struct Px4 {
  unsigned w[3];
};

__device__ __forceinline__ unsigned grey_bright(float fb, int r, int g, int b) {
  int c[3] = {r, g, b};
  bright3(fb, c);
  return (unsigned)grey3(c);
}

// four pixels in three words: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
__device__ __forceinline__ unsigned grey_bright4(float fb, const Px4& w) {
  const unsigned a = w.w[0], m = w.w[1], z = w.w[2];
  return grey_bright(fb, a & 255, (a >> 8) & 255, (a >> 16) & 255) + grey_bright(fb, a >> 24, m & 255, (m >> 8) & 255) +
         grey_bright(fb, (m >> 16) & 255, m >> 24, z & 255) + grey_bright(fb, (z >> 8) & 255, (z >> 16) & 255, z >> 24);
}

__global__ void __launch_bounds__(TPB) frame_grey_means_kernel(const long* __restrict__ tab,
                                                               const long* __restrict__ frame_idx,
                                                               const long* __restrict__ jit, int n_fast, int crop,
                                                               int* __restrict__ means) {
  const int f = blockIdx.x, b = blockIdx.y;
  const ClipGeo g = batch_row(tab, b, crop);
  const JitGeo j = jitter_row(jit, b);
  int* out = means + (long)b * n_fast + f;
  if (!g.ok || !j.ok || !(j.fc > 0.f)) {  // no contrast stage (or no valid row): nothing is read
    if (threadIdx.x == 0) *out = 0;
    return;
  }
  const unsigned char* fr = batch_frame(g, frame_idx, b, n_fast, f, 3);
  const long n = (long)g.H * g.W;
  long head = (long)((unsigned long)fr & 3);  // base + 3 * head is 4-byte aligned: 3 h = -a (mod 4) <=> h = a
  if (head > n) head = n;
  const long groups = (n - head) / 4;
  const long rest = head + groups * 4;  // first pixel of the tail
  unsigned long acc = 0;
  for (long i = threadIdx.x; i < head + (n - rest); i += TPB) {
    const unsigned char* p = fr + (i < head ? i : rest + (i - head)) * 3;
    acc += grey_bright(j.fb, p[0], p[1], p[2]);
  }
  const auto* q = (const __attribute__((address_space(1))) unsigned*)(unsigned long)(fr + head * 3);
  const auto load4 = [q](long i) { return Px4{{q[3 * i], q[3 * i + 1], q[3 * i + 2]}}; };
  long i = threadIdx.x;
  for (; i + 3 * TPB < groups; i += 4 * TPB) {  // four loads in flight per thread
    const Px4 w0 = load4(i), w1 = load4(i + TPB), w2 = load4(i + 2 * TPB), w3 = load4(i + 3 * TPB);
    acc += grey_bright4(j.fb, w0) + grey_bright4(j.fb, w1) + grey_bright4(j.fb, w2) + grey_bright4(j.fb, w3);
  }
  for (; i < groups; i += TPB) acc += grey_bright4(j.fb, load4(i));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  __shared__ unsigned long part[TPB / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long S = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) S += part[w];
    const unsigned long un = (unsigned long)n;
    *out = (int)(S / un + (2 * (S % un) >= un ? 1 : 0));  // (2 S + n) / (2 n) without the doubled sum
  }
}

// clip_batch_kernel with the jitter in every tap: grid, ownership, borders and stores are its own.
__global__ void clip_batch_jitter_kernel(const long* __restrict__ tab, const long* __restrict__ frame_idx,
                                         const long* __restrict__ slow_idx, const long* __restrict__ jit,
                                         const int* __restrict__ means, int n_fast, int n_slow, int crop, int reverse,
                                         NormArgs nm, float* __restrict__ fast, float* __restrict__ slow, int ph, int pw,
                                         int Wp, int plane) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= plane) return;
  const int f = blockIdx.y, b = blockIdx.z;
  const ClipGeo g = batch_row(tab, b, crop);
  JitGeo j = jitter_row(jit, b);
  const int yp = p / Wp, xp = p - yp * Wp;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  const int yy = yp - ph, xx = xp - pw;
  if (g.ok && j.ok && yy >= 0 && yy < crop && xx >= 0 && xx < crop) {
    j.m = means[(long)b * n_fast + f];
    const int ys = g.y0 + yy;
    const int xs = g.x0 + (g.flip ? crop - 1 - xx : xx);
    float c[3];
    sample_rgb_jitter(batch_frame(g, frame_idx, b, n_fast, f, 3), g.H, g.W, g.new_h, g.new_w, ys, xs, nm, j, c);
    if (reverse) {
      o[0] = c[2]; o[1] = c[1]; o[2] = c[0];
    } else {
      o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    }
  }
  *reinterpret_cast<f32x4*>(fast + (((long)b * n_fast + f) * plane + p) * 4) = o;
  for (int k = 0; k < n_slow; ++k)  // n_slow <= n_fast / alpha entries, wave-uniform
    if (slow_idx[k] == f) *reinterpret_cast<f32x4*>(slow + (((long)b * n_slow + k) * plane + p) * 4) = o;
}

// Host-side check of the jitter rows behind a batch table: [B][SF_JITTER_ROW] after the Slow positions.
bool jitter_table_ok(const long* tab, int B, int n_fast, int n_slow) {
  const long* jit = tab + (long)B * (BATCH_ROW + n_fast) + n_slow;
  for (int b = 0; b < B; ++b)
    if (!jitter_row_ok(jit + (long)b * JITTER_ROW)) return false;
  return true;
}

bool means_ok(const int* means) { return means && (uintptr_t)means % sizeof(int) == 0; }

void launch_grey_means(const long* table, int B, int n_fast, int n_slow, int crop, int* means, hipStream_t stream) {
  const long* frame_idx = table + (long)B * BATCH_ROW;
  hipLaunchKernelGGL(frame_grey_means_kernel, dim3(n_fast, B), dim3(TPB), 0, stream, table, frame_idx,
                     frame_idx + (long)B * n_fast + n_slow, n_fast, crop, means);
}
// ---- all B clips of one DETECTION batch (AVA, `AVA.IMG_PROC_BACKEND == "pytorch"`), both pathways, in ONE launch
// (datasets/ava_dataset.py:233-338 per sample; datasets/loader.py:18-52 collates).  The grid, the table idea, the Slow
// search and the one-owner stores are clip_batch_kernel's; the pixel arithmetic is NOT sample_rgb's, because the AVA
// loader orders it differently: u / 255 per tap, resample the unnormalised image, crop and flip, add the PCA-lighting
// offset (transform.py:636-663), then (. - mean) / std (:666-688), and only then BGR -> RGB.  The output window is
// win_h x win_w (the `test` split takes no crop: the window is the whole scaled frame and need not be square).
constexpr int DET_ROW = 12;  // clip address, T, H, W, new_h, new_w, y0, x0, flip, three lighting offsets (float32 bits)

struct DetGeo {
  const unsigned char* clip;
  int T, H, W, new_h, new_w, y0, x0, flip, ok;
  float off[3];
};

// One row's check, shared by the host entry and the kernel, as batch_row_ok with a rectangular window.
__host__ __device__ __forceinline__ bool det_row_ok(const long* r, int win_h, int win_w) {
  const long lim = 0x7fffffffL;
  return r[0] != 0 && r[1] > 0 && r[1] <= lim && r[2] > 0 && r[2] <= lim && r[3] > 0 && r[3] <= lim && r[4] > 0 &&
         r[4] <= lim && r[5] > 0 && r[5] <= lim && r[6] >= 0 && r[6] <= lim && r[7] >= 0 && r[7] <= lim &&
         r[6] + win_h <= r[4] && r[7] + win_w <= r[5];
}

__device__ __forceinline__ DetGeo det_row(const long* __restrict__ tab, int b, int win_h, int win_w) {
  const long* r = tab + (long)b * DET_ROW;
  DetGeo g;
  g.clip = (const unsigned char*)(const __attribute__((address_space(1))) unsigned char*)(unsigned long)r[0];
  g.T = (int)r[1]; g.H = (int)r[2]; g.W = (int)r[3];
  g.new_h = (int)r[4]; g.new_w = (int)r[5]; g.y0 = (int)r[6]; g.x0 = (int)r[7];
  g.flip = r[8] != 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) g.off[c] = __uint_as_float((unsigned)r[9 + c]);
  g.ok = det_row_ok(r, win_h, win_w);
  return g;
}

__device__ __forceinline__ float unit1(unsigned char u) { return __fdiv_rn((float)u, 255.f); }  // imgs / 255.0 (:247-248)

// The value of the scaled, lit and normalised frame at (ys, xs), three channels in source (BGR) order; mean, std and
// the offsets are indexed in that order too.
__device__ __forceinline__ void sample_det(const unsigned char* __restrict__ fr, int H, int W, int new_h, int new_w,
                                           int ys, int xs, const NormArgs& nm, const float off[3], float v[3]) {
  float r[3];
  if (new_h == H && new_w == W) {
    const unsigned char* p = fr + ((long)ys * W + xs) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = unit1(p[c]);
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
    for (int c = 0; c < 3; ++c)
      r[c] = ly0 * (lx0 * unit1(p00[c]) + lx1 * unit1(p01[c])) + ly1 * (lx0 * unit1(p10[c]) + lx1 * unit1(p11[c]));
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn((r[c] + off[c]) - nm.m[c], nm.s[c]);
}

__global__ void clip_batch_det_kernel(const long* __restrict__ tab, const long* __restrict__ frame_idx,
                                      const long* __restrict__ slow_idx, int n_fast, int n_slow, int win_h, int win_w,
                                      int reverse, NormArgs nm, float* __restrict__ fast, float* __restrict__ slow, int ph,
                                      int pw, int Wp, int plane) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= plane) return;
  const int f = blockIdx.y, b = blockIdx.z;
  const DetGeo g = det_row(tab, b, win_h, win_w);
  const int yp = p / Wp, xp = p - yp * Wp;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  const int yy = yp - ph, xx = xp - pw;
  if (g.ok && yy >= 0 && yy < win_h && xx >= 0 && xx < win_w) {
    const long ft = frame_idx[(long)b * n_fast + f];
    const int t = ft < 0 ? 0 : (ft > g.T - 1 ? g.T - 1 : (int)ft);  // clamped into [0, T_i)
    const int ys = g.y0 + yy;
    const int xs = g.x0 + (g.flip ? win_w - 1 - xx : xx);  // flip is applied after the crop
    float c[3];
    sample_det(g.clip + (long)t * g.H * g.W * 3, g.H, g.W, g.new_h, g.new_w, ys, xs, nm, g.off, c);
    if (reverse) {  // AVA.BGR False: imgs[:, [2, 1, 0]] (:329-332)
      o[0] = c[2]; o[1] = c[1]; o[2] = c[0];
    } else {
      o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    }
  }
  *reinterpret_cast<f32x4*>(fast + (((long)b * n_fast + f) * plane + p) * 4) = o;
  for (int j = 0; j < n_slow; ++j)  // n_slow <= n_fast / alpha entries, wave-uniform
    if (slow_idx[j] == f) *reinterpret_cast<f32x4*>(slow + (((long)b * n_slow + j) * plane + p) * 4) = o;
}

// Host-side check of the detection table's host copy: rows [B][12], then frame indices [B][n_fast], then n_slow Slow
// positions.  A lighting offset must be a finite float32.
bool det_table_ok(const long* tab, int B, int n_fast, int n_slow, int win_h, int win_w) {
  for (int b = 0; b < B; ++b) {
    const long* r = tab + (long)b * DET_ROW;
    if (!det_row_ok(r, win_h, win_w)) return false;
    for (int c = 0; c < 3; ++c)
      if (r[9 + c] < 0 || r[9 + c] > 0xffffffffL || ((unsigned)r[9 + c] & 0x7f800000u) == 0x7f800000u) return false;
  }
  const long* fi = tab + (long)B * DET_ROW;
  for (int b = 0; b < B; ++b) {
    const long T = tab[(long)b * DET_ROW + 1];
    for (int f = 0; f < n_fast; ++f)
      if (fi[(long)b * n_fast + f] < 0 || fi[(long)b * n_fast + f] >= T) return false;
  }
  const long* si = fi + (long)B * n_fast;
  for (int j = 0; j < n_slow; ++j)
    if (si[j] < 0 || si[j] >= n_fast || (j > 0 && si[j] <= si[j - 1])) return false;  // distinct: one owner per Slow frame
  return true;
}
}  // namespace

extern "C" int sf_clip_prologue(const unsigned char* clip, int T, int H, int W, int new_h, int new_w, int y0, int x0,
                                int crop, int flip, int reverse, const float* mean3, const float* std3,
                                const int* frame_idx, int n_frames, float* dst, int ph, int pw, int Wp, void* stream) {
  if (!clip || !dst || !mean3 || !std3 || T <= 0 || H <= 0 || W <= 0 || new_h <= 0 || new_w <= 0 || crop <= 0 ||
      n_frames <= 0 || ph < 0 || pw < 0)
    return SF_EINVAL;
  if (y0 < 0 || x0 < 0 || y0 + crop > new_h || x0 + crop > new_w || Wp < crop + 2 * pw) return SF_EINVAL;
  if (!frame_idx && n_frames != T) return SF_EINVAL;
  if (!sf_aligned16(dst)) return SF_EINVAL;
  NormArgs nm;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean3[c];   // HOST pointers: three floats each
    nm.s[c] = std3[c];
  }
  const long total = (long)n_frames * (crop + 2 * ph) * Wp;
  hipLaunchKernelGGL(clip_prologue_kernel, dim3(sf_cdiv(total, TPB)), dim3(TPB), 0, (hipStream_t)stream, clip, T, H, W,
                     new_h, new_w, y0, x0, crop, flip, reverse, nm, frame_idx, n_frames, dst, ph, pw, Wp, total);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_clip_prologue_gray(const unsigned char* clip, int T, int H, int W, int new_h, int new_w, int y0,
                                     int x0, int crop, int flip, float mean, float stdv, const int* frame_idx,
                                     int n_frames, float* dst, int ph, int pw, int Wp, void* stream) {
  if (!clip || !dst || T <= 0 || H <= 0 || W <= 0 || new_h <= 0 || new_w <= 0 || crop <= 0 || n_frames <= 0 || ph < 0 ||
      pw < 0)
    return SF_EINVAL;
  if (y0 < 0 || x0 < 0 || y0 + crop > new_h || x0 + crop > new_w || Wp < crop + 2 * pw) return SF_EINVAL;
  if (!frame_idx && n_frames != T) return SF_EINVAL;
  const long total = (long)n_frames * (crop + 2 * ph) * Wp;
  hipLaunchKernelGGL(clip_prologue_gray_kernel, dim3(sf_cdiv(total, TPB)), dim3(TPB), 0, (hipStream_t)stream, clip, T, H,
                     W, new_h, new_w, y0, x0, crop, flip, mean, stdv, frame_idx, n_frames, dst, ph, pw, Wp, total);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_clip_views(const unsigned char* video, int T, int H, int W, const int* table_host, const int* table,
                             int V, int n_fast, int n_slow, int crop, int reverse, const float* mean3,
                             const float* std3, float* fast, float* slow, int ph, int pw, int Wp, void* stream) {
  long plane = 0;
  if (!mean3 || !std3 ||
      !clip_views_args_ok(video, T, H, W, table_host, table, V, n_fast, n_slow, crop, fast, slow, ph, pw, Wp, &plane))
    return SF_EINVAL;
  if (!sf_aligned16(fast) || !sf_aligned16(slow)) return SF_EINVAL;
  NormArgs nm;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean3[c];   // HOST pointers: three floats each
    nm.s[c] = std3[c];
  }
  const int* frame_idx = table + (long)V * VIEW_ROW;
  hipLaunchKernelGGL(clip_views_kernel, dim3(sf_cdiv(plane, TPB), n_fast, V), dim3(TPB), 0, (hipStream_t)stream, video, T,
                     H, W, table, frame_idx, frame_idx + (long)V * n_fast, n_fast, n_slow, crop, reverse, nm, fast, slow,
                     ph, pw, Wp, (int)plane);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_clip_views_gray(const unsigned char* video, int T, int H, int W, const int* table_host,
                                  const int* table, int V, int n_fast, int n_slow, int crop, float mean, float stdv,
                                  float* fast, float* slow, int ph, int pw, int Wp, void* stream) {
  long plane = 0;
  if (!clip_views_args_ok(video, T, H, W, table_host, table, V, n_fast, n_slow, crop, fast, slow, ph, pw, Wp, &plane))
    return SF_EINVAL;
  const int* frame_idx = table + (long)V * VIEW_ROW;
  const int* slow_idx = frame_idx + (long)V * n_fast;
  if (Wp % 4 == 0 && sf_aligned16(fast) && sf_aligned16(slow)) {
    hipLaunchKernelGGL(clip_views_gray_kernel<4>, dim3(sf_cdiv(plane / 4, TPB), n_fast, V), dim3(TPB), 0,
                       (hipStream_t)stream, video, T, H, W, table, frame_idx, slow_idx, n_fast, n_slow, crop, mean, stdv,
                       fast, slow, ph, pw, Wp, (int)(plane / 4));
  } else {
    hipLaunchKernelGGL(clip_views_gray_kernel<1>, dim3(sf_cdiv(plane, TPB), n_fast, V), dim3(TPB), 0,
                       (hipStream_t)stream, video, T, H, W, table, frame_idx, slow_idx, n_fast, n_slow, crop, mean, stdv,
                       fast, slow, ph, pw, Wp, (int)plane);
  }
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_clip_batch(const long* table_host, const long* table, int B, int n_fast, int n_slow, int crop,
                             int reverse, const float* mean3, const float* std3, float* fast, float* slow, int ph,
                             int pw, int Wp, void* stream) {
  long plane = 0;
  if (!mean3 || !std3 ||
      !clip_batch_args_ok(table_host, table, B, n_fast, n_slow, crop, fast, slow, ph, pw, Wp, &plane))
    return SF_EINVAL;
  if (!sf_aligned16(fast) || !sf_aligned16(slow)) return SF_EINVAL;
  NormArgs nm;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean3[c];   // HOST pointers: three floats each
    nm.s[c] = std3[c];
  }
  const long* frame_idx = table + (long)B * BATCH_ROW;
  hipLaunchKernelGGL(clip_batch_kernel, dim3(sf_cdiv(plane, TPB), n_fast, B), dim3(TPB), 0, (hipStream_t)stream, table,
                     frame_idx, frame_idx + (long)B * n_fast, n_fast, n_slow, crop, reverse, nm, fast, slow, ph, pw, Wp,
                     (int)plane);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_clip_batch_gray(const long* table_host, const long* table, int B, int n_fast, int n_slow, int crop,
                                  float mean, float stdv, float* fast, float* slow, int ph, int pw, int Wp,
                                  void* stream) {
  long plane = 0;
  if (!clip_batch_args_ok(table_host, table, B, n_fast, n_slow, crop, fast, slow, ph, pw, Wp, &plane)) return SF_EINVAL;
  if (((uintptr_t)fast | (uintptr_t)slow) % sizeof(float)) return SF_EINVAL;  // not even a float's alignment
  const long* frame_idx = table + (long)B * BATCH_ROW;
  const long* slow_idx = frame_idx + (long)B * n_fast;
  if (Wp % 4 == 0 && sf_aligned16(fast) && sf_aligned16(slow)) {
    hipLaunchKernelGGL(clip_batch_gray_kernel<4>, dim3(sf_cdiv(plane / 4, TPB), n_fast, B), dim3(TPB), 0,
                       (hipStream_t)stream, table, frame_idx, slow_idx, n_fast, n_slow, crop, mean, stdv, fast, slow, ph,
                       pw, Wp, (int)(plane / 4));
  } else {
    hipLaunchKernelGGL(clip_batch_gray_kernel<1>, dim3(sf_cdiv(plane, TPB), n_fast, B), dim3(TPB), 0,
                       (hipStream_t)stream, table, frame_idx, slow_idx, n_fast, n_slow, crop, mean, stdv, fast, slow, ph,
                       pw, Wp, (int)plane);
  }
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_clip_batch_mix(const long* table_host, const long* table, int B, int n_fast, int n_slow, int crop,
                                 int reverse, const float* mean3, const float* std3, float* fast, float* slow, int ph,
                                 int pw, int Wp, void* stream) {
  long plane = 0;
  if (!mean3 || !std3 ||
      !clip_batch_args_ok(table_host, table, B, n_fast, n_slow, crop, fast, slow, ph, pw, Wp, &plane))
    return SF_EINVAL;
  if (!mix_table_ok(table_host, B, n_fast, n_slow, crop)) return SF_EINVAL;
  if (!sf_aligned16(fast) || !sf_aligned16(slow)) return SF_EINVAL;
  NormArgs nm;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean3[c];   // HOST pointers: three floats each
    nm.s[c] = std3[c];
  }
  const long* frame_idx = table + (long)B * BATCH_ROW;
  const long* slow_idx = frame_idx + (long)B * n_fast;
  hipLaunchKernelGGL(clip_batch_mix_kernel, dim3(sf_cdiv(plane, TPB), n_fast, B), dim3(TPB), 0, (hipStream_t)stream,
                     table, frame_idx, slow_idx, slow_idx + n_slow, B, n_fast, n_slow, crop, reverse, nm, fast, slow, ph,
                     pw, Wp, (int)plane);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_clip_batch_mix_gray(const long* table_host, const long* table, int B, int n_fast, int n_slow, int crop,
                                      float mean, float stdv, float* fast, float* slow, int ph, int pw, int Wp,
                                      void* stream) {
  long plane = 0;
  if (!clip_batch_args_ok(table_host, table, B, n_fast, n_slow, crop, fast, slow, ph, pw, Wp, &plane)) return SF_EINVAL;
  if (!mix_table_ok(table_host, B, n_fast, n_slow, crop)) return SF_EINVAL;
  if (((uintptr_t)fast | (uintptr_t)slow) % sizeof(float)) return SF_EINVAL;  // not even a float's alignment
  const long* frame_idx = table + (long)B * BATCH_ROW;
  const long* slow_idx = frame_idx + (long)B * n_fast;
  const long* mix = slow_idx + n_slow;
  if (Wp % 4 == 0 && sf_aligned16(fast) && sf_aligned16(slow)) {
    hipLaunchKernelGGL(clip_batch_mix_gray_kernel<4>, dim3(sf_cdiv(plane / 4, TPB), n_fast, B), dim3(TPB), 0,
                       (hipStream_t)stream, table, frame_idx, slow_idx, mix, B, n_fast, n_slow, crop, mean, stdv, fast,
                       slow, ph, pw, Wp, (int)(plane / 4));
  } else {
    hipLaunchKernelGGL(clip_batch_mix_gray_kernel<1>, dim3(sf_cdiv(plane, TPB), n_fast, B), dim3(TPB), 0,
                       (hipStream_t)stream, table, frame_idx, slow_idx, mix, B, n_fast, n_slow, crop, mean, stdv, fast,
                       slow, ph, pw, Wp, (int)plane);
  }
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_frame_grey_means(const long* table_host, const long* table, int B, int n_fast, int n_slow, int* means,
                                   void* stream) {
  if (!table_host || !table || !means_ok(means) || B <= 0 || n_fast <= 0 || n_slow < 0 || n_slow > n_fast || B > 65535 ||
      n_fast > 65535)
    return SF_EINVAL;
  // crop 0: the means read whole frames, there is no window to place
  if (!batch_table_ok(table_host, B, n_fast, n_slow, 0) || !jitter_table_ok(table_host, B, n_fast, n_slow))
    return SF_EINVAL;
  launch_grey_means(table, B, n_fast, n_slow, 0, means, (hipStream_t)stream);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_clip_batch_jitter(const long* table_host, const long* table, int B, int n_fast, int n_slow, int crop,
                                    int reverse, const float* mean3, const float* std3, int* means, float* fast,
                                    float* slow, int ph, int pw, int Wp, void* stream) {
  long plane = 0;
  if (!mean3 || !std3 ||
      !clip_batch_args_ok(table_host, table, B, n_fast, n_slow, crop, fast, slow, ph, pw, Wp, &plane))
    return SF_EINVAL;
  if (!means_ok(means) || !jitter_table_ok(table_host, B, n_fast, n_slow)) return SF_EINVAL;
  if (!sf_aligned16(fast) || !sf_aligned16(slow)) return SF_EINVAL;
  NormArgs nm;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean3[c];   // HOST pointers: three floats each
    nm.s[c] = std3[c];
  }
  launch_grey_means(table, B, n_fast, n_slow, crop, means, (hipStream_t)stream);
  SF_CHECK_LAUNCH();
  const long* frame_idx = table + (long)B * BATCH_ROW;
  const long* slow_idx = frame_idx + (long)B * n_fast;
  hipLaunchKernelGGL(clip_batch_jitter_kernel, dim3(sf_cdiv(plane, TPB), n_fast, B), dim3(TPB), 0, (hipStream_t)stream,
                     table, frame_idx, slow_idx, slow_idx + n_slow, means, n_fast, n_slow, crop, reverse, nm, fast, slow,
                     ph, pw, Wp, (int)plane);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_clip_batch_det(const long* table_host, const long* table, int B, int n_fast, int n_slow, int win_h,
                                 int win_w, int reverse, const float* mean3, const float* std3, float* fast,
                                 float* slow, int ph, int pw, int Wp, void* stream) {
  if (!table_host || !table || !fast || !mean3 || !std3 || B <= 0 || n_fast <= 0 || win_h <= 0 || win_w <= 0 || ph < 0 ||
      pw < 0)
    return SF_EINVAL;
  if (n_slow < 0 || n_slow > n_fast || (slow == nullptr) != (n_slow == 0)) return SF_EINVAL;
  if (B > 65535 || n_fast > 65535 || (long)Wp < (long)win_w + 2L * pw) return SF_EINVAL;
  const long plane = ((long)win_h + 2L * ph) * Wp;
  if (plane > 0x7fffffffL / 4) return SF_EINVAL;
  if (!det_table_ok(table_host, B, n_fast, n_slow, win_h, win_w)) return SF_EINVAL;
  if (!sf_aligned16(fast) || !sf_aligned16(slow)) return SF_EINVAL;
  NormArgs nm;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean3[c];   // HOST pointers: three floats each, in source (BGR) order
    nm.s[c] = std3[c];
  }
  const long* frame_idx = table + (long)B * DET_ROW;
  hipLaunchKernelGGL(clip_batch_det_kernel, dim3(sf_cdiv(plane, TPB), n_fast, B), dim3(TPB), 0, (hipStream_t)stream,
                     table, frame_idx, frame_idx + (long)B * n_fast, n_fast, n_slow, win_h, win_w, reverse, nm, fast, slow,
                     ph, pw, Wp, (int)plane);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
