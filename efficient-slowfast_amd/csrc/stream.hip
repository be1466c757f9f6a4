// stream.hip — the streaming demo (tools/demo_net.py:160-305) with its frame buffer on the device.
//
// Reference (host, per incoming frame once the buffer is full): torch.as_tensor over all S = NUM_FRAMES * SAMPLING_RATE
// scaled frames, tensor_normalize of all of them, permute, two index_selects, a float host-to-device copy of both
// pathways, the forward, torch.nonzero(preds > 0.1).cpu().  Only the newest frame is new.  Here the S scaled and
// normalised frames live in a device ring in the stem's PackedClip layout (channels padded to 4, zero borders, row
// pitch Wp):
//   sf_stream_push    one uint8 camera frame -> one ring slot   (3 B read per tap, 16 B written per pixel: HBM-bound)
//   sf_stream_window  ring -> both pathways' input buffers      (16 B read + 16 B (+16 B) written per pixel: HBM-bound)
//   sf_label_select   the forward's probabilities -> label ids  (one wavefront per row, 4 B read per class)
#include "clip_sample.h"

namespace {
constexpr int TPB = 256;

// One destination pixel of the padded plane per thread, one 16-byte store: the whole plane is written, zeros
// included, so a slot never keeps a stale element of the frame it held S pushes ago.  The arithmetic is sample_rgb's
// (the bits of clip_prologue_kernel with its window on the whole scaled frame).  The camera's frame is BGR: it is
// sampled in its own order — `nm` holds mean / std in that order — and channel 2 - c of the read lands in channel c.
__global__ void stream_push_kernel(const unsigned char* __restrict__ frame, int H, int W, int new_h, int new_w,
                                   NormArgs nm, float* __restrict__ dst, int ph, int pw, int Wp, int plane) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= plane) return;
  const int yp = p / Wp, xp = p - yp * Wp;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  const int yy = yp - ph, xx = xp - pw;
  if (yy >= 0 && yy < new_h && xx >= 0 && xx < new_w) {
    float v[3];
    sample_rgb(frame, H, W, new_h, new_w, yy, xx, nm, v);
    o[0] = v[2]; o[1] = v[1]; o[2] = v[0];
  }
  *reinterpret_cast<f32x4*>(dst + (long)p * 4) = o;
}

// Grid (plane pixels, Fast frame), as clip_views_kernel: the frame's window position, its slot and the "is this Fast
// frame also a Slow frame" search are uniform per workgroup (scalar loads); a thread moves one 16-byte element.  A
// window position outside [0, S) yields zeros, never a read.  Slow frame j belongs to the workgroups of Fast frame
// sidx[j]; when sidx[j] names no Fast frame, the workgroups of Fast frame j (j < n_slow <= n_fast) write it as zeros,
// so every element of both buffers has exactly one owner whatever the tables hold.
__global__ void stream_window_kernel(const float* __restrict__ ring, int S, int head, const int* __restrict__ fidx,
                                     const int* __restrict__ sidx, int n_fast, int n_slow, float* __restrict__ fast,
                                     float* __restrict__ slow, int plane) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= plane) return;
  const int f = blockIdx.y;
  const int w = fidx[f];
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (w >= 0 && w < S) {
    const int slot = (head + w) % S;  // head in [0, S): checked by the entry
    o = *reinterpret_cast<const f32x4*>(ring + ((long)slot * plane + p) * 4);
  }
  *reinterpret_cast<f32x4*>(fast + ((long)f * plane + p) * 4) = o;
  for (int j = 0; j < n_slow; ++j) {  // n_slow <= n_fast / alpha entries, wave-uniform
    const int sj = sidx[j];
    if (sj == f) {
      *reinterpret_cast<f32x4*>(slow + ((long)j * plane + p) * 4) = o;
    } else if ((sj < 0 || sj >= n_fast) && j == f) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(slow + ((long)j * plane + p) * 4) = z;
    }
  }
}

// One wavefront per row, 64 classes per step.  The lanes that select their class form a ballot; a lane's position
// among them (popcount of the ballot below the lane) plus the running count is where its id goes, so the ids come out
// in ascending order with no atomics and no LDS.  The argmax keeps, per lane, the first strictly larger value (a lane's
// classes ascend), and the lanes meet in a butterfly where the larger value wins and equal values give way to the
// smaller index: torch.argmax's first maximal index.  A NaN compares false everywhere: never selected, never a winner.
__global__ void __launch_bounds__(TPB) label_select_kernel(const float* __restrict__ preds, int R, int C, float thr,
                                                           int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (row >= R) return;  // wave-uniform
  const float* p = preds + (long)row * C;
  int* o = out + (long)row * (2 + C);
  const unsigned long long below = (1ull << lane) - 1ull;
  int count = 0, bidx = -1;
  float best = 0.f;
  for (int base = 0; base < C; base += 64) {
    const int c = base + lane;
    const bool in = c < C;
    const float v = in ? p[c] : 0.f;
    const bool sel = in && v > thr;
    const unsigned long long m = __ballot(sel);
    if (sel) o[2 + count + __popcll(m & below)] = c;
    count += __popcll(m);
    if (in && v == v && (bidx < 0 || v > best)) {
      best = v;
      bidx = c;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off);
    const int oi = __shfl_xor(bidx, off);
    if (oi >= 0 && (bidx < 0 || ov > best || (ov == best && oi < bidx))) {
      best = ov;
      bidx = oi;
    }
  }
  if (lane == 0) {
    o[0] = count;
    o[1] = bidx;
  }
}

// (new_h + 2 ph) * Wp pixels of one padded plane, or 0 when the geometry is not one the kernels index in 32 bits
long plane_of(int new_h, int new_w, int ph, int pw, int Wp) {
  if (new_h <= 0 || new_w <= 0 || ph < 0 || pw < 0 || (long)Wp < (long)new_w + 2L * pw) return 0;
  const long plane = ((long)new_h + 2L * ph) * Wp;
  return plane > 0x7fffffffL / 4 ? 0 : plane;
}
}  // namespace

extern "C" int sf_stream_push(const unsigned char* frame, int H, int W, int new_h, int new_w, const float* mean3,
                              const float* std3, float* ring, int S, int slot, int ph, int pw, int Wp, void* stream) {
  if (!frame || !ring || !mean3 || !std3 || H <= 0 || W <= 0 || S <= 0 || slot < 0 || slot >= S) return SF_EINVAL;
  const long plane = plane_of(new_h, new_w, ph, pw, Wp);
  if (plane == 0 || (long)H * W > 0x7fffffffL / 3) return SF_EINVAL;
  if (!sf_aligned16(ring)) return SF_EINVAL;
  NormArgs nm;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean3[2 - c];   // HOST pointers: three floats each in RGB order (DATA.MEAN / DATA.STD); the frame is BGR
    nm.s[c] = std3[2 - c];
  }
  hipLaunchKernelGGL(stream_push_kernel, dim3(sf_cdiv(plane, TPB)), dim3(TPB), 0, (hipStream_t)stream, frame, H, W, new_h,
                     new_w, nm, ring + (long)slot * plane * 4, ph, pw, Wp, (int)plane);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_stream_window(const float* ring, int S, int head, const int* fast_idx, int n_fast, const int* slow_idx,
                                int n_slow, float* fast, float* slow, int Hp, int Wp, void* stream) {
  if (!ring || !fast_idx || !fast || S <= 0 || head < 0 || head >= S || n_fast <= 0 || n_fast > 65535 || Hp <= 0 ||
      Wp <= 0)
    return SF_EINVAL;
  if (n_slow < 0 || n_slow > n_fast || (slow == nullptr) != (n_slow == 0) || (n_slow > 0 && !slow_idx)) return SF_EINVAL;
  const long plane = (long)Hp * Wp;
  if (plane > 0x7fffffffL / 4) return SF_EINVAL;
  if (!sf_aligned16(ring) || !sf_aligned16(fast) || !sf_aligned16(slow)) return SF_EINVAL;
  hipLaunchKernelGGL(stream_window_kernel, dim3(sf_cdiv(plane, TPB), n_fast), dim3(TPB), 0, (hipStream_t)stream, ring, S,
                     head, fast_idx, slow_idx, n_fast, n_slow, fast, slow, (int)plane);
  SF_CHECK_LAUNCH();
  return SF_OK;
}

extern "C" int sf_label_select(const float* preds, int R, int C, float thr, int* out, void* stream) {
  if (!preds || !out || R <= 0 || C <= 0 || C > 0x7fffffff - 64 || !(thr == thr)) return SF_EINVAL;
  if (((uintptr_t)preds | (uintptr_t)out) % 4) return SF_EINVAL;
  hipLaunchKernelGGL(label_select_kernel, dim3(sf_cdiv(R, TPB / 64)), dim3(TPB), 0, (hipStream_t)stream, preds, R, C, thr,
                     out);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
