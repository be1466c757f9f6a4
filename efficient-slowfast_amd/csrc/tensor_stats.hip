// tensor_stats.hip — what a run's watcher asks of every parameter or gradient (the reference's TensorboardWriter,
// TENSORBOARD.MODEL_VIS: which layer went dead, which gradient vanished, where the first Inf appeared) in ONE call of
// two launches, addressed like sf_grad_norm: an int64 table of (address, numel) rows and the (tensor, first element)
// chunk list tiled at sf_sgd_chunk_elems(), so a tensor's chunks are contiguous.  An address of 0 is a tensor that is
// absent (a parameter whose .grad is still None): its row is all zeros, present = 0.
//   launch 1   one workgroup per chunk reads its span once, in chunk_table.h's fixed order (span_reduce, then block_fold
//              for the fp64 sums), counts the sign-and-exponent histogram, NaN, Inf and zero elements with integer LDS
//              adds, takes min / max with integer LDS min / max on ordered keys, and leaves one workspace row per chunk.
//   launch 2   one workgroup per tensor folds that tensor's chunk rows in chunk order and writes the tensor's row into
//              slot `cursor` of a ring in device memory; workgroup 0 advances the cursor.
// No float atomics, no "last workgroup" finish, no memset: every word of a row has one writer and equal inputs give equal
// bits.  Nothing needs the host, so the call replays inside a captured graph; the ring is read once per logging period.
// The row (include/sfhip.h, SF_TSTATS_*), in 8-byte slots:
//   [0] present  [1] numel  [2] n_nan  [3] n_inf  [4] n_zero (int64)   [5] {min, max}  [6] {absmax, 0} (fp32 pairs)
//   [7] sum  [8] sumsq (fp64, finite elements)   [9 .. 9 + 2 B] hist (int64), B = 24 exponent bins per sign + a centre bin
#include "chunk_table.h"
#include "common.h"

#include <math.h>

namespace {
constexpr int TS_TAB_ROW = 2;  // address (0: absent), numel
constexpr int TS_B = SF_TSTATS_BINS;
constexpr int TS_HIST = 2 * TS_B + 1;  // 49 histogram bins, most negative first
constexpr int TS_ROW = SF_TSTATS_ROW;
constexpr int TS_EXP_LO = 127 - 20;  // the biased exponent of 2^-20: everything below goes to the centre bin
// The count columns a chunk leaves: the 49 bins, then NaN, Inf, zero.  Every element adds to exactly ONE of the first 51.
constexpr int COL_NAN = TS_HIST, COL_INF = TS_HIST + 1, COL_ZERO = TS_HIST + 2, TS_COLS = TS_HIST + 3;
// The counters in LDS: 32 copies of the columns, a thread uses copy threadIdx.x & 31.  Copy c of column k sits at word
// k * TS_COPIES + c, so the 32 lanes of a half wavefront — the only lanes that can conflict (MI355X_MICROARCH.md, LDS: a
// 4-byte access is banked by (a / 4) mod 32 within each group of 32 lanes of ONE instruction) — fall on 32 different
// banks whatever their elements are: no add waits for another, however peaked the histogram.  Eight threads of the
// workgroup (two per wavefront, in different halves) share a copy; the adds are atomics, so that is correct.
// Two more columns hold the chunk's min and max as ordered keys (below), folded by integer LDS min / max.
constexpr int TS_COPIES = 32;
constexpr int COL_MIN = TS_COLS, COL_MAX = TS_COLS + 1, TS_LDS_COLS = TS_COLS + 2;
static_assert(TS_LDS_COLS * 4 <= CHUNK_TPB, "four threads fold a column");
// A chunk's workspace row, in 8-byte words: sum, sumsq, {min, max}, then the 52 columns as int32 (a chunk has at most
// 4096 elements).  The workspace: 2 words (the ring slot of this call, unused), n_chunks words (per TENSOR: the index of
// its first chunk; a tensor has at least one chunk), n_chunks rows.
constexpr int WS_ROW = 3 + TS_COLS / 2, WS_HEAD = 2;
static_assert(TS_COLS % 2 == 0 && TS_COLS <= 64, "the columns fill whole words and fit one wavefront");

struct Acc {  // what a thread carries over its elements
  double s, ss;
  float mn, mx;
  unsigned nz;
};
struct Elem {  // span_reduce's step
  unsigned* h;  // this thread's copy of column 0
  __device__ __forceinline__ Acc operator()(Acc a, float x) const {
    const unsigned u = __float_as_uint(x), mag = u & 0x7fffffffu, e = mag >> 23;
    if (__builtin_expect(e == 255u, 0)) {  // a NaN or an Inf: counted, in no bin, in no sum (rare: off the main path)
      atomicAdd(h + (mag > 0x7f800000u ? COL_NAN : COL_INF) * TS_COPIES, 1u);
      return a;
    }
    // floor(log2 |x|) + 20 from the exponent field (a denormal has e = 0): c = clamp(e, 2^-21's, 2^3's) is the centre
    // bin at its low end and the last bin at its high end; the bins of the negative side run from the largest magnitude
    // to the smallest, so the 49 bins have increasing limits
    const int c = (int)min(max(e, (unsigned)(TS_EXP_LO - 1)), (unsigned)(TS_EXP_LO + TS_B - 1));
    const int col = (u >> 31) != 0u ? TS_EXP_LO + TS_B - 1 - c : c - (TS_EXP_LO - 1 - TS_B);
    atomicAdd(h + col * TS_COPIES, 1u);  // an integer LDS add: order-free
    a.nz += mag == 0u ? 1u : 0u;
    const double d = (double)x;
    a.s += d;
    a.ss += d * d;  // 24 x 24 bits: the product is exact in fp64
    a.mn = x < a.mn ? x : a.mn;
    a.mx = x > a.mx ? x : a.mx;
    return a;
  }
};
struct Max {  // block_fold for {-min, max}: no NaN reaches it
  __device__ __forceinline__ double operator()(double a, double b) const { return a > b ? a : b; }
};

// A float that is not a NaN as an unsigned key of the same order (and back): integer min / max on keys are the floats'.
__device__ __forceinline__ unsigned key_of(float f) {
  const unsigned u = __float_as_uint(f);
  return (u >> 31) != 0u ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned bits_of_key(unsigned k) { return (k >> 31) != 0u ? (k & 0x7fffffffu) : ~k; }

__device__ __forceinline__ long pack2(float lo, float hi) {
  return (long)(((unsigned long)__float_as_uint(hi) << 32) | (unsigned long)__float_as_uint(lo));
}

// Launch 1.  A chunk whose device row fails the checks the host entry made on its copy, or whose tensor is absent, reads
// nothing and leaves the neutral row (zero sums and counts, min = +inf, max = -inf).
__global__ __launch_bounds__(CHUNK_TPB) void tstats_partial_kernel(const long* __restrict__ table,
                                                                  const long* __restrict__ chunks, int n_tensors,
                                                                  long* __restrict__ ws, int n_chunks, int slots,
                                                                  const int* __restrict__ cursor) {
  __shared__ unsigned s_hist[TS_LDS_COLS * TS_COPIES];
  for (int i = threadIdx.x; i < TS_LDS_COLS * TS_COPIES; i += CHUNK_TPB)
    s_hist[i] = i / TS_COPIES == COL_MIN ? 0xffffffffu : 0u;
  __syncthreads();
  unsigned* mine = s_hist + (threadIdx.x & (TS_COPIES - 1));
  Chunk c;
  const bool ok = chunk_resolve(table, chunks, n_tensors, TS_TAB_ROW, 1, &c);  // block-uniform
  Acc a = {0.0, 0.0, INFINITY, -INFINITY, 0u};
  if (ok) {
    const long addr = c.row[0];
    if (addr != 0 && (addr & 3) == 0) {
      a = span_reduce(as_global(addr) + c.start, c.len, a, Elem{mine});
      if (a.nz != 0u) atomicAdd(mine + COL_ZERO * TS_COPIES, a.nz);
    }
  }
  // every thread, also one that saw no finite element (+inf / -inf: the neutral keys)
  atomicMin(mine + COL_MIN * TS_COPIES, key_of(a.mn));
  atomicMax(mine + COL_MAX * TS_COPIES, key_of(a.mx));
  double s[2] = {a.s, a.ss};
  block_fold(s, Sum());  // (its barrier also puts every LDS add, min and max above in front of the reads below)
  long* row = ws + WS_HEAD + n_chunks + (long)blockIdx.x * WS_ROW;
  // four threads per column fold 8 copies each, then two xor steps; the count columns' order in the row is their number
  const int col = threadIdx.x >> 2, q = threadIdx.x & 3;
  const bool is_min = col == COL_MIN, is_max = col == COL_MAX;
  unsigned n = is_min ? 0xffffffffu : 0u;
  if (col < TS_LDS_COLS) {
    const unsigned* h = s_hist + col * TS_COPIES + q * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) n = is_min ? min(n, h[i]) : (is_max ? max(n, h[i]) : n + h[i]);
  }
#pragma unroll
  for (int o = 1; o <= 2; o <<= 1) {
    const unsigned v = __shfl_xor(n, o, 64);
    n = is_min ? min(n, v) : (is_max ? max(n, v) : n + v);
  }
  if (q == 0) {
    if (col < TS_COLS) reinterpret_cast<unsigned*>(row + 3)[col] = n;
    if (is_min) reinterpret_cast<unsigned*>(row + 2)[0] = bits_of_key(n);  // {min, max}: the low and the high half
    if (is_max) reinterpret_cast<unsigned*>(row + 2)[1] = bits_of_key(n);
  }
  if (threadIdx.x == 0) {
    reinterpret_cast<double*>(row)[0] = s[0];
    reinterpret_cast<double*>(row)[1] = s[1];
    if (ok && c.start == 0) ws[WS_HEAD + c.ti] = (long)blockIdx.x;
    if (blockIdx.x == 0) {  // the slot every workgroup of launch 2 writes: read here, before anybody advances the cursor
      const int cur = cursor[0];
      ws[0] = (cur >= 0 && cur < slots) ? (long)cur : 0L;
      ws[1] = 0L;
    }
  }
}

// Launch 2.  Workgroup t: thread i folds the sums and min / max of the tensor's chunk rows i, i + 256, ... in chunk
// order, then block_fold; wavefront w adds the count columns of rows w, w + 4, ... (integers: order-free).  A tensor that
// is absent, or whose device row or first-chunk word fails the checks, gets the all-zero row.
__global__ __launch_bounds__(CHUNK_TPB) void tstats_finish_kernel(const long* __restrict__ table,
                                                                 const long* __restrict__ chunks, int n_tensors,
                                                                 const long* __restrict__ ws, int n_chunks,
                                                                 long* __restrict__ ring, int slots,
                                                                 int* __restrict__ cursor) {
  __shared__ long s_cnt[CHUNK_WAVES][64];
  const long t = blockIdx.x;
  long slot = ws[0];
  if (slot < 0 || slot >= slots) slot = 0;
  if (t == 0 && threadIdx.x == 0) {  // the only writer of both words; nobody reads them in this launch
    const int made = cursor[1];
    cursor[0] = (int)((slot + 1) % slots);
    cursor[1] = made < 0 ? 1 : (made < 0x7fffffff ? made + 1 : made);
  }
  long* out = ring + (slot * n_tensors + t) * TS_ROW;
  const long addr = table[t * TS_TAB_ROW], numel = table[t * TS_TAB_ROW + 1], first = ws[WS_HEAD + t];
  const long nch = (numel > 0 && numel <= (1L << 48)) ? (numel + CHUNK_ELEMS - 1) / CHUNK_ELEMS : 0;
  bool ok = addr != 0 && (addr & 3) == 0 && nch > 0 && first >= 0 && first <= n_chunks - nch;  // block-uniform
  if (ok) ok = chunks[2 * first] == t && chunks[2 * first + 1] == 0;
  if (!ok) {
    for (int i = threadIdx.x; i < TS_ROW; i += CHUNK_TPB) out[i] = 0L;
    return;
  }
  const long* rows = ws + WS_HEAD + n_chunks + first * WS_ROW;
  double s[2] = {0.0, 0.0};
  double m[2] = {-(double)INFINITY, -(double)INFINITY};  // -min, max
  for (long i = threadIdx.x; i < nch; i += CHUNK_TPB) {
    const long* r = rows + i * WS_ROW;
    s[0] += reinterpret_cast<const double*>(r)[0];
    s[1] += reinterpret_cast<const double*>(r)[1];
    const float mn = __uint_as_float((unsigned)((unsigned long)r[2] & 0xffffffffu));
    const float mx = __uint_as_float((unsigned)((unsigned long)r[2] >> 32));
    m[0] = Max()(m[0], -(double)mn);
    m[1] = Max()(m[1], (double)mx);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long n = 0;
  if (lane < TS_COLS)
    for (long i = wave; i < nch; i += CHUNK_WAVES) n += (long)reinterpret_cast<const unsigned*>(rows + i * WS_ROW + 3)[lane];
  s_cnt[wave][lane] = n;
  block_fold(s, Sum());  // (its barrier also publishes s_cnt)
  block_fold(m, Max());
  if (threadIdx.x < TS_COLS) {
    long tot = 0;
#pragma unroll
    for (int w = 0; w < CHUNK_WAVES; ++w) tot += s_cnt[w][threadIdx.x];
    const int k = threadIdx.x;
    out[k < TS_HIST ? 9 + k : (k == COL_NAN ? 2 : (k == COL_INF ? 3 : 4))] = tot;
  }
  if (threadIdx.x == 0) {
    const float mn = (float)-m[0], mx = (float)m[1];
    const float am = mn > mx ? 0.f : fmaxf(-mn, mx);  // no finite element: min = +inf, max = -inf, absmax = 0
    out[0] = 1L;
    out[1] = numel;
    out[5] = pack2(mn, mx);
    out[6] = pack2(am, 0.f);
    reinterpret_cast<double*>(out)[7] = s[0];
    reinterpret_cast<double*>(out)[8] = s[1];
  }
}

bool tstats_tables_ok(const long* tab, int n_tensors, const long* chunks, int n_chunks) {
  for (int t = 0; t < n_tensors; ++t) {
    const long* r = tab + (long)t * TS_TAB_ROW;
    if ((r[0] & 3) != 0 || r[1] <= 0 || r[1] > (1L << 48)) return false;  // (an address of 0: absent, not an error)
  }
  return chunks_tile(tab, TS_TAB_ROW, 1, n_tensors, chunks, n_chunks);
}
}  // namespace

extern "C" long sf_tensor_stats_ws_bytes(int n_chunks) {
  return n_chunks > 0 ? 8L * (WS_HEAD + (long)n_chunks * (1 + WS_ROW)) : 0L;
}

extern "C" int sf_tensor_stats(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                               const long* chunks, int n_chunks, void* ws, long ws_bytes, long* ring, int row, int slots,
                               int* cursor, void* stream) {
  if (!tables_args_ok(table_host, table, n_tensors, chunks_host, chunks, n_chunks)) return SF_EINVAL;
  if (!ws || !ring || !cursor || row != TS_ROW || slots <= 0) return SF_EINVAL;
  if (ws_bytes < sf_tensor_stats_ws_bytes(n_chunks)) return SF_EINVAL;
  if (!tstats_tables_ok(table_host, n_tensors, chunks_host, n_chunks)) return SF_EINVAL;
  if ((reinterpret_cast<uintptr_t>(ws) & 7) != 0 || (reinterpret_cast<uintptr_t>(ring) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(cursor) & 3) != 0)
    return SF_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tstats_partial_kernel, dim3(n_chunks), dim3(CHUNK_TPB), 0, s, table, chunks, n_tensors, (long*)ws,
                     n_chunks, slots, cursor);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(tstats_finish_kernel, dim3(n_tensors), dim3(CHUNK_TPB), 0, s, table, chunks, n_tensors,
                     (const long*)ws, n_chunks, ring, slots, cursor);
  SF_CHECK_LAUNCH();
  return SF_OK;
}
