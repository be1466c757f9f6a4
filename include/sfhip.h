/* sfhip.h — C ABI of libsfhip.so: the MI355X (gfx950) kernels behind the SlowFast / CMDA hot path.
 *
 * The reference (weidafeng/Efficient-SlowFast) has NO FFI: its hot path is Python nn.Modules whose
 * arithmetic is executed by ATen ops.  Each entry point below therefore names the reference module
 * call(s) it replaces (file:line under SlowFast/slowfast/models/) instead of a native symbol.
 *
 * Conventions
 *   - all tensors fp32, device pointers owned by the caller, NDHWC ("channels-last 3D"):
 *     element (n,t,h,w,c) of a tensor with row pitch `cs` (floats) and channel offset `coff` lives at
 *     ((((n*T + t)*H + h)*W + w) * cs + coff + c).  A pitch larger than the channel count lets a
 *     producer write straight into a slice of a wider (concatenated) tensor — torch.cat is never run.
 *   - every function only enqueues work on `stream` (a hipStream_t passed as void*); no allocation,
 *     no synchronisation, safe to capture into a hipGraph.
 *   - return 0 on success, a negative SF_E* code on a bad argument (nothing is enqueued then).
 */
#ifndef SFHIP_H
#define SFHIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define SF_OK 0
#define SF_EINVAL (-1)   /* inconsistent descriptor */
#define SF_EALIGN (-2)   /* pointer / pitch alignment not supported by any kernel variant */
#define SF_ELAUNCH (-3)  /* hipLaunch failed (hipGetLastError is left set) */
#define SF_ENOTTAKEN (-4) /* a specialised entry point (sf_conv_fwd_pw / _bx, sf_conv_wgrad_bx) does not serve this shape
                             or view: nothing was enqueued and the arguments are not at fault — call the general entry
                             point (sf_conv_fwd_ws / sf_conv_wgrad) instead */

#define SF_ACT_NONE 0
#define SF_ACT_RELU 1
#define SF_ACT_SIGMOID 2      /* head only */
#define SF_ACT_SOFTMAX 3      /* head only */
#define SF_ACT_HSIGMOID 4     /* relu6(x+3)/6, ghostnet_helper.py:27-31 */
#define SF_ACT_RELU6 5        /* min(max(x,0),6), mobilenetv2_helper.py:15-30 */

int sf_abi_version(void);
/* Name of the gfx target the library was built for ("gfx950"). */
const char* sf_build_arch(void);

/* ---- layout -------------------------------------------------------------------------------
 * NCTHW (the callers' layout, datasets/utils.py:73-112) -> NDHWC with the channel dim padded to
 * `cpad` (zeros) and the H/W borders zero-padded by ph/pw (so the stem conv needs no border test).
 * dst dims: [N, T, H+2*ph, Wp, cpad] with Wp >= W+2*pw (extra columns zero).            */
int sf_ncthw_to_ndhwc(const float* src, float* dst, int N, int C, int T, int H, int W,
                      int cpad, int ph, int pw, int Wp, void* stream);
/* NDHWC slice (pitch cs, offset coff, C channels) -> dense NCTHW (module-boundary outputs). */
int sf_ndhwc_to_ncthw(const float* src, int cs, int coff, float* dst, int N, int C, int T, int H,
                      int W, void* stream);

/* ---- dense convolution as implicit GEMM on fp32 MFMA ------------------------------------------
 * Replaces nn.Conv3d(+BatchNorm3d eval affine)(+residual add)(+ReLU) of
 *   stem_helper.py:157-178 (conv), resnet_helper.py:182-223 (a/b/c), :326-335 (branch1),
 *   video_model_builder.py:128-141 (conv_f2s), custom_video_model_builder.py:102-108
 *   (downsample_c_of_slow), wdf_attention_helper.py:21-29 (q/k/v), head Linear (head_helper.py:181).
 * out[m, n] = act( scale[n] * (sum_{tap,c} in[row(m,tap), c] * w[n, tap, c]) + bias[n] + res[m, n] )
 * Weights are pre-packed [Cout][kT*kH*kW][cin_pad] (cin_pad = Cin rounded up to 16, zero filled). */
typedef struct sf_conv_desc {
  int N, Ti, Hi, Wi, Cin;      /* input dims; Cin = contiguous floats consumed per tap            */
  int in_cs, in_coff;          /* input pitch / channel offset                                    */
  int To, Ho, Wo, Cout;        /* output dims                                                     */
  int out_cs, out_coff;        /* output pitch / channel offset                                   */
  int out_cmul;                /* output channel n is stored at out_coff + n*out_cmul (channel    */
                               /* shuffle folded into index math, shufflenetv2_helper.py:32-43)   */
  int kT, kH, kW, sT, sH, sW, pT, pH, pW, dT, dH, dW;
  int cin_pad;                 /* packed weight row length per tap                                */
  int act;                     /* SF_ACT_NONE | SF_ACT_RELU | SF_ACT_RELU6                        */
  int res_cs, res_coff;        /* residual pitch / offset (used when res != NULL)                 */
  int transposed;              /* 1: data-gradient of the conv described by k/s/p/d: "in" is dL/dz with   */
                               /* dims (Ti,Hi,Wi) = the forward OUTPUT dims, "out" is dL/dx with dims     */
                               /* (To,Ho,Wo) = the forward INPUT dims, weights packed [Cin][tap][Cout]    */
  int os_T, os_H, os_W;        /* scattered store (all <= 1: dense).  Output position (t,h,w) of this launch  */
  int oo_T, oo_H, oo_W;        /* is written (and its residual read) at (t*os_T+oo_T, h*os_H+oo_H,            */
  int ob_T, ob_H, ob_W;        /* w*os_W+oo_W) of a destination with dims ob_T x ob_H x ob_W: one residue     */
                               /* class of the data gradient of a strided conv (resnet_helper.py:179,         */
                               /* :326-335 stride-2 3x3 / 1x1) is then a DENSE small-kernel conv over dL/dz.   */
} sf_conv_desc;
int sf_conv_fwd(const sf_conv_desc* d, const float* in, const float* w_packed, const float* scale,
                const float* bias, const float* res, float* out, void* stream);
/* Split-K schedule for short-M / long-K layers (res4 / res5: M <= 12544 positions, K = 2304..6144): the K steps of a
 * tile are shared by S workgroups that store raw partial tiles to ws [S][M][Cout]; a finish kernel sums them in split
 * order (no float atomics) and applies the epilogue.  sf_conv_fwd_ws_floats(d) = workspace floats (0: the single-pass
 * schedule is used); ws == NULL makes sf_conv_fwd_ws identical to sf_conv_fwd.                                   */
long sf_conv_fwd_ws_floats(const sf_conv_desc* d);
int sf_conv_fwd_ws(const sf_conv_desc* d, const float* in, const float* w_packed, const float* scale,
                   const float* bias, const float* res, float* out, float* ws, void* stream);
/* nn.Conv3d(groups = G) with 1 < G < channels — the grouped 1x1x1 convs of ShuffleUnit (shufflenet_helper.py:48-63,
 * conv1x1x1(groups) :36-45, followed by channel_shuffle :22-34) and the grouped 1x3x3 of BottleneckTransform when
 * RESNET.NUM_GROUPS > 1 (resnet_helper.py:196-205) — as ONE launch: the block-diagonal GEMM's group is the grid's z
 * index of the LDS-tiled kernel (conv_igemm.hip).  `d` describes the WHOLE layer: Cin / Cout = all groups' channels,
 * cin_pad = the packed width of ONE group's Cin / G input channels; w_packed = [Cout][taps][cin_pad] = the G per-group
 * packs one after the other (sf_pack_conv_weight of the grouped parameter [Cout][Cin / G][kT][kH][kW]).  Group g reads
 * input channels [g Cin / G, (g + 1) Cin / G) and owns output channels, scale / bias / residual entries
 * [g Cout / G, (g + 1) Cout / G).  shuffle != 0: its channel j is STORED at channel j * G + g — channel_shuffle(., G)
 * as index math of the stores.  d->transposed = 1: the data gradient (d->Cin = the forward Cout, w_packed = the G
 * transposed packs [Cin_fwd][taps][pad(Cout_fwd / G)]; strided layers predicate the taps, os_* must be <= 1).
 * d->out_cmul must be 1.  groups == 1 && !shuffle: sf_conv_fwd.                                                   */
int sf_conv_fwd_grouped(const sf_conv_desc* d, int groups, int shuffle, const float* in, const float* w_packed,
                        const float* scale, const float* bias, const float* res, float* out, void* stream);
/* Training-mode BN statistics out of the conv's epilogue (Conv3d -> BatchNorm3d of stem_helper.py:239-254,
 * resnet_helper.py:150-215 in train mode): the per-wavefront conv kernels keep shifted sums of the outputs they store
 * and leave [count, K, sum(v - K), sum((v - K)^2)] x 4 channels per (part, channel quad) in stats_ws
 * [parts][Cout / 4][4][4] (a part = one M tile, or the 4 M tiles of a workgroup); sf_bn_train_stats_merge below turns those into what sf_bn_train_stats returns without a pass over
 * the activation.  sf_conv_stats_ws_floats(d) = floats of stats_ws (0: this shape never produces statistics).
 * sf_conv_fwd_stats sets *parts to the rows written, or to 0 when none were (epilogue with scale / res / act, or the
 * LDS-tiled kernels took the launch): the caller then runs sf_bn_train_stats on the output.                      */
long sf_conv_stats_ws_floats(const sf_conv_desc* d);
int sf_conv_fwd_stats(const sf_conv_desc* d, const float* in, const float* w_packed, const float* scale,
                      const float* bias, const float* res, float* out, float* stats_ws, int* parts, void* stream);
/* Tuning knobs of the conv launchers for tests and microbenchmarks (process-wide, not used by the model code; the one
 * way to force a form — the library reads no environment variable for this):
 *   0: value 0 routes every conv to the LDS-tiled kernels of conv_igemm.hip instead of the per-wavefront kernels of
 *      conv_wave.hip;  1: force tile configuration `value` of conv_wave.hip (-1: planner);  2: force the rows per M
 *      tile (0: planner);  4: the persistent swapped-operand form (0 never, 1 the built-in default = level 3,
 *      10 + L = level L: 1 every KS == 1 layer it covers, 2 plain layers, 3 plain layers with <= 5 K steps);
 *   6: conv_small.hip (0 off, 1 by rule, 3 every shape it covers; values 0..3);
 *   7: conv_bx.hip forward / data gradient (0 off, 1 where it wins, 2 every shape it covers);  9: its weight gradient
 *      (same values);
 *   10 / 11 / 12: the weight-gradient kernels of conv_wgrad_wave.hip / conv_wgrad_rows.hip — 10: value 0 routes every
 *      weight gradient to conv_wgrad.hip, 11: force the blocks per wavefront (-1: planner), 12: workgroups to aim at
 *      (0: default);
 *   20: conv_wgrad_rows.hip off / on;  21: conv_pw_bx_kernel (0 off, 1 by model, 2 every shape it covers);
 *   22: conv_rows.hip (0 off, 1 the built-in default: the ring over t for 3x1x1 layers with <= 16 output channels,
 *      2 every shape it covers);  23: the weight-gradient ring over t of conv_wgrad_rows.hip (0 off, 1 on, -1 the
 *      built-in default = on);
 *   30: the row-march depthwise kernels (dwconv_march.hip) off / on;  31: its stride-(1,2,2) marches alone.
 * Returns SF_EINVAL for any other knob (3, 5 and 8 were removed with the forms they selected) and for a value of knob
 * 6 outside 0..3. */
int sf_conv_tune(int knob, int value);
/* ---- long reductions on the bf16 matrix pipe with fp32-exact operands (conv_bx.hip) --------------------------------
 * gfx950's f32-input MFMA runs at the vector rate, its bf16 MFMA at 16x that.  Every fp32 value is the EXACT sum of
 * three bf16 pieces (8 significand bits each) and six bf16 MFMAs with fp32 accumulation give the fp32 product to fp32
 * rounding level (the dropped terms are below 2^-24 |a||b|): the 1x3x3 / 3x1x1 layers over >= 128 channels of
 * resnet_helper.py:182-223 and their data gradients run that way where it is faster than v_mfma_f32_*_f32
 * (sf_conv_fwd_ws routes them itself; sf_conv_tune(7, 0) switches it off, (7, 2) takes every shape the kernel covers).
 * sf_bx_split: x [rows][cs] fp32 (C channels from coff; C % 8 == 0) -> planes[3][rows + 1][C] bf16 (row `rows` = 0),
 *   sf_bx_planes_elems(rows, C) 16-bit elements, 16-byte aligned.
 * sf_conv_fwd_bx: sf_conv_fwd_ws with the operand planes handed in — in_planes = sf_bx_split of the input view
 *   ([N*Ti*Hi*Wi][Cin]), w_planes = sf_bx_split of the packed weights ([Cout][taps*Cin]); either may be NULL (made in
 *   ws).  ws: sf_conv_bx_ws_floats(d, have_in_planes, have_w_planes) floats; 0 = the shape is not served (SF_EINVAL). */
long sf_bx_planes_elems(long rows, int C);
int sf_bx_split(const float* x, int cs, int coff, long rows, int C, unsigned short* planes, void* stream);
/* sf_bx_split of n DENSE tensors (pitch = C) in one launch — the packed weights of every bf16-piece layer after an
 * optimizer step (models/optimizer.py step -> every nn.Conv3d weight of resnet_helper.py:182-223 changes).  items: n
 * records {const float* x; uint16_t* planes; int64_t rows; int32_t C; int32_t 0}; blk0[i] = first workgroup of item i
 * (a workgroup = 256 elements of 8 channels over (rows + 1) * C / 8), blk0[n] = nblocks.                           */
int sf_bx_split_batched(const void* items, const int* blk0, int n, int nblocks, void* stream);
/* Small-channel stride-1 "same" layers (Cin <= 32 or Cout <= 32; 1x1x1, 3x1x1, 1x3x3 — the Fast pathway's convs of
 * resnet_helper.py:182-223, the lateral and query / key / value projections) and, with desc.transposed, their data
 * gradients: conv_rows.hip (whole rows through LDS, swapped-operand MFMAs, BN statistics in the epilogue).  sf_conv_fwd
 * / sf_conv_fwd_stats route there by themselves; sf_conv_rows_parts = the statistics records per channel such a launch
 * leaves (4 per workgroup; 0: the shape is not served).  sf_conv_tune(22, 0 | 1 | 2) = off / by rule / every shape the
 * kernel covers.                                                                                                     */
int sf_conv_rows_parts(const sf_conv_desc* d);
/* Pointwise layers — 1x1x1 stride-1 convs with >= 64 channels on both sides, forward and (desc.transposed) data
 * gradient: nn.Conv3d branch2a / branch2c of resnet_helper.py:182-223 — on the bf16 matrix pipe with the ACTIVATIONS
 * split in registers (no activation planes; conv_bx.hip conv_pw_bx_kernel).  sf_conv_pw_ws_floats: workspace floats
 * (0: the shape is not served, or the launcher's time model leaves it to the f32 kernels); w_planes = sf_bx_split of the
 * packed weight ([Cout][Cin]) or NULL (made in ws).  stats != NULL (a buffer of sf_conv_pw_stats_floats(d) floats,
 * only without scale / res / activation): the training-mode BN statistics of the stored outputs as sf_conv_fwd_stats
 * leaves them — *parts record rows per channel for sf_bn_train_stats_merge.  sf_conv_fwd_ws routes here by itself
 * (sf_conv_fwd_ws_floats covers it); sf_conv_tune(21, 0 | 1 | 2) = off / by model / every shape it covers.            */
long sf_conv_pw_ws_floats(const sf_conv_desc* d, int have_w_planes);
long sf_conv_pw_stats_floats(const sf_conv_desc* d);
int sf_conv_fwd_pw(const sf_conv_desc* d, const float* in, const float* w_packed, const unsigned short* w_planes,
                   const float* scale, const float* bias, const float* res, float* out, float* ws, float* stats,
                   int* parts, void* stream);
long sf_conv_bx_ws_floats(const sf_conv_desc* d, int have_in_planes, int have_w_planes);
int sf_conv_fwd_bx(const sf_conv_desc* d, const float* in, const unsigned short* in_planes, const float* w_packed,
                   const unsigned short* w_planes, const float* scale, const float* bias, const float* res, float* out,
                   float* ws, void* stream);
/* Packs an nn.Conv3d weight [Cout][Cin][kT*kH*kW] (device) into wp [Cout][taps][cin_pad] and — when wtp != NULL —
 * wtp [Cin][taps][cout_pad] (the data-gradient order), zero padded, in one launch.                           */
int sf_pack_conv_weight(const float* w, int Cout, int Cin, int taps, float* wp, int cin_pad, float* wtp,
                        int cout_pad, void* stream);
/* The same for n weights in ONE launch (a training step re-packs every conv after the optimizer step).  items: device
 * array of n records { const float* w; float* wp; float* wtp; int Cout, Cin, taps, cin_pad, cout_pad, pad; long n_wp
 * (= Cout*taps*cin_pad), total (= n_wp + Cin*taps*cout_pad, or n_wp when wtp is NULL) } (64 bytes each); blk0: device
 * array of n + 1 ints, blk0[i] = first 256-thread workgroup of weight i, blk0[n] = nblocks.  Weight i takes, for the
 * forward layout, ceil(Cout / 8) * ceil(cin_pad / 32) workgroups when 2 <= taps <= 9 and ceil(n_wp / 256) otherwise,
 * plus ceil(Cin*taps / 32) * ceil(cout_pad / 32) for the transposed one (32 x 32 tiles through LDS; wtp required).  */
int sf_pack_conv_weights(const void* items, const int* blk0, int n, int nblocks, void* stream);

/* ---- depthwise convolution (groups == channels) ----------------------------------------------
 * ghostnet_helper.py:88-90,114-120,137-143; shufflenetv2_helper.py:62-64,74-75,89-91.
 * Weights packed [kT*kH*kW][C].  `Cout` <= C output channels are produced (GhostModule's
 * out[:, :oup] slice, ghostnet_helper.py:99).  kT x 3 x 3 (kT = 1 | 3) stride-1 "same" layers — the cheap operations
 * and stride-1 conv_dw of ghostnet_helper.py, the branch convs of shufflenetv2_helper.py — run as row marches
 * (dwconv_march.hip: a thread walks a column of rows with the 3 x 3 x kT window in registers), forward, data and weight
 * gradient; every other shape on the position-per-thread kernels.  Same results either way (fp32 sums in tap order). */
int sf_dwconv_fwd(const sf_conv_desc* d, const float* in, const float* w_packed, const float* scale,
                  const float* bias, const float* res, float* out, void* stream);

/* ---- pooling ------------------------------------------------------------------------------------
 * MaxPool3d (stem_helper.py:169-171; ShuffleNetV2 stem :248) / AvgPool3d stride 1 (head_helper.py:176).
 * is_avg: 0 = max (padding ignored), 1 = average, count_include_pad (no padding used by callers). */
typedef struct sf_pool_desc {
  int N, Ti, Hi, Wi, C, in_cs, in_coff;
  int To, Ho, Wo, out_cs, out_coff;
  int kT, kH, kW, sT, sH, sW, pT, pH, pW;
  int is_avg;
} sf_pool_desc;
int sf_pool_fwd(const sf_pool_desc* d, const float* in, float* out, void* stream);
/* Max pooling that also records the winning tap of every window — the FIRST maximum in (kt, kh, kw) scan order,
 * nn.MaxPool3d's rule (stem_helper.py:117-119 pool1, nonlocal_helper.py:75-79) — as one byte per output element, arg
 * [N*To*Ho*Wo][C] dense.  sf_maxpool_bwd_arg then gathers dL/dy into dL/dx from `arg` alone (no x, no y, no tie
 * search); overwrite != 0: dx is written (zero where an element won no window), else accumulated.  Both need
 * float4-addressable views (C, pitches, offsets multiples of 4, 16-byte aligned bases) and <= 255 taps: SF_EINVAL
 * otherwise (callers keep sf_pool_fwd / sf_maxpool_bwd for those).                                                 */
int sf_maxpool_fwd_arg(const sf_pool_desc* d, const float* in, float* out, unsigned char* arg, void* stream);
int sf_maxpool_bwd_arg(const sf_pool_desc* d, const unsigned char* arg, const float* dy, int dy_cs, int dy_coff,
                       float* dx, int dx_cs, int dx_coff, int overwrite, void* stream);

/* ---- CMDA Fast->Slow edge: MaxPool3d(alpha,1,1) -> ECA -> BN -> ReLU -> concat ------------------
 * custom_video_model_builder.py:131-135 + wdf_attention_helper.py:77-91, two launches:
 *  (1) pooled[b,c] = mean_{t',h,w} max_{r<alpha} x[b, t'*alpha + r, h, w, c]        (sf_tmax_mean)
 *  (2) out[b,t',h,w,coff+c] = act(scale[c] * (max_r x[...] * gate[b,c]) + bias[c])   (sf_gate_apply)
 *      gate = sigmoid(conv1d_k3(pooled)) when w3 != NULL (ECA), or
 *      gate = hsigmoid(pooled_gate[b,c]) when w3 == NULL (SqueezeExcite, ghostnet_helper.py:46-52;
 *      `pooled` then already holds conv_expand's output).                                          */
/* `ws` is caller-provided scratch of sf_tmax_mean_ws_floats(N, C) floats: the mean is reduced through a
 * FIXED number of partial sums per clip (no float atomics), so results are bit-reproducible.        */
long sf_tmax_mean_ws_floats(int N, int C);
int sf_tmax_mean(const float* x, int cs, int coff, int N, int T, int H, int W, int C, int alpha,
                 float* pooled, float* ws, void* stream);
int sf_gate_apply(const float* x, int cs, int coff, int N, int T, int H, int W, int C, int alpha,
                  const float* pooled, const float* w3, const float* scale, const float* bias, int act,
                  float* out, int out_cs, int out_coff, void* stream);

/* ---- CMDA Slow->Fast edge: SpatialAttention (flash-style, never materialises N x N) -------------
 * wdf_attention_helper.py:41-54 fused with custom_video_model_builder.py:143-146:
 *   S = q k^T (no 1/sqrt(d)), P = softmax_j(S), o = P v, y = gamma*o + x,
 *   z = relu(scale*y + bias)  (bn_s2f eval affine; skipped when scale == NULL),
 *   written `alpha` times along T (nn.Upsample nearest) into out (pitch out_cs, offset out_coff).
 * q,k,v,x: [B, N=T*H*W, C] views with pitches q_cs.. (q,k,v normally slices of one [B,N,3C] buffer).
 * gamma is read from device memory (it is an nn.Parameter).
 * o_save / lse_save (optional, training): O = P v [B, N, C] dense and the log2-domain log-sum-exp [B, N]
 * of every query row, which sf_attn_bwd recomputes P from.                                           */
int sf_attn_fwd(const float* q, int q_cs, const float* k, int k_cs, const float* v, int v_cs,
                const float* x, int x_cs, const float* gamma, const float* scale, const float* bias,
                int act, float* out, int out_cs, int out_coff, int B, int T, int H, int W, int C,
                int alpha, float* o_save, float* lse_save, void* stream);

/* Same, with a workspace of sf_attn_fwd_ws_floats(B, N = T*H*W, C) floats (16-byte aligned): the launcher may then
 * cut the key sweep into up to 8 parts so that the last round of workgroups fills all CUs (B * N/128 query tiles on
 * 256 CUs otherwise leave up to one workgroup-time of tail), merging the parts' (O, max, denominator) in a second
 * kernel that also runs the epilogue.  Same results up to fp32 summation order; deterministic.              */
long sf_attn_fwd_ws_floats(int B, int N, int C);
/* Which arithmetic serves the attention products of head width C when a workspace is given (sf_attn_fwd_ws,
 * sf_attn_bwd_fused): 0 = v_mfma_f32_*_f32 (fp32 operands); 6 = every fp32 operand as the exact sum of three bf16
 * pieces and every fp32 product as six v_mfma_f32_32x32x16_bf16 (fp32 accumulate; the dropped terms are below
 * 2^-24 |a||b|, one fp32 rounding) — 17 <= C <= 64 (33..64 as two 32-channel blocks) and C = 8 (packed planes)
 * with 16-byte aligned rows; other views (C % 4 != 0, unaligned strides or pointers) take the f32 MFMA.           */
int sf_attn_products_per_fp32(int C);
int sf_attn_fwd_ws(const float* q, int q_cs, const float* k, int k_cs, const float* v, int v_cs,
                   const float* x, int x_cs, const float* gamma, const float* scale, const float* bias,
                   int act, float* out, int out_cs, int out_coff, int B, int T, int H, int W, int C,
                   int alpha, float* o_save, float* lse_save, float* ws, void* stream);

/* SpatialAttention backward (recompute form): dz = dL/d(gamma*O + x) [B, N, C]; dvec[i] = <dz_i, O_i>
 * (sf_rowdot); writes dq, dk, dv (overwrite).  dx = dz and dgamma = sum(dvec) are the caller's.        */
int sf_attn_bwd(const float* q, int q_cs, const float* k, int k_cs, const float* v, int v_cs,
                const float* dz, int dz_cs, const float* lse, const float* dvec, const float* gamma,
                float* dq, int dq_cs, float* dk, int dk_cs, float* dv, int dv_cs, int B, int N, int C,
                int which /* 1 = dQ kernel, 2 = dK/dV kernel, 3 = both */, void* stream);

/* Single-sweep form of sf_attn_bwd for 16 < C <= 64: dK/dV and dQ in one pass over the (key block, query tile)
 * pairs — S and dP are recomputed once (5 MFMA products per tile instead of 3 + 4).  Each 128-key workgroup writes
 * its share of dQ to a plane of the workspace ws [B][ceil(N/128)][N][32|64] (four wavefronts summed in a fixed order
 * through LDS) and a second kernel sums the planes: no float atomics, bit-reproducible.
 * sf_attn_bwd_fused_ws_floats returns the workspace size in floats, or 0 when the shape is not served.          */
long sf_attn_bwd_fused_ws_floats(int B, int N, int C);
int sf_attn_bwd_fused(const float* q, int q_cs, const float* k, int k_cs, const float* v, int v_cs, const float* dz,
                      int dz_cs, const float* lse, const float* dvec, const float* gamma, float* dq, int dq_cs,
                      float* dk, int dk_cs, float* dv, int dv_cs, int B, int N, int C, float* ws, void* stream);

/* Which kernel instantiation sf_attn_bwd_fused launches for (B, N, C) on 16-byte aligned views, as 10 * family +
 * wavefronts per workgroup (family 1 = f32 MFMA d <= 16, 2 = packed bf16 planes d = 8, 3 = bf16 pieces d <= 32,
 * 4 = bf16 pieces d <= 64 in two channel blocks, 5 / 6 = f32 MFMA d <= 32 / <= 64, 7 = two-kernel form d = 128;
 * 0 = shape not served).  The choice depends on the batch (B * ceil(N / 256) >= 256 selects the 8-wavefront form of
 * family 3, i.e. B >= 3 at N = 25 088): parity tests assert which one they exercised.                             */
int sf_attn_bwd_variant(int B, int N, int C);
/* Process-wide knobs of the attention launchers for tests, 0 when the library loads: knob 0 = wavefronts per
 * workgroup of the backward sweeps that come in two widths, the bf16 d = 32 and d = 8 ones and the f32 d <= 4 one
 * (0 = by shape, 4, 8); knob 1 = parts every sweep is cut into (0 = by fill, 1..8).  Other values: SF_EINVAL.    */
int sf_attn_tune(int knob, int value);

/* ---- streaming cross-length attention (M/nonlocal_helper.py:105-148; attn_cross.hip) --------------------------------
 *   Y[b,i,:] = sum_j softmax_j(sm_scale <Q[b,i,:], K[b,j,:]>) V[b,j,:]
 * Q [B,Nq,d], K [B,Nk,d], V [B,Nk,dv], Y [B,Nq,dv] as (pointer, row pitch) views: pitch >= width, 16-byte aligned
 * rows.  The Nq x Nk scores are never written to memory, forward or backward.  fp32 on v_mfma_f32_32x32x2_f32.
 * sf_xattn_accepts (M/nonlocal_helper.py:105-148): 1 when the kernels serve the shape (1 <= Nq, Nk; 4 <= d, dv <= 512,
 *   both multiples of 4), else 0.  Host only.
 * sf_xattn_bwd_ws_floats (M/nonlocal_helper.py:105-148): workspace of sf_xattn_bwd in floats (0: every gradient element
 *   has one owner, so there are no partial planes).  Host only.
 * sf_xattn_fwd (M/nonlocal_helper.py:105-148): writes y and lse [B,Nq] (log2-domain log-sum-exp of every query row).
 * sf_xattn_bwd (M/nonlocal_helper.py:105-148): dvec[b,i] = <dY_i, Y_i> (sf_rowdot); a key-stationary kernel writes
 *   dk, dv_, a query-stationary one dq, both recomputing P from lse; no float atomics, bit-reproducible.
 *   accumulate_mask: bit 0 / 1 / 2 set = dq / dk / dv_ is added to, clear = overwritten.  ws may be NULL.
 * SF_EALIGN: a misaligned view; SF_ENOTTAKEN: a shape sf_xattn_accepts refuses; SF_EINVAL: anything else.  No
 * allocation and no host synchronisation.                                                                        */
int sf_xattn_accepts(long Nq, long Nk, int d, int dv);
long sf_xattn_bwd_ws_floats(int B, long Nq, long Nk, int d, int dv);
int sf_xattn_fwd(const float* q, int q_cs, const float* k, int k_cs, const float* v, int v_cs, float* y, int y_cs,
                 float* lse, int B, long Nq, long Nk, int d, int dv, float sm_scale, void* stream);
int sf_xattn_bwd(const float* q, int q_cs, const float* k, int k_cs, const float* v, int v_cs, const float* dy,
                 int dy_cs, const float* lse, const float* dvec, float* dq, int dq_cs, float* dk, int dk_cs,
                 float* dv_, int dv_cs, int accumulate_mask, int B, long Nq, long Nk, int d, int dv, float sm_scale,
                 float* ws, void* stream);

/* ---- associative "dot_product" attention (M/nonlocal_helper.py:105-148; attn_assoc.hip) ------------------------------
 *   Y = (theta phi^T / N_k) g = theta (phi^T g / N_k): without a softmax the product is associative, so the
 *   N_q x N_k scores are never formed; M = phi^T g / N_k is one d x dv matrix per sample.  Two batched products on
 *   v_mfma_f32_32x32x2_f32, fp32 in and out.  Views are (pointer, row pitch): pitch >= width, 16-byte aligned rows,
 *   widths multiples of 4 in 4..512.  No float atomics: one owner per output element and a fixed summation order.
 * sf_assoc_accepts (M/nonlocal_helper.py:105-148): 1 when the two kernels serve theta [Nq,d], phi [Nk,d], g [Nk,dv]
 *   (1 <= Nq, Nk; 4 <= d, dv <= 512, both multiples of 4), else 0.  Host only.
 * sf_gram_splits (M/nonlocal_helper.py:105-148): chunks S >= 1 the R rows of sf_gram are cut into (more than 1 only
 *   where da x db has too few 32 x 32 tiles to fill the chip).  S depends on (R, da, db) alone, so the bits of one
 *   sample do not depend on the batch it is in.  Host only.
 * sf_gram_ws_floats (M/nonlocal_helper.py:105-148): workspace of sf_gram in floats, S B da db partial planes; 0 when
 *   S == 1.  Host only.
 * sf_gram (M/nonlocal_helper.py:105-148): G[b] = alpha A[b]^T B[b] for A [B,R,da], B [B,R,db] (views) into dense
 *   G [B,da,db]; gt != NULL also receives G^T [B,db,da], element for element the same floats.  Rows past R and columns
 *   past the width are never read.  ws: sf_gram_ws_floats floats, 16-byte aligned (may be NULL when that is 0); with
 *   S > 1 a second launch sums the planes in chunk order.
 * sf_rowmat (M/nonlocal_helper.py:105-148): Y[b,r,j] = alpha sum_i X[b,r,i] W[b,j,i] for X [B,R,k] (view), dense
 *   W [B,n,k] ("weight layout": both operands reduce along contiguous floats) into the view Y [B,R,n]; accumulate != 0
 *   adds to Y instead of overwriting it.
 * SF_EALIGN: a misaligned pointer or a pitch that is not a multiple of 4; SF_ENOTTAKEN: a shape sf_assoc_accepts
 *   refuses; SF_EINVAL: anything else (null pointers, B <= 0, R <= 0, pitch < width, a missing workspace).  No
 *   allocation and no host synchronisation.                                                                        */
int sf_assoc_accepts(long Nq, long Nk, int d, int dv);
int sf_gram_splits(int B, long R, int da, int db);
long sf_gram_ws_floats(int B, long R, int da, int db);
int sf_gram(const float* a, int a_cs, const float* b, int b_cs, float* g, float* gt, int B, long R, int da, int db,
            float alpha, float* ws, void* stream);
int sf_rowmat(const float* x, int x_cs, const float* w, float* y, int y_cs, int B, long R, int k, int n, float alpha,
              int accumulate, void* stream);

/* ---- training-mode BatchNorm3d forward pieces (batchnorm_helper.py:15-34 -> nn.BatchNorm3d, training=True)
 * sf_channel_stats: per-channel mean and BIASED variance over all rows of an NDHWC slice, reduced through
 *   a fixed number of fp32 partials combined in fp64 (bit-reproducible; ws = sf_channel_stats_ws_floats(C)).
 * sf_affine_fwd:    out = act(x * scale[c] + bias[c] + res), optionally repeated `rep` times along T
 *   (nn.Upsample nearest, custom_video_model_builder.py:120-121) — the normalise(+residual)(+ReLU) pass.   */
long sf_channel_stats_ws_floats(int C);
int sf_channel_stats(const float* x, int cs, int coff, long rows, int C, float* mean, float* var, float* ws,
                     void* stream);
/* Statistics + everything parameter-sized in one call: mean/var/invstd, scale = gamma*invstd,
 * shift = beta - mean*scale, and the in-place running_mean / running_var update (momentum, unbiased var). */
int sf_bn_train_stats(const float* x, int cs, int coff, long rows, int C, const float* gamma, const float* beta,
                      float eps, float momentum, float* run_mean, float* run_var, float* mean, float* var,
                      float* invstd, float* scale, float* shift, float* ws, void* stream);
/* The same outputs from the per-part sums of sf_conv_fwd_stats (every part shifted to one reference, summed in fp64
 * in a fixed order); C must be a multiple of 4.                                                              */
int sf_bn_train_stats_merge(const float* parts_ws, int parts, int C, const float* gamma, const float* beta, float eps,
                            float momentum, float* run_mean, float* run_var, float* mean, float* var, float* invstd,
                            float* scale, float* shift, void* stream);
int sf_affine_fwd(const float* x, int cs, int coff, int N, int T, int H, int W, int C, const float* scale,
                  const float* bias, const float* res, int res_cs, int res_coff, int act, int rep, float* out,
                  int out_cs, int out_coff, int out_cmul, void* stream);

/* ---- head tail (eval): activation over classes then mean over T,H,W -----------------------------
 * head_helper.py:217-221.  logits [B, P, K] -> out [B, K]; act = SF_ACT_SOFTMAX | SIGMOID | RELU | NONE */
int sf_head_act_mean(const float* logits, int B, int P, int K, int act, float* out, void* stream);

/* ---- elementwise helpers ------------------------------------------------------------------------
 * Copy a channel slice (concat pass-through / channel shuffle of the un-convolved half,
 * shufflenetv2_helper.py:100-107): out[.., out_coff + c*out_cmul] = in[.., in_coff + c].          */
int sf_copy_channels(const float* in, int in_cs, int in_coff, float* out, int out_cs, int out_coff,
                     int out_cmul, long rows, int C, void* stream);
/* channel_shuffle(x, groups) of shufflenet_helper.py:22-34 (view [B, G, C/G, ...] -> transpose(1, 2) -> flatten) in
 * one launch: out[.., out_coff + j*G + g] (+)= in[.., in_coff + g*(C/G) + j]  (accumulate != 0 adds).  Its inverse —
 * the backward's gather — is the same call with groups = C / G.                                               */
int sf_channel_shuffle(const float* in, int in_cs, int in_coff, float* out, int out_cs, int out_coff, int groups,
                       long rows, int C, int accumulate, void* stream);

/* ================================ backward (training) ============================================
 * Gradients of the ops above.  Activation gradients live in NDHWC buffers shaped like their forward
 * tensors; producers ACCUMULATE into them (the caller zero-fills once), which realises autograd's fan-in
 * sums (residual branches, the two consumers of each pathway tensor in the lateral fusions).
 *
 * Data gradient of a dense conv = sf_conv_fwd with desc.transposed = 1 (see sf_conv_desc).
 *
 * Weight gradient: partial[s][co][tap][ci] over S = sf_conv_wgrad_splits(d) position splits; the caller
 * sums the S partials (fixed order).  `d` is the FORWARD descriptor; dz is dL/d(conv output).          */
int sf_conv_wgrad_splits(const sf_conv_desc* d);
/* The same on the bf16 matrix pipe (conv_bx.hip: fp32 operands as three exact bf16 pieces, six MFMAs per product,
 * fragments by transposing LDS reads) for the long-reduction layers: sf_conv_wgrad_bx_splits(d) = S of its partial
 * buffer [S][Cout][taps][Cin] (0: shape not served, use sf_conv_wgrad); x_planes / dz_planes = sf_bx_split of the
 * input view ([N*Ti*Hi*Wi][Cin]) / of dz ([M][Cout]) or NULL (made in ws: sf_conv_wgrad_bx_ws_floats(d, have_x,
 * have_dz) floats).  sf_conv_wgrad_finish sums and un-packs the partials as for sf_conv_wgrad.  sf_conv_tune(9, 0 | 1
 * | 2): off / where it wins / every shape it covers.                                                              */
int sf_conv_wgrad_bx_splits(const sf_conv_desc* d);
long sf_conv_wgrad_bx_ws_floats(const sf_conv_desc* d, int have_x_planes, int have_dz_planes);
int sf_conv_wgrad_bx(const sf_conv_desc* d, const float* x, const unsigned short* x_planes, const float* dz, int dz_cs,
                     int dz_coff, const unsigned short* dz_planes, float* partial, float* ws, void* stream);
int sf_conv_wgrad(const sf_conv_desc* d, const float* x, const float* dz, int dz_cs, int dz_coff,
                  float* partial, void* stream);
/* Weight gradient of the grouped convs of sf_conv_fwd_grouped in ONE launch (group = grid z of conv_wgrad.hip's
 * LDS-tiled kernels): `d` = the forward descriptor of the whole layer, partial [S][Cout][taps][cin_pad] with S =
 * sf_conv_wgrad_grouped_splits(d, groups) (0: channels not divisible by groups); group g's rows are
 * [g Cout / G, (g + 1) Cout / G), so sf_conv_wgrad_finish(partial, S, Cout, taps, cin_pad, Cin / G, 0, dst, ...)
 * leaves nn.Conv3d's grouped parameter layout [Cout][Cin / G][kT][kH][kW].                                          */
int sf_conv_wgrad_grouped_splits(const sf_conv_desc* d, int groups);
int sf_conv_wgrad_grouped(const sf_conv_desc* d, int groups, const float* x, const float* dz, int dz_cs, int dz_coff,
                          float* partial, void* stream);
/* Sum the S split partials [S][Cout][packed_taps][cin_pad] in a fixed order and store / accumulate them in
 * nn.Conv3d's own layout dst[Cout][Cin][kT][kH][kW] (one pass, so the gradient can land directly in the
 * parameter's .grad).  fold_kw > 0: the stem layout, where a packed tap is (kt,kh) and a packed channel is
 * (kw, ci) = (c/4, c%4) (sf_conv_fwd over the NDHWC4 border-padded clip), Cin <= 4.                          */
int sf_conv_wgrad_finish(const float* partial, int S, int Cout, int packed_taps, int cin_pad, int Cin, int fold_kw,
                         float* dst, int accumulate, void* stream);

/* Training BatchNorm3d backward fused with ReLU mask (y > 0), residual fan-out (dres += g) and the sum over
 * `rep` nearest-upsampled copies:  g = sum_q dy * [y > 0];  dbeta = sum g;  dgamma = sum g * xhat;
 * dz = gamma * invstd * (g - dbeta/M - xhat * dgamma/M)  (dz may alias z).  ws: sf_bn_bwd_ws_floats(C).
 * relu: 0 none, 1 ReLU (y > 0), 2 ReLU6 (0 < y < 6), 3 = SF_BN_MASK_BYTES: `y` is the byte mask sf_affine_fwd_mask
 * left in the forward pass (cast to const float*; y_cs = C/4, y_coff = 0, rep = 1, float4-addressable views) — the
 * backward then reads 1/16 of the activation's bytes for the mask, twice.                                       */
#define SF_BN_MASK_BYTES 3
long sf_bn_bwd_ws_floats(int C);
/* sf_affine_fwd (below) for a ReLU / ReLU6 layer that also leaves mask[rows][C/4]: bit e of a byte says channel
 * 4i+e passes a gradient through the activation.  Flat float4 case only (C % 4 == 0, 16-byte addressable views, no
 * T repeat, no channel multiplier): SF_EINVAL otherwise.                                                        */
int sf_affine_fwd_mask(const float* x, int cs, int coff, int N, int T, int H, int W, int C, const float* scale,
                       const float* bias, const float* res, int res_cs, int res_coff, int act, float* out,
                       int out_cs, int out_coff, unsigned char* mask, void* stream);
int sf_bn_bwd_reduce(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff,
                     const float* z, int z_cs, int z_coff, int N, int T, int H, int W, int C, int rep, int relu,
                     const float* mean, const float* invstd, float* dbeta, float* dgamma, float* ws, void* stream);
/* As sf_bn_bwd_reduce, additionally accumulating dbeta_acc[c] += dbeta[c], dgamma_acc[c] += dgamma[c] (the
 * BatchNorm3d bias / weight .grad) in the same launch.                                                        */
int sf_bn_bwd_reduce_acc(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff,
                         const float* z, int z_cs, int z_coff, int N, int T, int H, int W, int C, int rep, int relu,
                         const float* mean, const float* invstd, float* dbeta, float* dgamma, float* ws,
                         float* dbeta_acc, float* dgamma_acc, void* stream);
int sf_bn_bwd_apply(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff,
                    const float* z, int z_cs, int z_coff, int N, int T, int H, int W, int C, int rep, int relu,
                    const float* mean, const float* invstd, const float* gamma, const float* dbeta,
                    const float* dgamma, float* dz, int dz_cs, int dz_coff, float* dres, int dres_cs,
                    int dres_coff, void* stream);
/* As sf_bn_bwd_apply with dres != NULL, but dres is WRITTEN (dres = g) instead of accumulated: the first writer of
 * the residual branch's gradient buffer needs neither a zero fill nor a read of it.                         */
int sf_bn_bwd_apply_first(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff,
                          const float* z, int z_cs, int z_coff, int N, int T, int H, int W, int C, int rep, int relu,
                          const float* mean, const float* invstd, const float* gamma, const float* dbeta,
                          const float* dgamma, float* dz, int dz_cs, int dz_coff, float* dres, int dres_cs,
                          int dres_coff, void* stream);
/* sf_bn_frozen_bwd: backward of an EVAL-mode BatchNorm3d epilogue under a training tape — the layers
 * misc.frozen_bn_stats (misc.py:246-254) has put into eval() while the model trains; torch.nn.BatchNorm3d eval
 * semantics: the running statistics are constants, gamma and beta stay trainable:
 *     y = act(gamma * (z - mean) * invstd + beta + res),  mean = running_mean, invstd = 1 / sqrt(running_var + eps),
 *     y repeated `rep` times along T;   g = sum_{q<rep} dy * m  (m: the activation's mask, as sf_bn_bwd_*: relu 0 / 1 /
 *     2 / SF_BN_MASK_BYTES);   dz = gamma * invstd * g  (gamma NULL: 1; dz may alias z);   dres (=|+=) g  (rep must be
 *     1; dres_accumulate == 0 writes every element: the first writer needs no zero fill);
 *     dbeta[c] += sum g;   dgamma[c] += sum g * (z - mean) * invstd.
 * dz does not depend on the sums, so ONE pass reads dy, the mask and z once, writes dz (and dres) and leaves per-block
 * partial sums in ws (sf_bn_bwd_ws_floats(C) floats); a second small kernel adds them in a fixed order in fp64 and
 * ACCUMULATES into dbeta / dgamma — zero-filled temporaries or the parameters' .grad.  dbeta == dgamma == NULL (a BN
 * without affine): dz and dres only, ws may be NULL.  Null pointers, non-positive sizes, a slice outside its pitch or
 * rep > 1 with dres return SF_EINVAL with nothing launched; 64-bit element offsets; float4 kernel when C, every pitch
 * and offset are multiples of 4 and dy, y, z, dz, dres are 16-byte aligned, scalar kernel otherwise; no atomics, one
 * owner per output element, fixed summation order: bitwise reproducible.                                          */
int sf_bn_frozen_bwd(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff,
                     const float* z, int z_cs, int z_coff, int N, int T, int H, int W, int C, int rep, int relu,
                     const float* mean, const float* invstd, const float* gamma, float* dz, int dz_cs, int dz_coff,
                     float* dres, int dres_cs, int dres_coff, int dres_accumulate, float* dbeta, float* dgamma,
                     float* ws, void* stream);

/* MaxPool3d backward (equality gather; dx accumulates).  `d` is the forward descriptor.                 */
int sf_maxpool_bwd(const sf_pool_desc* d, const float* x, const float* y, const float* dy, int dy_cs,
                   int dy_coff, float* dx, int dx_cs, int dx_coff, void* stream);
/* As sf_maxpool_bwd, but dx is WRITTEN (zero where a position won no window) instead of accumulated: the first
 * writer of the gradient buffer needs neither a zero fill nor a read of it.                                 */
int sf_maxpool_bwd_first(const sf_pool_desc* d, const float* x, const float* y, const float* dy, int dy_cs,
                         int dy_coff, float* dx, int dx_cs, int dx_coff, void* stream);

/* ECA backward: out[b,c] = sum_{t',hw} dz * max_r x (sf_tmax_dot), then
 * dx[frames holding the max] += dz * gate[b,c] + dpool[b,c]  (sf_eca_bwd_apply).  ws as sf_tmax_mean.   */
int sf_tmax_dot(const float* x, int cs, int coff, int N, int T, int H, int W, int C, int alpha, const float* dz,
                int dz_cs, int dz_coff, float* out, float* ws, void* stream);
int sf_eca_bwd_apply(const float* x, int cs, int coff, int N, int T, int H, int W, int C, int alpha,
                     const float* dz, int dz_cs, int dz_coff, const float* gate, const float* dpool, float* dx,
                     int dx_cs, int dx_coff, void* stream);

/* ECA's gate algebra on [N, C] vectors — backward of Conv1d(1,1,k=3,pad=1,bias=False) along the channel axis +
 * sigmoid (reference wdf_attention_helper.py:68-69, 83-88; replaces the F.conv1d / conv_transpose1d calls autograd
 * would make): gate = sigmoid(w3 (*) pooled), da = dg*gate*(1-gate), dpool = dpool_scale * convT(da, w3),
 * dw3[k] += sum da * shift_k(pooled).  dg = sf_tmax_dot's output; gate / dpool feed sf_eca_bwd_apply.        */
int sf_eca_gate_bwd(const float* dg, const float* pooled, const float* w3, int N, int C, float dpool_scale,
                    float* gate, float* dpool, float* dw3, void* stream);

/* Depthwise conv backward (`d` = forward descriptor, weights [taps][C]): dx accumulates; dw [taps][C] through
 * a fixed-count partial workspace (sf_dwconv_wgrad_ws_floats).                                           */
int sf_dwconv_dgrad(const sf_conv_desc* d, const float* dz, int dz_cs, int dz_coff, const float* w_packed,
                    float* dx, int dx_cs, int dx_coff, int C, void* stream);
long sf_dwconv_wgrad_ws_floats(const sf_conv_desc* d, int C);
int sf_dwconv_wgrad(const sf_conv_desc* d, const float* x, const float* dz, int dz_cs, int dz_coff, int C,
                    float* dw, float* ws, void* stream);
/* sf_dwconv_wgrad with the sum stored (accumulate == 0) or accumulated in the parameter's own layout
 * dw_param[C][1][kT][kH][kW] (nn.Conv3d(C, C, k, groups = C).weight): the gradient reaches .grad in the same launch. */
int sf_dwconv_wgrad_param(const sf_conv_desc* d, const float* x, const float* dz, int dz_cs, int dz_coff, int C,
                          float* dw_param, int accumulate, float* ws, void* stream);
/* out[r, c] (+)= in[r, in_coff + c*in_cmul]: backward of a channel-multiplier (shuffled) store.           */
int sf_gather_add(const float* in, int in_cs, int in_coff, int in_cmul, float* out, int out_cs, int out_coff,
                  long rows, int C, int accumulate, void* stream);

/* g[n, r, c] += v[n, c] * scale (global-mean backward);  out[r] = scale * <a[r,:], b[r,:]>;
 * out[r, c] (+)= alpha * a[r, c].                                                                       */
int sf_bcast_add(float* g, int cs, int coff, int N, long rows_per_n, int C, const float* v, float scale,
                 void* stream);
int sf_rowdot(const float* a, int a_cs, int a_coff, const float* b, int b_cs, int b_coff, long rows, int C,
              float scale, float* out, void* stream);
int sf_axpy(const float* a, int a_cs, int a_coff, float alpha, float* out, int out_cs, int out_coff, long rows,
            int C, int accumulate, void* stream);
/* ---- SubBatchNorm3d (batchnorm_helper.py:37-109): the batch is viewed as [N/S, S*C, T, H, W], i.e. sample n
 * belongs to split n % S and every split normalises with its own statistics (nn.BatchNorm3d(S*C, affine=False)).
 * The `_split` variants take nsplit = S and per-channel arrays of S*C entries indexed [split*C + c] (the layout of
 * split_bn.running_mean / running_var); with nsplit = 1 they are the plain functions above.  Requires N % S == 0
 * and N <= 1024.  sf_bn_bwd_apply_split divides by the rows of ONE split (M = N/S * T*H*W).                 */
int sf_bn_train_stats_split(const float* x, int cs, int coff, int N, long rows_per_sample, int C, int nsplit,
                            const float* gamma, const float* beta, float eps, float momentum, float* run_mean,
                            float* run_var, float* mean, float* var, float* invstd, float* scale, float* shift,
                            float* ws, void* stream);
int sf_affine_fwd_split(const float* x, int cs, int coff, int N, int T, int H, int W, int C, int nsplit,
                        const float* scale, const float* bias, const float* res, int res_cs, int res_coff, int act,
                        int rep, float* out, int out_cs, int out_coff, int out_cmul, void* stream);
int sf_bn_bwd_reduce_split(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff,
                           const float* z, int z_cs, int z_coff, int N, int T, int H, int W, int C, int nsplit,
                           int rep, int relu, const float* mean, const float* invstd, float* dbeta, float* dgamma,
                           float* ws, void* stream);
int sf_bn_bwd_apply_split(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff,
                          const float* z, int z_cs, int z_coff, int N, int T, int H, int W, int C, int nsplit,
                          int rep, int relu, const float* mean, const float* invstd, const float* gamma,
                          const float* dbeta, const float* dgamma, float* dz, int dz_cs, int dz_coff, float* dres,
                          int dres_cs, int dres_coff, void* stream);
/* dx[r, c] (+)= dy[r, c] * [0 < y[r, c] (< 6)]: backward of a bare nn.ReLU / nn.ReLU6 (act = SF_ACT_RELU |
 * SF_ACT_RELU6) that has no BN in front of it, e.g. relu(cat([out, shortcut(x)])) in the ShuffleNet v1
 * Bottleneck (shufflenet_helper.py:76-77); the mask is taken from the activation's OUTPUT y.            */
int sf_act_bwd(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff, int act, float* dx,
               int dx_cs, int dx_coff, long rows, int C, int accumulate, void* stream);

/* ---- Nonlocal block core (nonlocal_helper.py:105-148).  The score matrix theta^T phi of ONE sample is small here
 * (N_q <= 6272 queries x N_k <= 1568 max-pooled keys, d = 256 / 512), so it is materialised by sf_conv_fwd with the
 * sample's phi rows as the "weights" ([N_k][d] is already the packed layout), normalised in place by the kernels
 * below ("softmax": softmax(scale * s) over the keys; "dot_product" needs no kernel: 1/N_k in the GEMM epilogue),
 * and multiplied by g with a second sf_conv_fwd (weights = g^T).  x / dp: rows of C = N_k scores, pitch cs.       */
int sf_row_softmax_fwd(float* x, int cs, int coff, long rows, int C, float scale, void* stream);
/* dp <- scale * p * (dp - <p, dp>)  (gradient w.r.t. the un-scaled scores, in place over dL/dp)                 */
int sf_row_softmax_bwd(const float* p, int p_cs, int p_coff, float* dp, int dp_cs, int dp_coff, long rows, int C,
                       float scale, void* stream);

/* ---- action-detection head (ResNetRoIHead, head_helper.py:11-130; models wire it at video_model_builder.py:349-371,
 * :570-580 and custom_video_model_builder.py:378-400).  detectron2 ROIAlign semantics (spatial_scale, sampling_ratio 0,
 * aligned) and the max-pool's first-maximum rule are spelled out in csrc/roi_head.hip.
 * sf_roi_tpool_fwd: s{p}_tpool = AvgPool3d([T,1,1], stride 1) + squeeze(2) (head_helper.py:96-100, T_out == 1):
 *   x [N,T,H,W] channel slice (cs, coff) -> out [N,H,W,C] dense.
 * sf_roi_align_max_fwd: s{p}_roi + s{p}_spool (head_helper.py:102-106): map [N,H,W,C] dense, boxes [K,5] fp32 on the
 *   device, rows (batch_idx, x1, y1, x2, y2) in input pixels -> out[k, out_coff + c] (the pathway's slice of the
 *   concat buffer, pitch out_cs) and arg[k, c] = winning bin (row-major, < R*R <= 256).  A box whose batch index does
 *   not truncate into [0, N) reads nothing and yields 0.  K == 0 launches nothing.
 * sf_roi_align_max_bwd: dx[n, t, h, w] (+)= (1/T) dL/d(map)[n, h, w]: the RoIAlign / max-pool backward fused with the
 *   temporal broadcast (T = 1: the map's own gradient).  Gather form: each element walks the boxes of its clip in
 *   index order, so the result is bitwise reproducible (no atomics).  accumulate == 0 overwrites every element.
 * sf_sigmoid_bwd: dx (+)= dy * y * (1 - y) over n dense elements (head_helper.py:125, nn.Sigmoid's backward).   */
int sf_roi_tpool_fwd(const float* x, int cs, int coff, int N, int T, int H, int W, int C, float* out, void* stream);
int sf_roi_align_max_fwd(const float* x, int N, int H, int W, int C, const float* boxes, int K, int R,
                         float spatial_scale, int aligned, float* out, int out_cs, int out_coff, unsigned char* arg,
                         void* stream);
int sf_roi_align_max_bwd(const float* dy, int dy_cs, int dy_coff, const unsigned char* arg, const float* boxes, int K,
                         int N, int T, int H, int W, int C, int R, float spatial_scale, int aligned, float* dx,
                         int dx_cs, int dx_coff, int accumulate, void* stream);
int sf_sigmoid_bwd(const float* y, const float* dy, float* dx, long n, int accumulate, void* stream);

/* ---- fully-convolutional classification head (csrc/head_pool.hip): ResNetBasicHead's nn.AvgPool3d(pool_size, stride=1)
 * per pathway (head_helper.py:174-179) and its concatenation (head_helper.py:203-207) when the window is smaller than
 * res5 — the driver-monitoring YAMLs' RESNET.SPATIAL_STRIDES [[1,1],[1,1],[2,2],[2,2]]: a crop//32 window over a
 * crop/16 map — and autograd's backward of that pool.  d: is_avg = 1, strides 1, padding 0, kT <= Ti (H, W likewise),
 * To = Ti - kT + 1 (H, W likewise), divisor kT * kH * kW.  Null pointers, non-positive dims, a window larger than the
 * input, any other stride / padding / output extent or a channel slice outside its pitch: SF_EINVAL, nothing launched.
 * sf_avgpool_win_fwd: x channel slice (d->in_cs, d->in_coff) -> out[n,to,ho,wo, d->out_coff + c], the pathway's slice
 *   of the concat buffer (pitch d->out_cs); channels outside the slice are not touched.  The window's frames are
 *   summed first and that plane is box-filtered from LDS, so x is read once; a plane of more than 2048 positions
 *   (8192 on the scalar path) goes to sf_pool_fwd's kernel instead.
 * sf_avgpool_win_bwd: dx[n,t,h,w, dx_coff + c] (+)= 1/|k| * sum of dy[n,to,ho,wo, dy_coff + c] over to in
 *   [max(0, t-kT+1), min(To-1, t)] (ho, wo likewise); d's own pitches / offsets are not read.  overwrite != 0: every
 *   element of dx's slice is written (no zero fill, no read: the first writer of the gradient), else accumulated.
 *   To == 1: the sum is formed once per (n, h, w, c) and stored to all Ti frames.
 * Both: float4 kernels when C, both pitches and both offsets are multiples of 4 and both pointers 16-byte aligned,
 * scalar kernels otherwise; fixed summation order and one owner per output element (no atomics): bitwise reproducible. */
int sf_avgpool_win_fwd(const sf_pool_desc* d, const float* x, float* out, void* stream);
int sf_avgpool_win_bwd(const sf_pool_desc* d, const float* dy, int dy_cs, int dy_coff, float* dx, int dx_cs,
                       int dx_coff, int overwrite, void* stream);

/* ---- input step (datasets/kinetics.py:230-248 -> datasets/utils.py:298-315 tensor_normalize, :151-203
 * spatial_sampling, :73-112 pack_pathway_output; transform.py:283-337 / 359-393 / 395-423 / 425-468).
 * clip: ONE decoded clip, uint8 [T,H,W,3] on the device.  The short side is scaled bilinearly to (new_h, new_w)
 * (== (H, W): no resampling), a crop x crop window at (y0, x0) of the scaled frame is taken, optionally mirrored,
 * normalised as (u/255 - mean)/std, channel-reversed if asked, and the frames frame_idx[0..n_frames) (device ints;
 * NULL = all T frames) are written to dst [n_frames][crop+2ph][Wp][4]: the stems' NDHWC layout with the channel
 * padded to 4 and zero borders, so the stem convolution consumes it without a layout pass.  mean3/std3: HOST.   */
int sf_clip_prologue(const unsigned char* clip, int T, int H, int W, int new_h, int new_w, int y0, int x0, int crop,
                     int flip, int reverse, const float* mean3, const float* std3, const int* frame_idx,
                     int n_frames, float* dst, int ph, int pw, int Wp, void* stream);

/* One-channel (grayscale) clips, uint8 [T,H,W] (the fork's configs/TIRED, configs/WHEEL: DATA.INPUT_CHANNEL_NUM [1],
 * MEAN [0.45], STD [0.225]): the same arithmetic with a scalar mean / std, written to the ONE-channel stem layout
 * dst [n_frames][crop+2ph][Wp] (one float per pixel, zero borders).                                               */
int sf_clip_prologue_gray(const unsigned char* clip, int T, int H, int W, int new_h, int new_w, int y0, int x0,
                          int crop, int flip, float mean, float stdv, const int* frame_idx, int n_frames, float* dst,
                          int ph, int pw, int Wp, void* stream);

/* ---- multi-view testing (tools/test_net.py: TEST.NUM_ENSEMBLE_VIEWS x TEST.NUM_SPATIAL_CROPS views per video,
 * datasets/kinetics.py:166-181 and decoder.py:35-83 decide which frames and which crop a view takes).
 * sf_clip_views: ALL V views of ONE decoded video, uint8 [T,H,W,3] on the device, for both pathways in one launch.
 *   The view table is V rows (new_h, new_w, y0, x0, flip), then V * n_fast frame indices (view-major), then the
 *   n_slow Fast-frame positions the Slow pathway takes (datasets/utils.py:96-104; strictly increasing), all int32.
 *   `table` is its device copy and `table_host` the host array it was uploaded from: the host copy is checked before
 *   anything is launched, the kernel reads the device copy (a device row that fails the same check writes zeros).
 *   fast [V][n_fast][crop+2ph][Wp][4] and slow [V][n_slow][crop+2ph][Wp][4] are the layouts sf_clip_prologue writes,
 *   zero borders included, and hold the same bits: the pixel arithmetic is one device function.  Slow frame j of a
 *   view is its Fast frame number table[slow j]; a frame that goes to both pathways is resampled once and stored twice.
 *   slow == NULL with n_slow == 0: a single-pathway model.  One owner per output element, 16-byte stores, 64-bit
 *   element offsets, no atomics.
 *   SF_EINVAL, nothing launched: null pointers, V <= 0, non-positive sizes, a crop window outside its scaled frame, a
 *   frame index outside [0, T), n_slow > n_fast, Slow positions outside [0, n_fast) or not increasing, slow given
 *   without n_slow (or the reverse), Wp < crop + 2 pw, V or n_fast above 65535, buffers not 16-byte aligned.
 * sf_clip_views_gray: the same for a one-channel video, uint8 [T,H,W]: one float per pixel ([V][n][crop+2ph][Wp]);
 *   four pixels per 16-byte store when Wp % 4 == 0 and both buffers are 16-byte aligned, one pixel per store otherwise. */
int sf_clip_views(const unsigned char* video, int T, int H, int W, const int* table_host, const int* table, int V,
                  int n_fast, int n_slow, int crop, int reverse, const float* mean3, const float* std3, float* fast,
                  float* slow, int ph, int pw, int Wp, void* stream);
int sf_clip_views_gray(const unsigned char* video, int T, int H, int W, const int* table_host, const int* table, int V,
                       int n_fast, int n_slow, int crop, float mean, float stdv, float* fast, float* slow, int ph,
                       int pw, int Wp, void* stream);

/* ---- training input step, one launch per batch (datasets/kinetics.py:146-165 short-cycle crop and jitter, :186-189
 * sampling rate, :230-248 normalise / spatial_sampling / pack_pathway_output; decoder.py:55-83 random temporal window,
 * :35-52 temporal_sampling, :449 the span; datasets/utils.py:318-327 get_random_sampling_rate).
 * sf_clip_batch: ALL B clips of ONE training batch, for both pathways in one launch.  The B decoded spans are separate
 *   device allocations, uint8 [T_i,H_i,W_i,3], each with its own scale, crop and flip.  The batch table is B rows
 *   (clip device address, T_i, H_i, W_i, new_h, new_w, y0, x0, flip), then B * n_fast frame indices into each clip's
 *   own span (clip-major; this is temporal_sampling's gather), then the n_slow Fast-frame positions the Slow pathway
 *   takes (shared by the batch, strictly increasing), all int64.  `table` is its device copy and `table_host` the host
 *   array it was uploaded from: the host copy is checked before anything is launched, the kernel reads the device copy
 *   and re-checks its row — a device row that fails (zero address, non-positive or over-int extents, crop window
 *   outside its scaled frame) writes zeros for that clip, and a device frame index is clamped into [0, T_i).
 *   fast [B][n_fast][crop+2ph][Wp][4] and slow [B][n_slow][crop+2ph][Wp][4] are the layouts sf_clip_prologue writes,
 *   zero borders included, and hold the same bits: the pixel arithmetic is one device function.  A frame that goes to
 *   both pathways is resampled once and stored twice.  slow == NULL with n_slow == 0: a single-pathway model.  One
 *   owner per output element, 16-byte stores, 64-bit element offsets, no atomics.
 *   SF_EINVAL, nothing launched: null pointers, B <= 0, non-positive sizes, a zero clip address in the host table, a
 *   crop window outside its scaled frame, a frame index outside [0, T_i), n_slow > n_fast, Slow positions outside
 *   [0, n_fast) or not increasing, slow given without n_slow (or the reverse), Wp < crop + 2 pw, B or n_fast above
 *   65535, buffers not 16-byte aligned.  mean3 / std3: HOST.
 * sf_clip_batch_gray: the same for one-channel spans, uint8 [T_i,H_i,W_i]: one float per pixel ([B][n][crop+2ph][Wp]);
 *   four pixels per 16-byte store when Wp % 4 == 0 and both buffers are 16-byte aligned, one pixel per store otherwise
 *   (buffers that are not float-aligned: SF_EINVAL). */
int sf_clip_batch(const long* table_host, const long* table, int B, int n_fast, int n_slow, int crop, int reverse,
                  const float* mean3, const float* std3, float* fast, float* slow, int ph, int pw, int Wp,
                  void* stream);
int sf_clip_batch_gray(const long* table_host, const long* table, int B, int n_fast, int n_slow, int crop, float mean,
                       float stdv, float* fast, float* slow, int ph, int pw, int Wp, void* stream);

/* ---- mixup / CutMix inside the training input step (upstream SlowFast datasets/mixup.py: MixUp._mix_batch mixes the
 * collated float batch with its flip along the batch axis — x * lam + x.flip(0) * (1 - lam), or the flipped batch's
 * pixels inside one box).  Here a mixed pixel is one or two resamples of uint8 spans: no float batch is read back.
 * A MIX ROW is SF_MIX_ROW = 7 int64: partner row, mode (0 none, 1 mixup, 2 CutMix), lam as a float32 bit pattern in
 *   the low 32 bits (the high 32 zero), then the box y0, x0, y1, x1 in output (post-flip) crop coordinates.  A row is
 *   valid when the partner lies in [0, B), the mode in {0, 1, 2} and lam in [0, 1]; its box when 0 <= y0 <= y1 <= crop
 *   and 0 <= x0 <= x1 <= crop.  sf_ce_mix (below) reads the same rows.
 * sf_clip_batch_mix: sf_clip_batch whose table carries a tail: after the B rows, the frame indices and the Slow
 *   positions come B mix rows.  For output pixel (yy, xx) of frame f of clip b with partner p:
 *   mode 0: the pixel of clip b — sf_clip_batch's bits.
 *   mode 1: fl(fl(lam * own) + fl(fl(1.0f - lam) * other)) per channel — two rounded products and a rounded sum, never
 *           contracted into an fma: the bits of mixing the two sf_clip_batch outputs with separate float32 multiplies
 *           and an add.  `other` is clip p through ITS row (scale, crop offset, flip) and ITS frame index f.
 *   mode 2: clip p's pixel where y0 <= yy < y1 and x0 <= xx < x1, clip b's elsewhere, in every frame of both pathways:
 *           one resample per pixel, as without mixing.
 *   Borders stay zero, a frame that goes to both pathways is mixed once and stored twice, one owner per output
 *   element, 16-byte stores, no atomics.  The kernel re-checks the device rows it reads: clip b is written as zeros
 *   when its own or its partner's batch row fails sf_clip_batch's check, or its mix row or box is not valid.
 *   SF_EINVAL, nothing launched: sf_clip_batch's list, or a mix row or a box of the host table that is not valid.
 * sf_clip_batch_mix_gray: the same for one-channel spans, with both store widths of sf_clip_batch_gray. */
#define SF_MIX_ROW 7
int sf_clip_batch_mix(const long* table_host, const long* table, int B, int n_fast, int n_slow, int crop, int reverse,
                      const float* mean3, const float* std3, float* fast, float* slow, int ph, int pw, int Wp,
                      void* stream);
int sf_clip_batch_mix_gray(const long* table_host, const long* table, int B, int n_fast, int n_slow, int crop,
                           float mean, float stdv, float* fast, float* slow, int ph, int pw, int Wp, void* stream);

/* ---- Jester's colour jitter inside the training input step (datasets/decoder.py:456-469: decode(..., jester=True)
 * draws brightness, contrast and colour factors per clip and passes every sampled frame through
 * transform.RandomColorJitter, datasets/transform.py:692-717 — PIL's ImageEnhance.Brightness, then Contrast, then
 * Color — before tensor_normalize).  Here the jitter acts on each uint8 source pixel a resampling tap reads: no frame
 * goes back to the host.  The arithmetic is PIL's (checked against Pillow 12.2.0), bit for bit:
 *   blend(f, x0, x1) = fl(x0 + fl(f * (x1 - x0))) in float32 — f is the factor as a C float, one rounded product and
 *     one rounded sum, never an fma — truncated toward zero for 0 <= f <= 1, else clipped to [0, 255] and truncated;
 *   grey(c) = (19595 c0 + 38470 c1 + 7471 c2 + 32768) >> 16 (channel 0 is R);
 *   brightness: c_i <- blend(fb, 0, c_i); contrast: c_i <- blend(fc, m, c_i) with m the frame's grey mean; colour:
 *     c_i <- blend(fs, grey(c), c_i); in that order, a stage with a factor <= 0 skipped;
 *   m = (2 S + n) / (2 n) in integers, S the sum of grey(.) of the brightness-jittered pixels over the WHOLE decoded
 *     H x W frame (n = H * W), which is int(ImageStat.Stat(L).mean[0] + 0.5).  m belongs to a frame, the factors to a clip.
 * A JITTER ROW is SF_JITTER_ROW = 3 int64: the brightness, contrast and colour factors, each a float32 bit pattern in
 *   the low 32 bits (the high 32 zero); valid when all three are finite.  The table is sf_clip_batch's (B rows,
 *   B * n_fast frame indices, n_slow Slow positions) followed by B jitter rows.
 * sf_frame_grey_means: means[b * n_fast + f] (device int32) = the grey mean of clip b's source frame frame_idx[b][f]
 *   after clip b's brightness stage.  One workgroup per (clip, Fast frame), an integer reduction in registers and LDS
 *   with a 64-bit sum, one owner per element, no atomics; aligned 12-byte loads between a byte-wise head and tail.  A
 *   clip whose contrast factor is <= 0 gets 0 for its frames without a read; so does a device row that fails
 *   sf_clip_batch's row check (with no crop window) or whose factors are not finite.
 *   SF_EINVAL, nothing launched: what sf_clip_batch asks of the table (the crop window aside), a factor word of the
 *   host table that is not a finite float32 with a zero high half, `means` null or not 4-byte aligned.
 * sf_clip_batch_jitter: the means launch into `means` (int32 [B][n_fast], device, need not be initialised), then ONE
 *   clip launch of sf_clip_batch's shape — same grid, 16-byte stores, zero borders, a frame that goes to both pathways
 *   computed once and stored twice — whose every tap goes through the jitter before u / 255.  A clip whose three
 *   factors are all <= 0 holds sf_clip_batch's bits.  Clip b is written as zeros when its device batch row or its
 *   device jitter row fails the check.  RGB only: ImageEnhance.Color leaves a one-channel image as it is, and Jester is RGB.
 *   SF_EINVAL, nothing launched: sf_clip_batch's list, a factor word of the host table that is not valid, `means` null
 *   or not 4-byte aligned.  mean3 / std3: HOST. */
#define SF_JITTER_ROW 3
int sf_frame_grey_means(const long* table_host, const long* table, int B, int n_fast, int n_slow, int* means,
                        void* stream);
int sf_clip_batch_jitter(const long* table_host, const long* table, int B, int n_fast, int n_slow, int crop,
                         int reverse, const float* mean3, const float* std3, int* means, float* fast, float* slow,
                         int ph, int pw, int Wp, void* stream);

/* ---- detection input step, one launch per batch (AVA with AVA.IMG_PROC_BACKEND "pytorch":
 * datasets/ava_dataset.py:233-338 _images_and_boxes_preprocessing and the transform.py functions it calls — :283-337
 * random_short_side_scale_jitter, :359-392 random_crop, :395-422 horizontal_flip, :425-468 uniform_crop, :636-663
 * lighting_jitter, :666-688 color_normalization; datasets/utils.py:73-112 pack_pathway_output).
 * sf_clip_batch_det: ALL B clips of ONE detection batch, for both pathways in one launch.  The B frame spans are
 *   separate device allocations, uint8 [T_i,H_i,W_i,3] in BGR order.  The batch table is B rows (clip device address,
 *   T_i, H_i, W_i, new_h, new_w, y0, x0, flip, and the three PCA-lighting offsets as float32 bit patterns in the order
 *   they are added to source channels 0..2), then B * n_fast frame indices (clip-major), then the n_slow Fast-frame
 *   positions the Slow pathway takes (strictly increasing), all int64; anything behind that is not read.  `table` is
 *   the device copy and `table_host` the host array it was uploaded from: the host copy is checked before anything is
 *   launched, the kernel reads the device copy and re-checks its row — a device row that fails writes zeros for that
 *   clip, and a device frame index is clamped into [0, T_i).
 *   The arithmetic is the AVA loader's, in its order, in fp32: u / 255 per tap, torch's bilinear resample
 *   (align_corners=False; none when (new_h, new_w) == (H_i, W_i)), crop at (y0, x0) and flip inside the window,
 *   + offset[c], (. - mean3[c]) / std3[c] with true divides (mean3 / std3 in source, BGR, order), and with `reverse`
 *   (AVA.BGR False) the channels are stored 2, 1, 0.  This is not sf_clip_batch's arithmetic, which normalises first.
 *   The output window is win_h x win_w, shared by the batch; the `test` split takes no crop, so it need not be square.
 *   fast [B][n_fast][win_h+2ph][Wp][4] and slow [B][n_slow][win_h+2ph][Wp][4]: the stems' layout, borders and the pad
 *   channel zero.  A frame that goes to both pathways is computed once and stored twice.  slow == NULL with
 *   n_slow == 0: a single-pathway model.  One owner per output element, 16-byte stores, 64-bit element offsets, no
 *   atomics.
 *   SF_EINVAL, nothing launched: sf_clip_batch's list (null pointers, B <= 0, non-positive sizes, a zero clip address,
 *   a frame index outside [0, T_i), n_slow > n_fast, Slow positions outside [0, n_fast) or not increasing, slow given
 *   without n_slow or the reverse, B or n_fast above 65535, buffers not 16-byte aligned), the window outside the
 *   scaled frame in either dimension, Wp < win_w + 2 pw, and a lighting offset in the host table that is not a finite
 *   float32.  mean3 / std3: HOST. */
int sf_clip_batch_det(const long* table_host, const long* table, int B, int n_fast, int n_slow, int win_h, int win_w,
                      int reverse, const float* mean3, const float* std3, float* fast, float* slow, int ph, int pw,
                      int Wp, void* stream);

/* ---- streaming demo (csrc/stream.hip): tools/demo_net.py:160-305 with the frame buffer on the device.  The reference
 * keeps a Python list of the last S = DATA.NUM_FRAMES * DATA.SAMPLING_RATE scaled frames and rebuilds, normalises,
 * permutes, index_selects and uploads all of them for every incoming frame.  Here they live in a ring
 * [S][new_h + 2 ph][Wp][4] of fp32 in the layout sf_clip_prologue writes (channels padded to 4, zero borders, row pitch
 * Wp); no entry allocates or synchronises.
 * sf_stream_push (demo_net.py:166-169 cv2.cvtColor + cv2_transform.scale, :193-198 tensor_normalize + permute, for ONE
 *   frame): frame is uint8 [H,W,3] on the device in the camera's BGR order.  It is scaled bilinearly to (new_h, new_w)
 *   (== (H, W): no resampling) and normalised as (u/255 - mean)/std with sf_clip_prologue's arithmetic (one device
 *   function: the slot holds the bits sf_clip_prologue gives for the channel-swapped frame with its window on the whole
 *   scaled frame), B and R swapped on the read, and written to slot `slot` of the ring — the whole padded plane, zeros
 *   included, one 16-byte store per pixel.  mean3 / std3: HOST, three floats each, in RGB order (DATA.MEAN / DATA.STD).
 *   SF_EINVAL, nothing launched: null pointers, non-positive sizes or S, slot outside [0, S), negative ph / pw,
 *   Wp < new_w + 2 pw, a plane of more than 2^29 pixels, ring not 16-byte aligned.
 * sf_stream_window (demo_net.py:204-221 the two linspace index_selects, :232-238 the upload): both pathways of the
 *   window whose oldest frame is in slot `head`, in one launch.  fast_idx: n_fast window positions in [0, S), slow_idx:
 *   n_slow positions among the Fast frames, both int32 in DEVICE memory.  fast [n_fast][Hp][Wp][4] frame j is ring slot
 *   (head + fast_idx[j]) % S; slow [n_slow][Hp][Wp][4] frame j is Fast frame slow_idx[j].  Hp = new_h + 2 ph.  A pure
 *   copy: one 16-byte load per pixel of a Fast frame, stored to fast and — when slow_idx names the frame — to slow.
 *   The tables are read on the device only: a fast_idx entry outside [0, S) or a slow_idx entry outside [0, n_fast)
 *   makes that frame zeros, never a wild read, and every element of both buffers still has exactly one owner.
 *   slow == NULL with n_slow == 0: a single-pathway model.
 *   SF_EINVAL, nothing launched: null ring / fast_idx / fast, S <= 0, head outside [0, S), n_fast <= 0 or above 65535,
 *   n_slow < 0 or > n_fast, slow given without n_slow (or the reverse), n_slow > 0 without slow_idx, non-positive Hp /
 *   Wp, a plane of more than 2^29 pixels, a buffer not 16-byte aligned.
 * sf_label_select (demo_net.py:264-268 and :292-298 torch.nonzero(preds > 0.1) + .cpu(), :289 argmax): preds [R][C]
 *   fp32 (R = 1 for classification, the number of boxes for detection) -> out int32 [R][2 + C]: per row count, argmax,
 *   then the `count` class indices with preds > thr in ascending order; entries past 2 + count are not written.  argmax
 *   is the first maximal index (torch.argmax).  A NaN is never selected and never wins: a row of NaNs gives count 0,
 *   argmax -1.  One wavefront per row, any C; order from ballot + popcount, no atomics, no LDS.
 *   SF_EINVAL, nothing launched: null pointers, R <= 0, C <= 0, a NaN threshold, a pointer off 4 bytes. */
int sf_stream_push(const unsigned char* frame, int H, int W, int new_h, int new_w, const float* mean3, const float* std3,
                   float* ring, int S, int slot, int ph, int pw, int Wp, void* stream);
int sf_stream_window(const float* ring, int S, int head, const int* fast_idx, int n_fast, const int* slow_idx, int n_slow,
                     float* fast, float* slow, int Hp, int Wp, void* stream);
int sf_label_select(const float* preds, int R, int C, float thr, int* out, void* stream);

/* sf_ensemble_update (csrc/ensemble.hip): TestMeter.update_stats (utils/meters.py:283-317) on the device.  preds [B,K],
 *   video_idx int32 [B] (clip id / clips per video), labels int32 [B] or NULL; video_preds [Nv,K], video_labels int32
 *   [Nv], clip_count int32 [Nv] are the meter's accumulators.  mode 0: video_preds[video_idx[b]] += preds[b]; mode 1:
 *   the elementwise maximum.  The first clip of a video in the batch owns that video's row for the call and folds the
 *   batch in index order: the sum equals the host loop's bit for bit (no atomics).  video_labels takes the label of the
 *   video's last clip in the batch, clip_count the number of its clips.  A video_idx outside [0, Nv) is skipped and
 *   added to *bad_count (device int32).  Null pointers (labels excepted), non-positive sizes, another mode: SF_EINVAL. */
int sf_ensemble_update(const float* preds, const int* video_idx, const int* labels, float* video_preds,
                       int* video_labels, int* clip_count, int* bad_count, int B, int K, int Nv, int mode,
                       void* stream);
/* sf_ensemble_update_ml (csrc/ensemble.hip): the multi-label TestMeter.update_stats (utils/meters.py:290-310) on the
 *   same owner rule and fold.  labels fp32 [B,K] with row stride ldl >= K, video_labels fp32 [Nv,K].  The owner of a
 *   video walks its clips in batch order as the host loop does: when the row the video holds (the stored one, then the
 *   previous clip's) has a positive sum and differs from the clip's row — the reference's `assert torch.equal`,
 *   :292-296 — one mismatch is added to bad_count[1]; the last clip's whole row is then stored.  bad_count is int32 [2]:
 *   {clips with a video outside [0, Nv), label mismatches}.  Null pointers, non-positive sizes, ldl < K, another mode:
 *   SF_EINVAL. */
int sf_ensemble_update_ml(const float* preds, const int* video_idx, const float* labels, int ldl, float* video_preds,
                          float* video_labels, int* clip_count, int* bad_count, int B, int K, int Nv, int mode,
                          void* stream);

/* ---- one-channel stem (csrc/conv_stem_gray.hip): nn.Conv3d(1, Cout, [kT,7,7], stride [1,2,2], padding [pT,3,3]) of
 * ResNetBasicStem (stem_helper.py:157-164) and its weight gradient (autograd's conv backward for `conv.weight`) on
 * the one-channel layout x [N][T][Hp][Wp] fp32, Hp = H + 2*3, zero H/W borders, Wp as for the RGB stem layout — what
 * sf_ncthw1_pack makes of an [N,1,T,H,W] tensor (the permute the reference never needs: it convolves NCTHW) and
 * sf_clip_prologue_gray of a decoded clip.  Output extents: To = T + 2 pT - kT + 1, Ho = (Hp - 7)/2 + 1,
 * Wo = (Wp - 7)/2 + 1.  Weights w / dw are in the parameter's layout [Cout][1][kT][7][7].
 * Range: Cout in {8, 16, 64}, kT <= 5, and a one-output-row band (7 kT input rows + the weights, forward; + that row's
 * dz, weight gradient) that fits 128 KB of LDS — bands are sized for 64 KB (two workgroups per CU) where they can be
 * (sf_stem1_accepts == 1; host only);
 * anything else returns SF_ENOTTAKEN and launches nothing.
 * sf_stem1_fwd:  out[n,t,ho,wo, out_coff + co] = act(scale[co] * z + bias[co]) (scale / bias may be NULL: 1 / 0).
 * sf_stem1_wgrad: dw (+)= sum over positions of dz * x.  Per-workgroup partial sums go to ws
 *   (sf_stem1_wgrad_ws_floats floats, caller-owned) and are added in workgroup order: no atomics, bitwise
 *   reproducible.  accumulate == 0 overwrites dw.                                                                */
int sf_stem1_accepts(int Hp, int Wp, int Cout, int kT);
int sf_stem1_fwd(const float* x, int N, int T, int Hp, int Wp, const float* w, int Cout, int kT, int pT,
                 const float* scale, const float* bias, int act, float* out, int out_cs, int out_coff, void* stream);
long sf_stem1_wgrad_ws_floats(int N, int T, int Hp, int Wp, int Cout, int kT, int pT);
int sf_stem1_wgrad(const float* x, int N, int T, int Hp, int Wp, const float* dz, int dz_cs, int dz_coff, int Cout,
                   int kT, int pT, float* dw, int accumulate, float* ws, void* stream);
int sf_ncthw1_pack(const float* src, float* dst, int N, int T, int H, int W, int ph, int pw, int Wp, void* stream);

/* ---- Grad-CAM (csrc/gradcam.hip): the arithmetic of wdf_visualization/gradcam_video.py's GradVideoCam on the eval
 * forward — the gradient of one class score with respect to a top-level child's output (gradcam_video.py:143-157:
 * a one-hot vector back-propagated from the head's eval output) and the per-frame class-activation maps
 * (gradcam_video.py:159-179).  Only ACTIVATION gradients: no entry here touches a parameter's gradient.
 * All of them: null pointers, non-positive sizes or a channel slice outside its pitch return SF_EINVAL with nothing
 * launched; 64-bit element indices; one owner per output element and a fixed summation order (no atomics): bitwise
 * reproducible.
 *
 * sf_epilogue_bwd: backward of the folded eval epilogue of sf_conv_fwd / sf_affine_fwd,
 *     y = relu?(scale[c] * z + bias[c] + res), y repeated `rep` times along T (nn.Upsample nearest,
 *     custom_video_model_builder.py:120-121):
 *   dz[n,t,h,w,c] (=|+=) scale[c] * sum_{r<rep} dy[n, t*rep + r, h,w,c] * m,  m = [y[n, t*rep + r, h,w,c] > 0] when
 *   relu != 0, else 1 (y is then not read and may be NULL); scale NULL means 1.  T is dz's frame count; dy and y hold
 *   T * rep frames.  dres != NULL (rep must be 1): dres (=|+=) dy * m in the same pass — the residual branch's
 *   gradient.  dz_accumulate / dres_accumulate == 0: every element of the slice is written (no zero fill needed).
 *   dy and y are read once.  float4 kernel when C, every pitch and offset are multiples of 4 and every pointer is
 *   16-byte aligned, scalar kernel otherwise.
 * sf_head_act_mean_bwd: backward of sf_head_act_mean (head_helper.py:217-221), out[b,k] = mean_p act(logits[b,p,:])[k]:
 *   given dout [B,K],  softmax: dl[b,p,k] = s[p,k] * (dout[k] - sum_j dout[j] * s[p,j]) / P;  sigmoid:
 *   s (1 - s) dout[k] / P;  relu: [l > 0] dout[k] / P;  none: dout[k] / P.  The activation is recomputed from the
 *   logits (max-subtracted softmax, as sf_head_act_mean); any K >= 1.  accumulate != 0 adds to dl.
 * sf_cam_weights: w[n,t,c] = mean_{h,w} g[n,t,h,w, g_coff + c]  (gradcam_video.py:159-166), w dense [N*T, C].
 * sf_cam_map: abar[n,h,w,c] = mean_t a[n,t,h,w, a_coff + c] (written to ws, sf_cam_map_ws_floats floats),
 *   raw[n,t,h,w] = max(0, 1 + sum_c w[n,t,c] * abar[n,h,w,c]) (optional output, may be NULL),
 *   cam[n,t,h,w] = (raw - min) / (max - min) over the frame (n,t)  (gradcam_video.py:167-179); a frame whose range is
 *   zero gives zeros (the reference divides by zero there).  The normalisation is taken of max(-1, sum) — the same
 *   map less its constant 1, summed from 0 — so a nearly flat map (sum of order 1e-3) is not first rounded at the
 *   magnitude of the 1.  Two launches.                                                                             */
int sf_epilogue_bwd(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff, int N, int T, int H,
                    int W, int C, int rep, const float* scale, int relu, float* dz, int dz_cs, int dz_coff,
                    int dz_accumulate, float* dres, int dres_cs, int dres_coff, int dres_accumulate, void* stream);
/* sf_epilogue_bwd_act: sf_epilogue_bwd for the efficient backbones' epilogues (gradcam_video.py:143-157 back-propagates
 * through them when the target is a child of SlowFastShuffleNet / SlowFastMoibleNetV2).
 *   act is an activation CODE: SF_ACT_NONE, SF_ACT_RELU or SF_ACT_RELU6 (nn.ReLU6, mobilenetv2_helper.py:30-68); the
 *   mask is taken from the output y as sf_act_bwd takes it: m = [0 < y], and [0 < y < 6] for ReLU6.
 *   groups > 1 undoes the channel-shuffled store of sf_conv_fwd_grouped(shuffle = 1) (channel_shuffle behind the
 *   grouped conv1 of shufflenet_helper.py:22-79): dz channel g * (C / groups) + j reads dy and y at channel
 *   j * groups + g; scale is indexed by the dz channel.  It requires rep == 1, dres == NULL and C % groups == 0
 *   (SF_EINVAL otherwise).  A thread owns contiguous dz channels and gathers the strided dy / y; dy and y are read
 *   once, dz is written once.
 *   groups == 1 and act in {SF_ACT_NONE, SF_ACT_RELU}: the same kernel and the same bits as sf_epilogue_bwd.
 * sf_dwconv_dgrad_epi: data gradient of the depthwise conv `d` (as sf_dwconv_dgrad: Ti/Hi/Wi = dx's dims, To/Ho/Wo =
 * dy's dims, which must be the conv's output dims; cin_pad = the pitch of w_packed [taps][cin_pad]) with the backward of
 * its folded eval epilogue y = act(scale[c] * z + bias[c]) applied while dy is loaded — the depthwise 3x3x3 + BN + ReLU6
 * of InvertedResidual (mobilenetv2_helper.py:30-68) and conv2 + bn2 of the ShuffleNet Bottleneck
 * (shufflenet_helper.py:22-79; no activation, scale only):
 *   dx[n,ti,hi,wi,c] (=|+=) scale[c] * sum_taps w[tap][c] * dy[pos(tap)] * m(y[pos(tap)]),  taps in (kt, kh, kw) order,
 *   m as above.  No dL/dz tensor exists: against sf_epilogue_bwd_act followed by sf_dwconv_dgrad one write and one read
 *   of a tensor the size of the layer's output are saved.  scale NULL means 1; y may be NULL when act is SF_ACT_NONE.
 *   accumulate == 0 writes every element of the dx slice.  One thread per dx position and 4 channels (float4 form: C,
 *   pitches, offsets and cin_pad multiples of 4, pointers 16-byte aligned) or per channel (scalar form).
 * Both follow the rules above (SF_EINVAL before any launch, 64-bit element offsets, one owner, fixed order).        */
int sf_epilogue_bwd_act(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff, int N, int T,
                        int H, int W, int C, int rep, const float* scale, int act, int groups, float* dz, int dz_cs,
                        int dz_coff, int dz_accumulate, float* dres, int dres_cs, int dres_coff, int dres_accumulate,
                        void* stream);
int sf_dwconv_dgrad_epi(const sf_conv_desc* d, const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs,
                        int y_coff, const float* w_packed, const float* scale, int act, float* dx, int dx_cs,
                        int dx_coff, int C, int accumulate, void* stream);
int sf_head_act_mean_bwd(const float* logits, const float* dout, int B, int P, int K, int act, float* dl,
                         int accumulate, void* stream);
int sf_cam_weights(const float* g, int g_cs, int g_coff, int N, int T, int H, int W, int C, float* w, void* stream);
long sf_cam_map_ws_floats(int N, int H, int W, int C);
int sf_cam_map(const float* a, int a_cs, int a_coff, const float* w, int N, int T, int H, int W, int C, float* ws,
               float* raw, float* cam, void* stream);

/* ---- Global-context pooling and the per-sample affine: ContextBlock3D / ChannelAttention (ctx_pool.hip) ------------
 * wdf_attention_helper.py:339-358 (spatial_pool, pooling_type 'att') per sample n, over its rows_per_sample = T*H*W
 * positions of the channel slice x (NDHWC, pitch cs, offset coff):
 *     l[pos] = sum_c w[c] * x[n,pos,c] + b[0];   p = softmax_pos(l);   ctx[n,c] = sum_pos p[pos] * x[n,pos,c];
 *     lse[n] = log sum_pos exp(l[pos]).
 * sf_ctx_pool_fwd reads x ONCE: every workgroup owns a contiguous run of one sample's positions, keeps a running
 * (max, sum, acc[C]) — online softmax, the logits and the maximum in fp64 so that only the rounded difference l - max
 * reaches expf — and leaves its partial in ws; a finish kernel merges the sf_ctx_pool_parts(rows_per_sample) partials
 * of a sample in a fixed order with the usual max-rescale.  w [C] and b [1] are device arrays (b NULL: 0); ctx [N][C]
 * and lse [N] are dense; ws: sf_ctx_pool_ws_floats(N, rows_per_sample, C) floats (0 for dimensions out of range).
 * sf_ctx_pool_bwd, ONE pass again: l is recomputed, p = exp(l - lse[n]),
 *     dl[pos] = p * (x[n,pos,:] . dctx[n,:] - ctx[n,:] . dctx[n,:]);
 *     dx[n,pos,c] (=|+=) p * dctx[n,c] + dl * w[c]     (accumulate == 0 writes every element of the slice: the first
 *                                                        writer needs no zero fill; else dx = prior + that value);
 *     dw[c] (=|+=) sum_{n,pos} dl * x[n,pos,c]          (per-workgroup partial sums in ws, added in fp64 in a fixed order
 *                                                        by a finish kernel; dw_accumulate != 0 accumulates, e.g. into
 *                                                        the parameter's .grad);
 *     db[0] = 0 exactly when dw_accumulate == 0 (the softmax is shift invariant: nothing is computed; untouched when
 *     accumulating).  dw NULL: activation gradient only (db must be NULL too, ws may be NULL); db may be NULL.
 * Both: 1 <= N <= 65535, 1 <= C <= 2048; null pointers, non-positive sizes or a slice outside its pitch return
 * SF_EINVAL with nothing launched; no host synchronisation; 64-bit element offsets; float4 kernels when C, every pitch
 * and offset are multiples of 4 and x (and dx) are 16-byte aligned, scalar kernels otherwise; no atomics, one owner per
 * output element, fixed summation order: bitwise reproducible.                                                      */
int sf_ctx_pool_parts(long rows_per_sample);
long sf_ctx_pool_ws_floats(int N, long rows_per_sample, int C);
int sf_ctx_pool_fwd(const float* x, int cs, int coff, int N, long rows_per_sample, int C, const float* w,
                    const float* b, float* ctx, float* lse, float* ws, void* stream);
int sf_ctx_pool_bwd(const float* x, int cs, int coff, int N, long rows_per_sample, int C, const float* w,
                    const float* b, const float* lse, const float* ctx, const float* dctx, float* dx, int dx_cs,
                    int dx_coff, int accumulate, float* dw, float* db, int dw_accumulate, float* ws, void* stream);
/* sf_sample_affine_fwd: out[n,pos,c] = x[n,pos,c] * mul[n,c] + add[n,c], mul / add dense [N][C] device arrays, either
 * may be NULL (1 / 0) — the broadcast fusion of ContextBlock3D.forward (wdf_attention_helper.py:371-378) and, with
 * mul = 1 + sigmoid(e), ChannelAttention's x * y + x (:121-124).  out may alias x element for element.
 * sf_sample_affine_bwd, one pass over dy (and over x when dmul is wanted):
 *     dx[n,pos,c] (=|+=) dy[n,pos,c] * mul[n,c]   (accumulate as above);
 *     dmul[n,c] = sum_pos dy * x;   dadd[n,c] = sum_pos dy    (written, not accumulated; either may be NULL; per-workgroup
 *     partial sums in ws — sf_sample_affine_ws_floats floats, NULL allowed when both are NULL — added in fp64 in a
 *     fixed order by a finish kernel).  x is only read when dmul != NULL.
 * Limits, SF_EINVAL rules, float4 / scalar forms and reproducibility as for sf_ctx_pool_*.                          */
long sf_sample_affine_ws_floats(int N, long rows_per_sample, int C);
int sf_sample_affine_fwd(const float* x, int cs, int coff, int N, long rows_per_sample, int C, const float* mul,
                         const float* add, float* out, int out_cs, int out_coff, void* stream);
int sf_sample_affine_bwd(const float* dy, int dy_cs, int dy_coff, const float* x, int x_cs, int x_coff, int N,
                         long rows_per_sample, int C, const float* mul, float* dx, int dx_cs, int dx_coff,
                         int accumulate, float* dmul, float* dadd, float* ws, void* stream);

/* ---- Stripe pooling and the per-stripe broadcast add: Stripe_NonLocalBlock (stripe_pool.hip) ------------------------
 * wdf_attention_helper.py:239-273.  A frame's H rows are cut into S stripes of hs = H / S rows (H % S == 0, the
 * reference's assert at :242); stripe s is rows s*hs .. (s+1)*hs-1 and all W columns — what
 * reshape(b*c*t, stripe, h//stripe, w) followed by AdaptiveAvg/MaxPool2d(1) selects (:243-254).  All views are NDHWC
 * channel slices (pointer, pitch, offset); x, z, dz, dx are [N,T,H,W,C], the pooled tensors [N,T,S,1,.].
 * sf_stripe_pool_fwd, x read ONCE: out[n,t,s,c] = mean | max | sum over the hs*W positions of the stripe; mode
 *     SF_STRIPE_MEANMAX writes 2C channels, the mean in [0,C) and the max in [C,2C) — torch.cat([avg, max], dim=1) of
 *     :250.  The max modes also write arg, a dense int32 [N][T][S][C]: the position h_in_stripe * W + w of the maximum,
 *     of equal values the FIRST in (h, w) order (what PyTorch's adaptive max-pool backward routes the gradient to); a
 *     NaN counts as the maximum.  arg may be NULL for mean / sum.  SF_STRIPE_SUM is the backward of the broadcast add:
 *     dv[n,t,s,c] = sum_stripe dz.  One workgroup per (stripe, chunk of channels), lanes along channels; the positions
 *     are split over the workgroup's remaining lanes and merged in LDS in lane order, sums in fp64.
 * sf_stripe_add_fwd: z[n,t,h,w,c] = x[n,t,h,w,c] + v[n,t,h/hs,c] — W_y.repeat(...).reshape(b,c,t,h,w) + x of :269-271
 *     without the repeated tensor.  z may alias x element for element.
 * sf_stripe_pool_bwd, one pass: dx[n,t,h,w,c] (=|+=) dz[n,t,h,w,c] + dmean[n,t,s,c] / (hs*W)
 *                                                     + [(h - s*hs)*W + w == arg[n,t,s,c]] * dmax[n,t,s,c]
 *     — the residual's gradient and the pooling's in one pass.  dz, dmean and dmax may each be NULL (0); dmax needs
 *     arg.  accumulate == 0 writes every element of the slice, else dx = prior + that value.
 * All: null pointers, non-positive sizes, H % S != 0, an unknown mode or a slice outside its pitch return SF_EINVAL
 * with nothing launched (also C > 2^20, N*T*S or hs*W >= 2^31); no host synchronisation; 64-bit element offsets;
 * float4 kernels when C, every pitch and offset are multiples of 4 and every pointer is 16-byte aligned, scalar
 * kernels otherwise; no atomics, one owner per output element, fixed summation order: bitwise reproducible.        */
#define SF_STRIPE_MEAN 0
#define SF_STRIPE_MAX 1
#define SF_STRIPE_MEANMAX 2
#define SF_STRIPE_SUM 3
int sf_stripe_pool_fwd(const float* x, int cs, int coff, int N, int T, int H, int W, int C, int S, int mode,
                       float* out, int out_cs, int out_coff, void* arg, void* stream);
int sf_stripe_add_fwd(const float* x, int cs, int coff, const float* v, int v_cs, int v_coff, int N, int T, int H,
                      int W, int C, int S, float* z, int z_cs, int z_coff, void* stream);
int sf_stripe_pool_bwd(const float* dz, int dz_cs, int dz_coff, const float* dmean, int dmean_cs, int dmean_coff,
                       const float* dmax, int dmax_cs, int dmax_coff, const void* arg, int N, int T, int H, int W,
                       int C, int S, float* dx, int dx_cs, int dx_coff, int accumulate, void* stream);

/* ---- the training step's tail (csrc/step_tail.hip): tools/train_net.py:87-138 and :93-96 without the host.
 * sf_ce_topk: softmax cross-entropy with mean reduction (losses.py "cross_entropy", train_net.py:87), its gradient
 *   and metrics.topks_correct for k = 1 and k = k_hi (TRAIN.TOPK; train_net.py:122-125) in ONE launch.
 *   logits fp32 [N][K] with row stride ld >= K floats, labels int64 [N].  dlogits [N][K] (dense) = (softmax - onehot) / N.
 *   ring is `float[cap][8]` and counter `int[1]`, both device memory: the kernel writes row (*counter % cap) as
 *   {loss, top-1 error %, top-k_hi error %, non-finite flag, N, bad-label count, 0, 0} and then stores *counter + 1 —
 *   one thread, a plain store; the slot comes from device memory, so a replayed graph advances it.  The errors are
 *   (1 - correct / N) * 100 in float32.  loss_out is `float[2]`: the loss (the autograd result) and the same non-finite
 *   flag at an address that does not move with the ring — what sf_sgd_step takes as `guard`.
 *   Hit rule: row i is a top-k hit iff  #{j : x_j > x_l} + #{j < l : x_j == x_l} < k  (l = labels[i]): ties go to the
 *   lower index.  A row holding a NaN or an Inf sets the flag and counts as wrong for every k; NaN propagates into the
 *   loss and that row's gradient (the row maximum is subtracted before exp; a non-finite loss sets the flag too).  A
 *   label outside [0, K): the row adds 0 to the loss, gets a zero gradient row, counts as wrong and is counted in the
 *   bad-label field; nothing is read out of bounds.  exp, log and all sums run in fp64 in a fixed order (no atomics):
 *   two runs give equal bits.  One workgroup; any N and K (the real sizes are N = 2..64, K = 27..700).
 *   SF_EINVAL, nothing enqueued: a null pointer, N <= 0, K <= 0, ld < K, cap <= 0, k_hi < 1 or k_hi > K.
 * sf_sgd_step: torch.optim.SGD's update (torch/optim/sgd.py::_single_tensor_sgd) of every parameter of every group in
 *   ONE launch, per element and in that order:  g += wd * p;  buf = g on the tensor's first step, else
 *   buf = m * buf + (1 - d) * g;  g = g + m * buf if nesterov else buf;  p -= lr * g  (buf steps skipped when m == 0).
 *   table: int64 [n_tensors][6] = parameter address, gradient address, momentum-buffer address (0: the group has no
 *   momentum), numel, group, first-step flag (0 / 1).  chunks: int64 [n_chunks][2] = tensor index, first element; a
 *   chunk covers min(sf_sgd_chunk_elems(), numel - first) elements of ONE tensor and the chunks tile the tensors
 *   exactly, in table order.  hyper: fp32 [n_groups][5] = lr, weight_decay, momentum, dampening, nesterov, read from
 *   DEVICE memory by the kernel: a new learning rate is a 4-byte device write that a replayed graph sees.  The *_host
 *   arguments are the host arrays the three were uploaded from: they are checked before anything is launched, and the
 *   kernel re-checks the device row it reads (a row that fails is skipped, never dereferenced).
 *   guard: NULL, or a device float; when it reads non-zero (NaN included) the launch updates nothing.
 *   zero_grad = 1: zeros are stored to every gradient element after it is read.
 *   A chunk whose three addresses are all 16-byte aligned moves 16 bytes per access, any other 4; one owner per
 *   element, no atomics.
 *   SF_EINVAL, nothing enqueued: a null pointer (guard excepted), non-positive counts, zero_grad outside {0, 1}, a
 *   zero or 4-byte-misaligned address, numel <= 0, a group outside [0, n_groups), a first-step flag outside {0, 1}, a
 *   momentum address of 0 in a group whose momentum is not 0, chunks that do not tile the tensors exactly.
 * sf_bce: nn.BCELoss (from_logits = 0, x = probabilities: losses.py "bce") or nn.BCEWithLogitsLoss (from_logits = 1,
 *   x = logits: "bce_logit") with mean reduction over all N * K elements, its gradient, a ring row and the flag in ONE
 *   launch.  x, y (targets) fp32 [N][K] with row strides ldx, ldy >= K floats; dx [N][K] dense.
 *   from_logits = 0, torch's binary_cross_entropy: loss = -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)),
 *   dx = (p - y) / max(p (1 - p), 1e-12) / (N K).  An element whose target or probability lies outside [0, 1] (torch
 *   asserts on the device) adds no loss, gets dx = 0 and is counted in the row's bad-element field; the divisor stays
 *   N K.  from_logits = 1: loss = max(x, 0) - x y + log1p(exp(-|x|)), dx = (sigmoid(x) - y) / (N K), both in the form
 *   that neither overflows nor drops the small term at large |x|; targets are not range-checked (torch does not).
 *   ring, counter, loss_out: as sf_ce_topk; the row is {loss, 0, 0, non-finite flag, N, bad-element count, 1, 0} —
 *   field 6 names the loss that wrote the row (0: sf_ce_topk, 1: sf_bce).  A NaN or Inf in x or y sets the flag and
 *   makes the loss NaN; the other elements' gradients are those of the clean input.  log, exp, log1p and the sums run
 *   in fp64 in a fixed order (no atomics): two runs give equal bits.  One workgroup; any N and K.
 *   SF_EINVAL, nothing enqueued: a null pointer, N <= 0, K <= 0, ldx < K, ldy < K, cap <= 0, from_logits not 0 / 1.
 * sf_adam_step: torch.optim.Adam's update (torch/optim/adam.py::_single_tensor_adam, amsgrad = maximize = False) of
 *   every parameter of every group in ONE call = two launches on `stream`: a one-workgroup kernel adds 1 to every
 *   listed tensor's step count, then the update kernel reads it.  Per element, in fp32:  g += wd * p;
 *   m += (g - m) (1 - beta1);  v = beta2 v + (1 - beta2) g g;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), with
 *   bc_i = 1 - beta_i^step computed once per workgroup in fp64 (torch: Python floats).
 *   table: int64 [n_tensors][7] = parameter, gradient, exp_avg, exp_avg_sq and step-count addresses (the step count
 *   is ONE float in device memory per tensor, each at its own address: a replayed graph keeps advancing it), numel,
 *   group.  chunks: as sf_sgd_step, tiled at sf_sgd_chunk_elems().  hyper: fp64 [n_groups][5] = lr, beta1, beta2, eps,
 *   weight_decay, read from DEVICE memory (fp64 because 1 - beta2 of a float beta2 is off by 1e-5 of itself).
 *   *_host, guard, zero_grad: as sf_sgd_step; a guarded-off call moves nothing, the step counts included.
 *   A chunk whose four addresses are all 16-byte aligned moves 16 bytes per access, any other 4.
 *   SF_EINVAL, nothing enqueued: a null pointer (guard excepted), non-positive counts, zero_grad outside {0, 1}, a
 *   zero or 4-byte-misaligned address, numel <= 0, a group outside [0, n_groups), a hyper-parameter that is not
 *   finite, a beta outside [0, 1), chunks that do not tile the tensors exactly.
 * sf_ce_topk_w: sf_ce_topk with class weights — F.cross_entropy(x, y, weight = w, reduction = "mean") — still ONE launch
 *   of one workgroup.  weight fp32 [K] in device memory (read by the kernel: a replayed graph sees new values).  With
 *   W = the sum of w[y_r] over the rows with a valid label:  loss = sum w[y_r] (logsumexp(x_r) - x_r[y_r]) / W  and
 *   dlogits[r] = (w[y_r] / W) (softmax(x_r) - onehot(y_r)).  W is summed first inside the launch (one pass over the
 *   labels, fixed order, one barrier; no atomics, no second launch).  The row's factor is formed as w[y_r] * (1 / W)
 *   and the mean as total * (1 / W): with every weight 1.0f and every label valid, loss, flag, dlogits and the ring row
 *   equal sf_ce_topk's bit for bit.  (With labels outside [0, K) the divisor differs: N there, W here — as in torch,
 *   where ignored rows leave the weighted mean.)
 *   Everything else is sf_ce_topk's: a label outside [0, K) adds no loss, no weight to W, gets a zero gradient row, is
 *   counted in the bad-label field, and neither x nor weight is read at that index; the top-1 / top-k_hi errors are
 *   unweighted; the ring row has the same layout and kind 0 with the weighted mean in field 0; the flag is set by a
 *   NaN or an Inf in a row with a valid label or by a non-finite loss.  ONE difference: a row with a label outside
 *   [0, K) is left out whole, as torch leaves an ignored row out — a NaN among its logits reaches neither the loss nor
 *   the gradient (its row is zeros) nor the flag (sf_ce_topk sets the flag for it).  A row whose class has weight 0
 *   adds nothing and is not "bad".
 *   W == 0 (every present class has weight 0 — torch returns NaN) or a W that is not finite: the loss is NaN, the flag
 *   1 (a guarded optimizer skips the update) and dlogits is ALL ZEROS — no NaN reaches a gradient.
 *   SF_EINVAL, nothing enqueued: as sf_ce_topk, or a null weight.
 * sf_bce_w: sf_bce with element weights, ONE launch of one workgroup.  weight and pos_weight are fp32 [K] in device
 *   memory; either may be NULL (= all ones).  from_logits = 0: nn.BCELoss(weight = w), mean over N K of w[j] l;
 *   pos_weight must be NULL (torch has none).  from_logits = 1: nn.BCEWithLogitsLoss(weight = w, pos_weight = p),
 *   l = (1 - y) x + (1 + (p[j] - 1) y) softplus(-x) in the overflow-free form (exp(-|x|), log1p),
 *   dx = w[j] ((1 + (p[j] - 1) y) sigmoid(x) - p[j] y) / (N K).  The divisor is N K whatever the weights, as in torch.
 *   The arithmetic is arranged so that a weight of 1.0f multiplies by one and p = 1.0f adds exact zeros: with both
 *   vectors NULL or all ones every output equals sf_bce's bit for bit.  Clamps, the bad-element rule, the row (kind 1)
 *   and the flag are sf_bce's; the weighted form scales the clamped loss.
 *   SF_EINVAL, nothing enqueued: as sf_bce, or pos_weight with from_logits = 0.
 * sf_ce_mix: sf_ce_topk on the soft targets of label smoothing, mixup and CutMix — F.cross_entropy(x, t) with probability
 *   targets, equal to upstream SlowFast's lam * CE(a) + (1 - lam) * CE(b) with label_smoothing = eps (datasets/mixup.py
 *   mixup_target, losses.py SoftTargetCrossEntropy) — still ONE launch of one workgroup and no N x K target tensor.
 *   mix: device int64 [N][SF_MIX_ROW], the rows sf_clip_batch_mix read (the loss reads the partner and lam only);
 *   mix_host: the host array it was uploaded from, checked before the launch.  Both NULL: no mixing, lam = 1.
 *   With a = labels[r], b = labels[partner_r], lam = lam_r, eps = smoothing:
 *     t_r = (1 - eps) (lam onehot(a) + (1 - lam) onehot(b)) + eps / K,
 *     loss = (1 / N) sum_r (logsumexp(x_r) - sum_j t_rj x_rj),   dlogits[r] = (softmax(x_r) - t_r) / N.
 *   The top-1 / top-k_hi errors use sf_ce_topk's hit rule against the row's dominant label: a when lam >= 0.5, else b.
 *   The ring row (kind 0, column 7 left 0), the flag and loss_out are sf_ce_topk's; exp, log and all sums in fp64 in a
 *   fixed order, no atomics: two runs give equal bits.  With smoothing == 0, no mix table and finite logits every
 *   output equals sf_ce_topk's bit for bit (eps = 0 and lam = 1 multiply by one and add exact zeros).
 *   A BAD ROW — a or b outside [0, K), a device mix row whose partner is outside [0, N) or whose lam is not in
 *   [0, 1] — adds no loss, gets a zero gradient row, counts as wrong and is counted in field 5; the divisor stays N and
 *   nothing is read out of bounds.
 *   SF_EINVAL, nothing enqueued: everything sf_ce_topk refuses, smoothing outside [0, 1) or NaN, exactly one of mix /
 *   mix_host, a host row with its partner outside [0, N), its mode outside {0, 1, 2} or lam outside [0, 1].
 *   Class weights together with soft targets are not offered: torch divides by N for probability targets and by the
 *   weight sum for index targets.
 * sf_adamw_step: torch.optim.AdamW's update (_single_tensor_adam with decoupled_weight_decay = True, amsgrad = maximize
 *   = False) — sf_adam_step with ONE change per element:  p *= f  in front, with f = (float)(1 - lr * weight_decay)
 *   computed once per workgroup in fp64 beside the bias corrections (torch multiplies by that Python float), and no
 *   wd * p added to g.  Table, chunks, hyper rows, *_host checks, guard, zero_grad and the step-count launch are
 *   sf_adam_step's, and both are one kernel body behind a template flag.  With weight_decay == 0 in every group f is
 *   1.0f and every output equals sf_adam_step's bit for bit.  SF_EINVAL: sf_adam_step's list.
 * sf_lars_sgd_step: sf_sgd_step behind a per-tensor trust ratio (LARS / LARC).  ratios: fp32 [n_tensors][2] = {r, wd_t}
 *   in DEVICE memory, row i for row i of the table — what sf_lars_ratios writes.  Per element
 *   g = (g + wd_t * p) * r  — sf_sgd_step's fused form of the decay, then one fp32 multiply — and then sf_sgd_step's
 *   momentum, dampening, nesterov, first-step flag and  p -= lr * g,  unchanged; the group's weight_decay (hyper column
 *   1) is NOT applied again.  One kernel body behind a template flag: when every tensor has r == 1 and wd_t == its
 *   group's weight decay every output equals sf_sgd_step's bit for bit.  guard (hand it sf_lars_ratios' state + 5),
 *   zero_grad and the *_host checks are sf_sgd_step's.  SF_EINVAL: sf_sgd_step's list, or a null ratios. */
int sf_adamw_step(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
                  int n_chunks, const double* hyper_host, const double* hyper, int n_groups, const float* guard,
                  int zero_grad, void* stream);
int sf_lars_sgd_step(const long* table_host, const long* table, int n_tensors, const long* chunks_host,
                     const long* chunks, int n_chunks, const float* hyper_host, const float* hyper, int n_groups,
                     const float* ratios, const float* guard, int zero_grad, void* stream);
int sf_ce_mix(const float* logits, int ld, const long* labels, const long* mix_host, const long* mix, int N, int K,
              int k_hi, float smoothing, float* dlogits, float* ring, int* counter, int cap, float* loss_out,
              void* stream);
int sf_ce_topk(const float* logits, int ld, const long* labels, int N, int K, int k_hi, float* dlogits, float* ring,
               int* counter, int cap, float* loss_out, void* stream);
int sf_sgd_chunk_elems(void);
int sf_sgd_step(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
                int n_chunks, const float* hyper_host, const float* hyper, int n_groups, const float* guard,
                int zero_grad, void* stream);
int sf_bce(const float* x, int ldx, const float* y, int ldy, int N, int K, int from_logits, float* dx, float* ring,
           int* counter, int cap, float* loss_out, void* stream);
int sf_adam_step(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
                 int n_chunks, const double* hyper_host, const double* hyper, int n_groups, const float* guard,
                 int zero_grad, void* stream);
int sf_ce_topk_w(const float* logits, int ld, const long* labels, const float* weight, int N, int K, int k_hi,
                 float* dlogits, float* ring, int* counter, int cap, float* loss_out, void* stream);
int sf_bce_w(const float* x, int ldx, const float* y, int ldy, const float* weight, const float* pos_weight, int N,
             int K, int from_logits, float* dx, float* ring, int* counter, int cap, float* loss_out, void* stream);

/* ---- gradient clipping (csrc/grad_clip.hip): torch/nn/utils/clip_grad.py (clip_grad_norm_, clip_grad_value_) between
 * the backward pass and sf_sgd_step / sf_adam_step, without the host.  No entry point synchronises or reads back.
 * All three are addressed like sf_sgd_step.  table: int64 [n_tensors][2] = gradient address, numel.  chunks: int64
 *   [n_chunks][2] = tensor index, first element, tiled at sf_sgd_chunk_elems() exactly as sf_sgd_step's.  The *_host
 *   arguments are the host arrays the two were uploaded from: they are checked before anything is launched, and every
 *   kernel re-checks the device row it reads (a row that fails does nothing, never a wild access).  One workgroup per
 *   chunk; a chunk whose address is 16-byte aligned moves 16 bytes per access, any other 4.
 * sf_grad_norm: the total norm of all listed gradients, norm_type = SF_NORM_L2 or SF_NORM_INF, in TWO launches.
 *   Launch 1, one workgroup per chunk: thread t squares (fp64) and adds the elements of the groups of four t, t + 256,
 *   ... in order, xor butterfly over the wavefront, the four wavefronts in order through LDS; ONE fp64 partial per chunk
 *   goes to partials (caller-owned, fp64 [n_chunks]).  Both access widths read the same elements in the same order:
 *   the partial does not depend on the alignment.  SF_NORM_INF: the partial is max |g|, a NaN propagating (torch.max).
 *   Launch 2, ONE workgroup: thread t folds partials t, t + 256, ... in order, then the same two steps.  No atomics, no
 *   "last workgroup" finish: equal inputs give equal bits.  It writes state (caller-owned, 8 floats, 8-byte aligned):
 *     [0..1] the norm as one fp64 (sqrt of the sum, or the maximum);  [2] the norm rounded once to fp32;
 *     [3] the coefficient min(1, max_norm / (norm + 1e-6)) — torch's formula — evaluated in fp64, rounded once to fp32;
 *         1 when max_norm is NULL or not positive, or when the norm is not finite;
 *     [4] 1 when the norm is not finite (a NaN or an Inf among the gradients), else 0;
 *     [5] guard_out = (guard_in != NULL && *guard_in != 0) || [4] ? 1 : 0 — what sf_grad_scale reads and what
 *         sf_sgd_step / sf_adam_step take as `guard`;  [6..7] unused.
 *   max_norm: NULL, or ONE fp32 in DEVICE memory (a replayed graph sees a new value).  guard_in: NULL, or the loss's
 *   guard (sf_ce_topk's loss_out + 1).  ring / counter / cap: NULL, NULL, anything — or sf_ce_topk's ring: when
 *   *counter > 0 the fp32 norm goes to column 7 of row (*counter - 1) % cap, the row the step's loss kernel wrote and
 *   whose column 7 every loss kernel leaves 0; no other column is touched and *counter == 0 writes nothing.
 *   SF_EINVAL, nothing enqueued: a null table / chunks / partials / state, non-positive counts, an unknown norm_type, a
 *   zero or 4-byte-misaligned address, numel <= 0, chunks that do not tile the tensors exactly, ring without counter or
 *   the reverse, a ring with cap <= 0.  SF_EALIGN: partials or state not on 8 bytes.
 * sf_grad_scale: g *= state[3] in fp32, ONE launch.  Every workgroup returns without touching memory when state[5] is
 *   not 0 or state[3] is not in [0, 1): g * 1.0f is g, so a step that needs no clipping costs no gradient traffic here,
 *   and a step whose norm is not finite leaves the gradients as they are (torch multiplies them by NaN).
 *   SF_EINVAL as above (or a null state); SF_EALIGN: state not on 8 bytes.
 * sf_grad_clamp: clip_grad_value_, g = min(max(g, -v), v) with torch.clamp's bits (a NaN passes, -0.0 keeps its sign,
 *   +-Inf become +-v), ONE launch.  value: ONE fp32 in DEVICE memory; not positive or NaN: nothing moves.  Elements
 *   inside the range are not written again.  SF_EINVAL as above (or a null value). */
#define SF_NORM_INF 0
#define SF_NORM_L2 2
int sf_grad_norm(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
                 int n_chunks, int norm_type, const float* max_norm, const float* guard_in, double* partials,
                 float* state, float* ring, int* counter, int cap, void* stream);
int sf_grad_scale(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
                  int n_chunks, const float* state, void* stream);
int sf_grad_clamp(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
                  int n_chunks, const float* value, void* stream);

/* ---- layer-wise trust ratios (csrc/lars.hip): LARS / LARC (upstream SlowFast's SOLVER.LARS_ON, NVIDIA apex's LARC)
 * between the backward pass and sf_lars_sgd_step, without the host.  Nothing synchronises or reads back.
 * sf_lars_ratios: ||p|| and ||g|| of every listed tensor and the ratio they give, in TWO launches.
 *   table: int64 [n_tensors][6] = parameter address, gradient address, numel, group, index of the tensor's first
 *   chunk, ignored flag (0 / 1: the tensor gets plain SGD — 1-D parameters under ignore_1d_param).  chunks: int64
 *   [n_chunks][2] as sf_sgd_step's, tiled at sf_sgd_chunk_elems() in table order, so a tensor's chunks are contiguous.
 *   hyper: fp32 [n_groups + 1][3] in DEVICE memory = per group lr, weight_decay, apply (0 / 1); then ONE row
 *   trust_coefficient, eps, clip (0 / 1).  A new lr is a 4-byte device write that a replayed graph sees.  The *_host
 *   arguments are the host arrays the three were uploaded from: checked before anything is launched, and every kernel
 *   re-checks the device row it reads (a row that fails reads nothing: zero partials, r = 1, wd_t = 0).
 *   Launch 1, one workgroup per chunk, reads the chunk of p and of g once: thread t squares (fp64) and adds the
 *   elements of the groups of four t, t + 256, ... in order, xor butterfly over the wavefront, the four wavefronts in
 *   order through LDS — sf_grad_norm's order; TWO fp64 partials per chunk go to partials (caller-owned, fp64
 *   [n_chunks][2] = sum p^2, sum g^2).  Both access widths (16 bytes where the array's address allows, else 4) read
 *   the same elements in the same order: a partial does not depend on the alignment.
 *   Launch 2, n_tensors + 1 workgroups.  Workgroup t folds tensor t's partials in chunk order (thread i takes i,
 *   i + 256, ..., then the same two steps), takes pn = sqrt(sum p^2), gn = sqrt(sum g^2) and writes ratios[t] (caller-
 *   owned, fp32 [n_tensors][2]) = {r, wd_t}, evaluated in fp64 and rounded once, wd = the group's weight_decay:
 *     apply == 0 or the tensor is ignored:   r = 1, wd_t = wd  (plain SGD with weight decay);
 *     a norm that is not finite:             r = 1, wd_t = wd, and the guard is raised;
 *     pn != 0 and gn != 0:                   r = trust * pn / (gn + pn * wd + eps);  with clip: r = min(r / lr, 1);
 *                                            wd_t = wd;
 *     a zero norm:                           r = 1, wd_t = 0.
 *   The last workgroup looks at every partial and writes state (caller-owned, 8 floats, 8-byte aligned, sf_grad_norm's
 *   layout):  [4] 1 when a partial is not finite (a NaN or an Inf in a parameter or a gradient, ignored tensors
 *   included), else 0;  [5] guard_out = (guard_in != NULL && *guard_in != 0) || [4] ? 1 : 0 — what sf_lars_sgd_step
 *   takes as `guard`; the other six floats are not touched.  Every word has ONE writer, a plain store: no atomics, no
 *   "last workgroup" finish — equal inputs give equal bits.
 *   SF_EINVAL, nothing enqueued: a null pointer (guard_in excepted), non-positive counts, a zero or 4-byte-misaligned
 *   address, numel <= 0, a group outside [0, n_groups), a first-chunk column that is not the running chunk count, an
 *   ignored flag, apply or clip outside {0, 1}, chunks that do not tile the tensors exactly.  SF_EALIGN: partials or
 *   state not on 8 bytes. */
int sf_lars_ratios(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
                   int n_chunks, const float* hyper_host, const float* hyper, int n_groups, const float* guard_in,
                   double* partials, float* ratios, float* state, void* stream);

/* ---- averaged weights (csrc/weight_avg.hip): the EMA / SWA copy of parameters and BN buffers that large-batch recipes
 * evaluate and checkpoint (torch.optim.swa_utils.AveragedModel), and the running mean of the precise-BN pass, without
 * the host.  Nothing synchronises or reads back.
 * table: int64 [n_tensors][4] = average address, source address, numel, kind:
 *     0  float32, averaged;
 *     1  float32, copied source -> average (a buffer when buffers are not averaged: torch's use_buffers = False);
 *     2  int64 words, copied (num_batches_tracked); numel counts 8-byte words.
 *   chunks: int64 [n_chunks][2] as sf_sgd_step's, tiled at sf_sgd_chunk_elems() in table order.  The *_host arguments are
 *   the host arrays the device ones were uploaded from: checked before anything is launched, and every workgroup
 *   re-checks the device row it reads, its numel against the chunk list included (a row that fails touches nothing; a
 *   numel that moved inside its last chunk's slack cannot be told).  Accesses are 16 bytes wide where both addresses of
 *   a span allow, else 4; every element has one owner and one formula, so both widths give the same bits.
 * sf_avg_update: ONE launch over the table, then a one-thread launch.  count: ONE int64 in DEVICE memory, the number of
 *   updates so far (torch's n_averaged); hyper: ONE fp32 in DEVICE memory (mode 0 only; may be NULL otherwise), hyper_host
 *   the host value it was uploaded from.  Every kind-0 element a with its source s:
 *     *count == 0 (any mode):  a = s — the first update is a copy, as in torch;
 *     mode 0 (EMA):            a = lerp(a, s, w),  w = hyper[0] = 1 - decay;
 *     mode 1 (equal mean):     a = lerp(a, s, 1.f / (float)(*count + 1));
 *     mode 2 (running mean):   a = a + (s - a) * (1.f / (float)(*count + 1)) — three fp32 operations rounded one by
 *                              one, what torch's GPU kernels compute for  m += (s - m) / (k + 1)  with a host k (their
 *                              division by a host scalar multiplies by the fp32 reciprocal);
 *     lerp(a, s, w) = w < 0.5 ? fma(w, s - a, a) : fma(-(s - a), 1 - w, s) — torch's lerp, its bits.
 *   Kinds 1 and 2 are copied at every update.  The second launch stores *count + 1: every workgroup of the first has
 *   read the old value, no atomics.  guard: NULL, or the loss's / clipper's / LARS's guard — non-zero or NaN switches
 *   the whole call off, the count included.  A negative count moves nothing.
 *   SF_EINVAL, nothing enqueued: a null table / chunks / count, non-positive counts, a mode outside 0..2, in mode 0 a
 *   null hyper / hyper_host or hyper_host[0] outside [0, 1] or NaN, a zero address, numel <= 0, a kind outside 0..2,
 *   chunks that do not tile the tensors exactly.  SF_EALIGN: a float address not on 4 bytes, a word address or count
 *   not on 8.
 * sf_avg_exchange: ONE launch over the same table, all three kinds.  op 0: swap average and source element by element
 *   (twice restores every bit); op 1: average -> source; op 2: source -> average.  16 bytes per swapped element.
 *   SF_EINVAL: an op outside 0..2 and the table refusals above; SF_EALIGN as above. */
int sf_avg_update(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
                  int n_chunks, int mode, const float* hyper_host, const float* hyper, long* count, const float* guard,
                  void* stream);
int sf_avg_exchange(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
                    int n_chunks, int op, void* stream);

/* ---- training telemetry (csrc/tensor_stats.hip): what the reference's TensorboardWriter (TENSORBOARD.MODEL_VIS) is
 * there to watch — per-tensor statistics and a histogram of EVERY parameter or gradient — in one call of TWO launches
 * that reads every element once, without the host.  Nothing synchronises or reads back.
 * sf_tensor_stats: table: int64 [n_tensors][2] = address, numel, as sf_grad_norm's; an address of 0 is a tensor that is
 *   ABSENT (a parameter whose .grad is still None) and not an error: its numel still tiles the chunk list, nothing of it
 *   is read, and its row is all zeros (present = 0).  chunks: int64 [n_chunks][2] as sf_sgd_step's, tiled at
 *   sf_sgd_chunk_elems() in table order.  The *_host arguments are the host arrays the two were uploaded from: checked
 *   before anything is launched, and every kernel re-checks the device row it reads (a row that fails is treated as
 *   absent, never a wild access).
 *   The row of a tensor is SF_TSTATS_ROW = 58 slots of 8 bytes:
 *     [0] present (0 / 1)   [1] numel   [2] n_nan   [3] n_inf (+Inf and -Inf)   [4] n_zero (+0.0 and -0.0)      int64
 *     [5] min (low 4 bytes), max (high 4 bytes)   [6] absmax (low), 0.f (high)     fp32, over the FINITE elements; none:
 *                                                                                  min = +inf, max = -inf, absmax = 0
 *     [7] sum   [8] sumsq       fp64, over the finite elements, each widened to fp64 before it is squared or added
 *     [9 .. 57] hist[2 B + 1]   int64, B = SF_TSTATS_BINS = 24 exponent bins per sign and one centre bin
 *   The bin of a finite x, with e = floor(log2 |x|) taken from the exponent field by integer arithmetic:
 *     |x| < 2^-20 (zeros and denormals included):  the centre bin, hist[B];
 *     otherwise k = min(max(e + 20, 0), B - 1):    hist[B + 1 + k] for x > 0, hist[B - 1 - k] for x < 0 — everything at
 *                                                  or above 2^3 lands in the last bin of its side.
 *   The 2 B + 2 bin boundaries increase: -2^4, -2^3, ..., -2^-20, +2^-20, ..., +2^4 (the outermost two are nominal: the
 *   outer bins are open).  Every finite element is in exactly one bin and a NaN or an Inf in none:
 *   sum(hist) + n_nan + n_inf == numel.
 *   Launch 1, one workgroup per chunk: thread t takes the elements of the groups of four t, t + 256, ... in order
 *   (sf_grad_norm's walk: 16-byte accesses where the address allows, else 4-byte ones, the same elements in the same order,
 *   so the bits do not depend on the alignment), the fp64 sums go through the xor butterfly and the four wavefronts in
 *   order through LDS, the counts through integer LDS adds and min / max through integer LDS min / max (on keys of the
 *   floats' order) on 32 copies laid out one per bank — integers: order-free; ONE row per chunk goes
 *   to ws (caller-owned, sf_tensor_stats_ws_bytes(n_chunks) bytes, 8-byte aligned, no need to clear it).
 *   Launch 2, one workgroup per tensor: thread i folds the tensor's chunk rows i, i + 256, ... in chunk order, then the
 *   same two steps, and writes the row.  No float atomics, no "last workgroup" finish, no memset: every byte of every
 *   row is written by one writer and equal inputs give equal bits.
 *   ring: int64-sized slots [slots][n_tensors][SF_TSTATS_ROW] in DEVICE memory; cursor: int32 [2] in DEVICE memory =
 *   {the slot this call writes, the calls made so far (saturating)}.  Launch 1 reads the slot (a value outside
 *   [0, slots) counts as 0), launch 2 writes slot's rows and stores cursor[0] = (slot + 1) % slots, cursor[1] + 1: a caller
 *   records every step, also inside a captured graph, and reads the ring once per logging period.  row: the row width
 *   the caller allocated the ring with.
 *   SF_EINVAL, nothing enqueued: a null table / chunks / ws / ring / cursor, non-positive counts, row != SF_TSTATS_ROW,
 *   slots <= 0, ws_bytes below sf_tensor_stats_ws_bytes(n_chunks), an address off 4 bytes, numel <= 0, chunks that do
 *   not tile the tensors exactly.  SF_EALIGN: ws or ring not on 8 bytes, cursor not on 4.
 * sf_tensor_stats_ws_bytes: host only; 0 for n_chunks <= 0. */
#define SF_TSTATS_BINS 24
#define SF_TSTATS_ROW 58
long sf_tensor_stats_ws_bytes(int n_chunks);
int sf_tensor_stats(const long* table_host, const long* table, int n_tensors, const long* chunks_host, const long* chunks,
                    int n_chunks, void* ws, long ws_bytes, long* ring, int row, int slots, int* cursor, void* stream);

/* ---- evaluation (csrc/eval_metrics.hip): tools/train_net.py:166-251 eval_epoch and utils/meters.py:557-714 (ValMeter,
 * get_map) without the host.  No entry point synchronises or reads anything back.
 * sf_topk_errors: metrics.topks_correct for k = 1 and k = k_hi and the two error percentages (train_net.py:227-232) of
 *   one evaluation batch in ONE launch.  preds fp32 [N][K] with row stride ld >= K (the eval head's probabilities; no
 *   exp, no log, no gradient), labels int64 [N].  ring / counter / cap: sf_ce_topk's memory and counter protocol; the
 *   row is {0, top-1 error %, top-k_hi error %, non-finite flag, N, bad-label count, 2, 0}.  The hit rule, the
 *   treatment of a row with a NaN or an Inf (wrong for every k, sets the flag) and of a label outside [0, K) (wrong,
 *   counted, never read) are sf_ce_topk's — one device function serves both.  One workgroup; any N and K.
 *   SF_EINVAL, nothing enqueued: a null pointer, N <= 0, K <= 0, ld < K, cap <= 0, k_hi < 1 or k_hi > K.
 * sf_rows_append: ValMeter.update_predictions (utils/meters.py:623-632) as a copy.  preds and labels fp32 [N][K] with
 *   row strides ldp, ldl >= K go to rows cursor[0] .. cursor[0] + N - 1 of the caller's stores store_preds /
 *   store_labels, fp32 [cap][K] dense; cursor is device int32 [2] = {rows filled, rows refused}.  Rows that would pass
 *   cap are not written and are added to cursor[1]; cursor[0] advances by the rows written.  The cursor is read from
 *   device memory, so a captured call appends where the previous one stopped.  One workgroup.
 *   SF_EINVAL, nothing enqueued: a null pointer, N <= 0, K <= 0, ldp < K, ldl < K, cap <= 0.
 * sf_map: get_map (utils/meters.py:690-714) of scores fp32 [N][C] against labels fp32 [N][C] (row strides lds, ldl >= C)
 *   in TWO launches whatever N and C are, without a sort.  For a class with P > 0 positives
 *       AP = (1/P) sum_{i : y_i = 1} TP(s_i) / CNT(s_i),  TP(t) = #{j : s_j >= t, y_j = 1},  CNT(t) = #{j : s_j >= t}
 *   — sklearn's average_precision_score: tied scores form one threshold there and every positive of the group adds the
 *   group's precision.  Scores compare as floats (-0.0 ties +0.0).  The counts are integers, every term one fp64
 *   division, every sum folded in a fixed order (no float atomics): the same inputs give the same bits.
 *   out fp64 [3] = {mean AP over the classes with a positive (0 when there is none, as get_map returns then), the
 *   number of those classes, the number of refused elements: a NaN or infinite score or a label other than 0 or 1 —
 *   the caller must not use out[0] when that is not 0}.  ap: NULL, or fp64 [C] per-class AP, -1 for a class left out.
 *   ws: sf_map_ws_bytes(N, C) bytes of caller-owned scratch (host-only query; 0 for sizes out of range), 8-byte
 *   aligned as out and ap (SF_EALIGN otherwise).  O(N P) comparisons per class.
 *   SF_EINVAL, nothing enqueued: a null pointer (ap excepted), N <= 0, C <= 0, lds < C, ldl < C, N above 16 776 960. */
int sf_topk_errors(const float* preds, int ld, const long* labels, int N, int K, int k_hi, float* ring, int* counter,
                   int cap, void* stream);
int sf_rows_append(const float* preds, int ldp, const float* labels, int ldl, int N, int K, float* store_preds,
                   float* store_labels, int* cursor, int cap, void* stream);
long sf_map_ws_bytes(int N, int C);
int sf_map(const float* scores, int lds, const float* labels, int ldl, int N, int C, void* ws, double* out,
           double* ap, void* stream);

/* ---- per-class evaluation (csrc/class_report.hip): which class is taken for which, and every class's precision,
 * recall and F1, from counters that stay on the device.  The reference has no code for this; the contract is this
 * comment, restated by brute force in tests/_class_report_ref.py.  No entry point synchronises or reads anything back;
 * every buffer is the caller's; both are capturable.
 * The rule of a row is sf_topk_errors': class j stands IN FRONT OF class c iff x[j] > x[c], or x[j] == x[c] and j < c
 *   (torch.topk's order).  Values compare as floats: -0.0 ties +0.0, and of equal values the lower index stands in
 *   front.  The PREDICTED class is the one nothing stands in front of — the largest value, the lowest index among
 *   equals; the label is within the top k iff fewer than k classes stand in front of it, so "predicted == label" and
 *   "within the top 1" are one statement.  A NaN compares false with everything; a row that holds a NaN or an infinity
 *   is refused whole (sf_topk_errors counts such a row as wrong for every k), as is a row whose label is outside [0, K).
 * sf_confusion_update: ONE launch that ADDS a batch to the counters (the caller zero-fills them at the start of an epoch).
 *   preds fp32 [N][K] with row stride ld >= K, labels int64 [N] (as sf_topk_errors takes them).
 *   conf int64 [K][K], indexed [true class][predicted class].  hits int64 [K][2]: per true class, the rows whose label
 *   is within the top 1 and within the top k_hi.  refused int64 [2] = {rows with a label outside [0, K) — their scores
 *   are never read; rows with a valid label that hold a NaN or an infinity}.  A refused row adds to nothing else.
 *   For every input: sum(conf) = N - refused[0] - refused[1]; trace(conf) = sum(hits[:, 0]) = the top-1 hits
 *   sf_topk_errors counts for the batch (N - refused - the top-1 errors among the accepted rows); sum(hits[:, 1]) = its
 *   top-k_hi hits; row sums of conf = support, column sums = predicted counts.
 *   Only integer adds are used — the result does not depend on the order of execution — and no float atomics.
 *   Two routes, split at K = sf_confusion_small_kmax() = 201, the largest K whose K*K + 2K + 2 uint32 counters fit the
 *   160 KiB - 512 B of LDS one workgroup may hold on gfx950:
 *     K <= 201: a thread per row; the counters of a workgroup's rows are kept in LDS and its non-zero ones go to
 *       global memory once, one 64-bit integer atomic each.
 *     K > 201: a wavefront per row; one global integer atomic per row into conf and at most two into hits.
 *   A row is swept once (plus the one read of the label's score).  Rows that all start on 16 bytes (pointer aligned,
 *   ld % 4 == 0) are read 16 bytes at a time, any other view 4 bytes at a time.
 *   SF_EINVAL, nothing enqueued: a null pointer, N <= 0, K <= 0, ld < K, k_hi < 1 or k_hi > K.  SF_EALIGN, nothing
 *   enqueued: preds not on 4 bytes, labels / conf / hits / refused not on 8.
 * sf_class_report: ONE launch, one workgroup, K <= 1024.  per_class fp64 [K][6] = {support, precision, recall, F1,
 *   top-1 accuracy, top-k_hi accuracy} with TP = conf[c][c], FP = column sum - TP, FN = support - TP:
 *   precision = TP / (TP + FP), recall = TP / (TP + FN), F1 = 2 TP / (2 TP + FP + FN), accuracies = hits / support;
 *   each is ONE fp64 division of exact integers, and 0 when the denominator is 0.
 *   out fp64 [8] = {samples, accuracy = trace / samples, mean-class accuracy (mean recall over the classes with
 *   support > 0), macro precision, macro recall, macro F1 (means over the same classes), the number of classes with
 *   support, the number of classes never predicted}.  The sums run in class order in one thread: the same counters give
 *   the same bits.  Means over no class, and the accuracy of no sample, are 0.
 *   SF_EINVAL, nothing enqueued: a null pointer, K <= 0, K > 1024.  SF_EALIGN: a buffer not on 8 bytes.
 * sf_class_weights: class weights for sf_ce_topk_w / sf_bce_w from the same counters, ONE launch, one workgroup,
 *   K <= 1024, no host read.  support[c] = row sum c of conf, S = the samples counted, K+ = the classes with
 *   support > 0; w fp32 [K]; a class without support gets 0 (all-zero counters give all zeros).
 *   SF_WEIGHTS_BALANCED: scikit-learn's compute_class_weight("balanced") over the classes with support,
 *     w[c] = S / (K+ support[c]) — ONE fp64 division of exact integers, rounded once to fp32.
 *   SF_WEIGHTS_EFFECTIVE: the class-balanced weight of the effective number of samples,
 *     e[c] = (1 - beta) / (1 - beta^support[c]), w[c] = e[c] K+ / sum(e) — in fp64, the sum in class order, rounded once
 *     to fp32; the weights over the classes with support sum to K+.  beta points to ONE fp64 in HOST memory, read
 *     during the call, in (0, 1); it is not read for SF_WEIGHTS_BALANCED and may be NULL there.
 *   Across ranks the counters must have been summed first (the caller's collective); there is none here.
 *   SF_EINVAL, nothing enqueued: a null conf or w, K <= 0, K > 1024, an unknown scheme, SF_WEIGHTS_EFFECTIVE with a
 *   null beta or one outside (0, 1).  SF_EALIGN: conf not on 8 bytes, w not on 4. */
#define SF_WEIGHTS_BALANCED 0
#define SF_WEIGHTS_EFFECTIVE 1
int sf_class_weights(const long* conf, int K, int scheme, const double* beta, float* w, void* stream);
int sf_confusion_small_kmax(void);
int sf_confusion_update(const float* preds, int ld, const long* labels, int N, int K, int k_hi, long* conf, long* hits,
                        long* refused, void* stream);
int sf_class_report(const long* conf, const long* hits, int K, double* out, double* per_class, void* stream);

/* ---- detection evaluation (csrc/ava_eval.hip): the AVA frame-mAP at IoU 0.5 as utils/ava_eval_helper.py and the
 * PascalDetectionEvaluator of utils/ava_evaluation/ define it, from device tensors.  No entry point synchronises or
 * reads anything back; every buffer is the caller's.  tests/_ava_ref.py restates the rules below in numpy.
 * Detections (ava_eval_helper.py:249-285): row i of preds fp32 [K][C] belongs to image (video, second) =
 *   rint(metadata[i][0..1]) and is, for every class column j with whitelist[j] != 0, one detection with score
 *   preds[i][j] and box boxes[i][1..4] = x1, y1, x2, y2 (boxes[i][0] is the batch index).  Rows of one image need not
 *   be contiguous; the order of an image's detections is the row order.
 * Ground truth, built on the host once: gt_box fp64 [G][4] (x1, y1, x2, y2), gt_cls int32 [G] (class COLUMN = id - 1),
 *   gt_off int32 [I + 1] (rows of image m are gt_off[m] .. gt_off[m + 1] - 1, grouped by class, CSV order within a
 *   class), lut int32 [V][S] ((video, second) -> image id, -1: not in the ground truth, -2: excluded; a second outside
 *   [0, S) is -1), whitelist uint8 [C], num_gt int32 [C] (ground-truth rows per class over the non-excluded images,
 *   whether or not they have detections).
 * sf_ava_match: a fill of `first` and TWO launches.  valid uint8 [K] = 1 for a row that is evaluated, 0 for a dropped
 *   one (excluded image; x1 >= x2 or y1 >= y2 or a NaN coordinate: _remove_invalid_boxes), 2 for a video index outside
 *   [0, V) or non-finite metadata.  tp uint8 [K][C] = 1 iff (row, class) is a true positive
 *   (per_image_evaluation.py:331-345): g* = the first maximum of the IoU over the image's ground-truth rows of the
 *   class, IoU(g*) >= 0.5, and no earlier row of the image has the same g* with IoU >= 0.5.  Launch 1 takes the integer
 *   minimum of the claiming rows per ground-truth box, launch 2 compares: the reference's sequential rule without an
 *   assumption on row order, and the same bits run to run.  IoU is np_box_ops.iou in fp64, every operation rounded on
 *   its own (no fused multiply-add).  An image without ground truth has false positives only.
 * sf_ava_ap: THREE launches, no sort (metrics.py:60-125, object_detection_evaluation.py:777-815).  Per class with
 *   num_gt > 0: AP = (1 / num_gt) sum over its true positives of the largest cumTP / position at or after it in
 *   descending score order; equal scores are ordered by DESCENDING row index (numpy's argsort leaves that open).
 *   Integer ranks, exact int64 fraction compares, one fp64 division per true positive, fixed-order fp64 sums.
 *   out fp64 [4] = {mean AP over the classes with num_gt > 0 (NaN when there is none, as np.nanmean), the number of
 *   those classes, the number of refused scores (NaN or infinite, of evaluated detections), the number of rows with
 *   valid == 2 — the caller must not use out[0] unless both are 0}.  ap: NULL, or fp64 [C], -1 for a class left out.
 *   O(K) comparisons per true positive.
 * ws: sf_ava_ws_bytes(K, C, G) bytes, shared by both calls (host-only query; 0 for sizes out of range: K <= 0, C <= 0,
 *   G < 0, K C >= 2^31, K above 16 776 960), on 8 bytes as gt_box, out and ap (SF_EALIGN otherwise).
 *   SF_EINVAL, nothing enqueued: a null pointer (ap excepted; gt_box / gt_cls when G == 0), a size out of range,
 *   ldb < 5, ldm < 2, ld < C, I < 0, V <= 0, S <= 0, V S >= 2^31. */
long sf_ava_ws_bytes(int K, int C, int G);
int sf_ava_match(const float* boxes, int ldb, const float* metadata, int ldm, int K, int C, const double* gt_box,
                 const int* gt_cls, const int* gt_off, int G, int I, const int* lut, int V, int S,
                 const unsigned char* whitelist, void* ws, unsigned char* tp, unsigned char* valid, void* stream);
int sf_ava_ap(const float* preds, int ld, const unsigned char* tp, const unsigned char* valid, int K, int C,
              const unsigned char* whitelist, const int* num_gt, int G, void* ws, double* out, double* ap,
              void* stream);

#ifdef __cplusplus
}
#endif
#endif
