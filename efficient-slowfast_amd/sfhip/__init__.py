"""sfhip — ctypes binding of libsfhip.so (include/sfhip.h), the MI355X kernels of the SlowFast/CMDA path.

PyTorch is used for device memory (torch.empty on the caching allocator), the current HIP stream and
parameter preprocessing only; every activation-sized computation is a libsfhip kernel.  There is NO CPU
or eager-PyTorch fallback: if the shared library is missing, or a tensor is not on a GPU, the ops raise.

Activations are NDHWC views (`Act`): a contiguous buffer [N, T, H, W, pitch] plus a channel slice
(coff, C).  Producers write straight into slices of wider buffers, so torch.cat never runs on the path.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SF_LIB: an alternative build of the library (A/B runs of compiler flags inside one GPU lease; default: the in-tree build)
_LIB_PATH = os.environ.get("SF_LIB") or os.path.join(_HERE, "libsfhip.so")
_lib = None

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SOFTMAX, ACT_HSIGMOID, ACT_RELU6 = 0, 1, 2, 3, 4, 5


def _act(relu):
    """relu: False/True (ReLU) or 6 (ReLU6)."""
    return ACT_RELU6 if relu == 6 else (ACT_RELU if relu else ACT_NONE)
SF_EINVAL, SF_EALIGN, SF_ELAUNCH, SF_ENOTTAKEN = -1, -2, -3, -4
_ERR = {-1: "SF_EINVAL (inconsistent descriptor)", -2: "SF_EALIGN", -3: "SF_ELAUNCH (hip launch failed)",
        -4: "SF_ENOTTAKEN (shape not served by this specialised entry point)"}
_REFUSED = (SF_EALIGN, SF_ENOTTAKEN)  # a specialised entry point declined before any launch: take the general one


class SfhipError(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "N", "Ti", "Hi", "Wi", "Cin", "in_cs", "in_coff", "To", "Ho", "Wo", "Cout", "out_cs", "out_coff",
        "out_cmul", "kT", "kH", "kW", "sT", "sH", "sW", "pT", "pH", "pW", "dT", "dH", "dW", "cin_pad", "act",
        "res_cs", "res_coff", "transposed", "os_T", "os_H", "os_W", "oo_T", "oo_H", "oo_W", "ob_T", "ob_H", "ob_W")]


class PoolDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "N", "Ti", "Hi", "Wi", "C", "in_cs", "in_coff", "To", "Ho", "Wo", "out_cs", "out_coff",
        "kT", "kH", "kW", "sT", "sH", "sW", "pT", "pH", "pW", "is_avg")]


# The C ABI as ctypes sees it: symbol -> (restype, [argtypes]), one line per prototype of include/sfhip.h.  The header is
# the authority — tests/test_cabi_cpu.py compares every line with its prototype, position by position (int -> c_int,
# long -> c_long, float -> c_float, descriptor pointers -> POINTER(ConvDesc / PoolDesc), int* -> POINTER(c_int), every
# other pointer -> c_void_p; mean3 / std3 of sf_clip_prologue are HOST arrays and stay POINTER(c_float)).
_vp, _ci, _cl, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
_CD, _PD, _pi, _pf = ctypes.POINTER(ConvDesc), ctypes.POINTER(PoolDesc), ctypes.POINTER(_ci), ctypes.POINTER(_cf)
_VIEW = [_vp, _ci, _ci]  # a channel slice: pointer, pitch, offset
_ATTN_FWD = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _ci, _vp, _ci, _ci] + [_ci] * 6 + [_vp, _vp]
_BN_BWD = _VIEW * 3 + [_ci] * 7 + [_vp] * 5        # dy, y, z views; N T H W C rep relu; mean invstd + three more
_BN_BWD_SPLIT = _VIEW * 3 + [_ci] * 8 + [_vp] * 5  # ... with nsplit after C
_BN_APPLY_TAIL = _VIEW * 2 + [_vp]                 # dz view, dres view, stream
_SIGNATURES = {
    "sf_abi_version": (_ci, []),
    "sf_build_arch": (ctypes.c_char_p, []),
    # layout, input step, one-channel stem
    "sf_ncthw_to_ndhwc": (_ci, [_vp, _vp] + [_ci] * 9 + [_vp]),
    "sf_ndhwc_to_ncthw": (_ci, [_vp, _ci, _ci, _vp] + [_ci] * 5 + [_vp]),
    "sf_clip_prologue": (_ci, [_vp] + [_ci] * 10 + [_pf] * 2 + [_vp, _ci, _vp, _ci, _ci, _ci, _vp]),
    "sf_clip_prologue_gray": (_ci, [_vp] + [_ci] * 9 + [_cf, _cf, _vp, _ci, _vp, _ci, _ci, _ci, _vp]),
    "sf_clip_views": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp] + [_ci] * 5 + [_vp] * 4 + [_ci, _ci, _ci, _vp]),
    "sf_clip_views_gray": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp] + [_ci] * 4 + [_cf, _cf, _vp, _vp, _ci, _ci, _ci, _vp]),
    "sf_clip_batch": (_ci, [_vp, _vp] + [_ci] * 5 + [_vp] * 4 + [_ci, _ci, _ci, _vp]),
    "sf_clip_batch_gray": (_ci, [_vp, _vp] + [_ci] * 4 + [_cf, _cf, _vp, _vp, _ci, _ci, _ci, _vp]),
    "sf_clip_batch_det": (_ci, [_vp, _vp] + [_ci] * 6 + [_vp] * 4 + [_ci, _ci, _ci, _vp]),
    "sf_clip_batch_mix": (_ci, [_vp, _vp] + [_ci] * 5 + [_vp] * 4 + [_ci, _ci, _ci, _vp]),
    "sf_clip_batch_mix_gray": (_ci, [_vp, _vp] + [_ci] * 4 + [_cf, _cf, _vp, _vp, _ci, _ci, _ci, _vp]),
    "sf_frame_grey_means": (_ci, [_vp, _vp, _ci, _ci, _ci, _pi, _vp]),
    "sf_clip_batch_jitter": (_ci, [_vp, _vp] + [_ci] * 5 + [_vp, _vp, _pi, _vp, _vp, _ci, _ci, _ci, _vp]),
    # streaming demo: device frame ring, window pack, label select
    "sf_stream_push": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp]),
    "sf_stream_window": (_ci, [_vp, _ci, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _ci, _ci, _vp]),
    "sf_label_select": (_ci, [_vp, _ci, _ci, _cf, _pi, _vp]),
    "sf_ensemble_update": (_ci, [_vp] * 4 + [_pi] * 3 + [_ci] * 4 + [_vp]),
    "sf_ensemble_update_ml": (_ci, [_vp] * 3 + [_ci, _vp, _vp, _pi, _pi] + [_ci] * 4 + [_vp]),
    "sf_ncthw1_pack": (_ci, [_vp, _vp] + [_ci] * 7 + [_vp]),
    "sf_stem1_accepts": (_ci, [_ci] * 4),
    "sf_stem1_fwd": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _ci, _ci, _vp]),
    "sf_stem1_wgrad_ws_floats": (_cl, [_ci] * 7),
    "sf_stem1_wgrad": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _vp, _vp]),
    # dense, grouped and depthwise convs
    "sf_conv_fwd": (_ci, [_CD] + [_vp] * 7),
    "sf_conv_fwd_ws_floats": (_cl, [_CD]),
    "sf_conv_fwd_ws": (_ci, [_CD] + [_vp] * 8),
    "sf_conv_fwd_grouped": (_ci, [_CD, _ci, _ci] + [_vp] * 7),
    "sf_conv_stats_ws_floats": (_cl, [_CD]),
    "sf_conv_fwd_stats": (_ci, [_CD] + [_vp] * 7 + [_pi, _vp]),
    "sf_conv_tune": (_ci, [_ci, _ci]),
    "sf_bx_planes_elems": (_cl, [_cl, _ci]),
    "sf_bx_split": (_ci, [_vp, _ci, _ci, _cl, _ci, _vp, _vp]),
    "sf_bx_split_batched": (_ci, [_vp, _vp, _ci, _ci, _vp]),
    "sf_conv_rows_parts": (_ci, [_CD]),
    "sf_conv_pw_ws_floats": (_cl, [_CD, _ci]),
    "sf_conv_pw_stats_floats": (_cl, [_CD]),
    "sf_conv_fwd_pw": (_ci, [_CD] + [_vp] * 9 + [_pi, _vp]),
    "sf_conv_bx_ws_floats": (_cl, [_CD, _ci, _ci]),
    "sf_conv_fwd_bx": (_ci, [_CD] + [_vp] * 10),
    "sf_pack_conv_weight": (_ci, [_vp, _ci, _ci, _ci, _vp, _ci, _vp, _ci, _vp]),
    "sf_pack_conv_weights": (_ci, [_vp, _vp, _ci, _ci, _vp]),
    "sf_dwconv_fwd": (_ci, [_CD] + [_vp] * 7),
    "sf_conv_wgrad_splits": (_ci, [_CD]),
    "sf_conv_wgrad": (_ci, [_CD, _vp, _vp, _ci, _ci, _vp, _vp]),
    "sf_conv_wgrad_bx_splits": (_ci, [_CD]),
    "sf_conv_wgrad_bx_ws_floats": (_cl, [_CD, _ci, _ci]),
    "sf_conv_wgrad_bx": (_ci, [_CD, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp]),
    "sf_conv_wgrad_grouped_splits": (_ci, [_CD, _ci]),
    "sf_conv_wgrad_grouped": (_ci, [_CD, _ci, _vp, _vp, _ci, _ci, _vp, _vp]),
    "sf_conv_wgrad_finish": (_ci, [_vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _vp]),
    "sf_dwconv_dgrad": (_ci, [_CD, _vp, _ci, _ci, _vp, _vp, _ci, _ci, _ci, _vp]),
    "sf_dwconv_wgrad_ws_floats": (_cl, [_CD, _ci]),
    "sf_dwconv_wgrad": (_ci, [_CD, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp]),
    "sf_dwconv_wgrad_param": (_ci, [_CD, _vp, _vp, _ci, _ci, _ci, _vp, _ci, _vp, _vp]),
    "sf_dwconv_dgrad_epi": (_ci, [_CD] + _VIEW * 2 + [_vp, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _vp]),
    # pooling
    "sf_pool_fwd": (_ci, [_PD, _vp, _vp, _vp]),
    "sf_maxpool_fwd_arg": (_ci, [_PD, _vp, _vp, _vp, _vp]),
    "sf_maxpool_bwd_arg": (_ci, [_PD, _vp] + _VIEW * 2 + [_ci, _vp]),
    "sf_maxpool_bwd": (_ci, [_PD, _vp, _vp] + _VIEW * 2 + [_vp]),
    "sf_maxpool_bwd_first": (_ci, [_PD, _vp, _vp] + _VIEW * 2 + [_vp]),
    "sf_avgpool_win_fwd": (_ci, [_PD, _vp, _vp, _vp]),
    "sf_avgpool_win_bwd": (_ci, [_PD] + _VIEW * 2 + [_ci, _vp]),
    # CMDA edges: ECA gate, SpatialAttention
    "sf_tmax_mean_ws_floats": (_cl, [_ci, _ci]),
    "sf_tmax_mean": (_ci, _VIEW + [_ci] * 6 + [_vp, _vp, _vp]),
    "sf_gate_apply": (_ci, _VIEW + [_ci] * 6 + [_vp, _vp, _vp, _vp, _ci] + _VIEW + [_vp]),
    "sf_tmax_dot": (_ci, _VIEW + [_ci] * 6 + _VIEW + [_vp, _vp, _vp]),
    "sf_eca_bwd_apply": (_ci, _VIEW + [_ci] * 6 + _VIEW + [_vp, _vp] + _VIEW + [_vp]),
    "sf_eca_gate_bwd": (_ci, [_vp, _vp, _vp, _ci, _ci, _cf, _vp, _vp, _vp, _vp]),
    "sf_attn_fwd": (_ci, _ATTN_FWD + [_vp]),
    "sf_attn_fwd_ws_floats": (_cl, [_ci] * 3),
    "sf_attn_products_per_fp32": (_ci, [_ci]),
    "sf_attn_fwd_ws": (_ci, _ATTN_FWD + [_vp, _vp]),
    "sf_attn_bwd": (_ci, [_vp, _ci] * 4 + [_vp, _vp, _vp] + [_vp, _ci] * 3 + [_ci] * 4 + [_vp]),
    "sf_attn_bwd_fused_ws_floats": (_cl, [_ci] * 3),
    "sf_attn_bwd_fused": (_ci, [_vp, _ci] * 4 + [_vp, _vp, _vp] + [_vp, _ci] * 3 + [_ci] * 3 + [_vp, _vp]),
    "sf_attn_bwd_variant": (_ci, [_ci] * 3),
    "sf_attn_tune": (_ci, [_ci, _ci]),
    # streaming cross-length and associative attention
    "sf_xattn_accepts": (_ci, [_cl, _cl, _ci, _ci]),
    "sf_xattn_bwd_ws_floats": (_cl, [_ci, _cl, _cl, _ci, _ci]),
    "sf_xattn_fwd": (_ci, [_vp, _ci] * 4 + [_vp, _ci, _cl, _cl, _ci, _ci, _cf, _vp]),
    "sf_xattn_bwd": (_ci, [_vp, _ci] * 4 + [_vp, _vp] + [_vp, _ci] * 3 + [_ci, _ci, _cl, _cl, _ci, _ci, _cf, _vp, _vp]),
    "sf_assoc_accepts": (_ci, [_cl, _cl, _ci, _ci]),
    "sf_gram_splits": (_ci, [_ci, _cl, _ci, _ci]),
    "sf_gram_ws_floats": (_cl, [_ci, _cl, _ci, _ci]),
    "sf_gram": (_ci, [_vp, _ci, _vp, _ci, _vp, _vp, _ci, _cl, _ci, _ci, _cf, _vp, _vp]),
    "sf_rowmat": (_ci, [_vp, _ci, _vp, _vp, _ci, _ci, _cl, _ci, _ci, _cf, _ci, _vp]),
    # BatchNorm forward / backward, affine
    "sf_channel_stats_ws_floats": (_cl, [_ci]),
    "sf_channel_stats": (_ci, _VIEW + [_cl, _ci, _vp, _vp, _vp, _vp]),
    "sf_bn_train_stats": (_ci, _VIEW + [_cl, _ci, _vp, _vp, _cf, _cf] + [_vp] * 9),
    "sf_bn_train_stats_split": (_ci, _VIEW + [_ci, _cl, _ci, _ci, _vp, _vp, _cf, _cf] + [_vp] * 9),
    "sf_bn_train_stats_merge": (_ci, [_vp, _ci, _ci, _vp, _vp, _cf, _cf] + [_vp] * 8),
    "sf_affine_fwd": (_ci, _VIEW + [_ci] * 5 + [_vp, _vp] + _VIEW + [_ci, _ci] + _VIEW + [_ci, _vp]),
    "sf_affine_fwd_split": (_ci, _VIEW + [_ci] * 6 + [_vp, _vp] + _VIEW + [_ci, _ci] + _VIEW + [_ci, _vp]),
    "sf_affine_fwd_mask": (_ci, _VIEW + [_ci] * 5 + [_vp, _vp] + _VIEW + [_ci] + _VIEW + [_vp, _vp]),
    "sf_bn_bwd_ws_floats": (_cl, [_ci]),
    "sf_bn_bwd_reduce": (_ci, _BN_BWD + [_vp]),
    "sf_bn_bwd_reduce_acc": (_ci, _BN_BWD + [_vp, _vp, _vp]),
    "sf_bn_bwd_reduce_split": (_ci, _BN_BWD_SPLIT + [_vp]),
    "sf_bn_bwd_apply": (_ci, _BN_BWD + _BN_APPLY_TAIL),
    "sf_bn_bwd_apply_first": (_ci, _BN_BWD + _BN_APPLY_TAIL),
    "sf_bn_bwd_apply_split": (_ci, _BN_BWD_SPLIT + _BN_APPLY_TAIL),
    "sf_bn_frozen_bwd": (_ci, _VIEW * 3 + [_ci] * 7 + [_vp] * 3 + _VIEW * 2 + [_ci] + [_vp] * 4),
    # elementwise helpers, head, nonlocal softmax
    "sf_head_act_mean": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _vp]),
    "sf_head_act_mean_bwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _vp, _ci, _vp]),
    "sf_copy_channels": (_ci, _VIEW * 2 + [_ci, _cl, _ci, _vp]),
    "sf_channel_shuffle": (_ci, _VIEW * 2 + [_ci, _cl, _ci, _ci, _vp]),
    "sf_gather_add": (_ci, _VIEW + [_ci] + _VIEW + [_cl, _ci, _ci, _vp]),
    "sf_bcast_add": (_ci, _VIEW + [_ci, _cl, _ci, _vp, _cf, _vp]),
    "sf_rowdot": (_ci, _VIEW * 2 + [_cl, _ci, _cf, _vp, _vp]),
    "sf_axpy": (_ci, _VIEW + [_cf] + _VIEW + [_cl, _ci, _ci, _vp]),
    "sf_act_bwd": (_ci, _VIEW * 2 + [_ci] + _VIEW + [_cl, _ci, _ci, _vp]),
    "sf_sigmoid_bwd": (_ci, [_vp, _vp, _vp, _cl, _ci, _vp]),
    "sf_row_softmax_fwd": (_ci, _VIEW + [_cl, _ci, _cf, _vp]),
    "sf_row_softmax_bwd": (_ci, _VIEW * 2 + [_cl, _ci, _cf, _vp]),
    # RoI head
    "sf_roi_tpool_fwd": (_ci, _VIEW + [_ci] * 5 + [_vp, _vp]),
    "sf_roi_align_max_fwd": (_ci, [_vp] + [_ci] * 4 + [_vp, _ci, _ci, _cf, _ci] + _VIEW + [_vp, _vp]),
    "sf_roi_align_max_bwd": (_ci, _VIEW + [_vp, _vp] + [_ci] * 7 + [_cf, _ci] + _VIEW + [_ci, _vp]),
    # Grad-CAM
    "sf_epilogue_bwd": (_ci, _VIEW * 2 + [_ci] * 6 + [_vp, _ci] + _VIEW + [_ci] + _VIEW + [_ci, _vp]),
    "sf_epilogue_bwd_act": (_ci, _VIEW * 2 + [_ci] * 6 + [_vp, _ci, _ci] + _VIEW + [_ci] + _VIEW + [_ci, _vp]),
    "sf_cam_weights": (_ci, _VIEW + [_ci] * 5 + [_vp, _vp]),
    "sf_cam_map_ws_floats": (_cl, [_ci] * 4),
    "sf_cam_map": (_ci, _VIEW + [_vp] + [_ci] * 5 + [_vp, _vp, _vp, _vp]),
    # global-context pooling, per-sample affine (ContextBlock3D, ChannelAttention)
    "sf_ctx_pool_parts": (_ci, [_cl]),
    "sf_ctx_pool_ws_floats": (_cl, [_ci, _cl, _ci]),
    "sf_ctx_pool_fwd": (_ci, _VIEW + [_ci, _cl, _ci] + [_vp] * 6),
    "sf_ctx_pool_bwd": (_ci, _VIEW + [_ci, _cl, _ci] + [_vp] * 5 + _VIEW + [_ci, _vp, _vp, _ci, _vp, _vp]),
    "sf_sample_affine_ws_floats": (_cl, [_ci, _cl, _ci]),
    "sf_sample_affine_fwd": (_ci, _VIEW + [_ci, _cl, _ci, _vp, _vp] + _VIEW + [_vp]),
    "sf_sample_affine_bwd": (_ci, _VIEW * 2 + [_ci, _cl, _ci, _vp] + _VIEW + [_ci, _vp, _vp, _vp, _vp]),
    # stripe pooling, per-stripe broadcast add (Stripe_NonLocalBlock)
    "sf_stripe_pool_fwd": (_ci, _VIEW + [_ci] * 7 + _VIEW + [_vp, _vp]),
    "sf_stripe_add_fwd": (_ci, _VIEW * 2 + [_ci] * 6 + _VIEW + [_vp]),
    "sf_stripe_pool_bwd": (_ci, _VIEW * 3 + [_vp] + [_ci] * 6 + _VIEW + [_ci, _vp]),
    # training-step tail: loss + top-k, one-launch SGD
    "sf_ce_topk": (_ci, [_vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _pi, _ci, _vp, _vp]),
    "sf_sgd_chunk_elems": (_ci, []),
    "sf_sgd_step": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _ci, _vp, _ci, _vp]),
    # multi-label / detection loss, one-call Adam
    "sf_bce": (_ci, [_vp, _ci, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _pi, _ci, _vp, _vp]),
    "sf_adam_step": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _ci, _vp, _ci, _vp]),
    # class-weighted losses
    "sf_ce_topk_w": (_ci, [_vp, _ci, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _pi, _ci, _vp, _vp]),
    "sf_bce_w": (_ci, [_vp, _ci, _vp, _ci, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _pi, _ci, _vp, _vp]),
    # soft targets: label smoothing, mixup and CutMix
    "sf_ce_mix": (_ci, [_vp, _ci, _vp, _vp, _vp, _ci, _ci, _ci, _cf, _vp, _vp, _pi, _ci, _vp, _vp]),
    # gradient clipping: global norm (two launches), scale, value clamp
    "sf_grad_norm": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _pi, _ci, _vp]),
    "sf_grad_scale": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _vp, _vp]),
    "sf_grad_clamp": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _vp, _vp]),
    # large-batch optimizers: one-call AdamW, per-tensor LARS trust ratios (two launches) and the SGD step behind them
    "sf_adamw_step": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _ci, _vp, _ci, _vp]),
    "sf_lars_sgd_step": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _ci, _vp]),
    "sf_lars_ratios": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp]),
    # averaged weights: one-launch EMA / SWA / running-mean update with a device-side count, swap / copy of the pairs
    "sf_avg_update": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp]),
    "sf_avg_exchange": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _ci, _vp]),
    # training telemetry: per-tensor statistics and sign-and-exponent histograms into a device-side ring (two launches)
    "sf_tensor_stats_ws_bytes": (_cl, [_ci]),
    "sf_tensor_stats": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _vp, _cl, _vp, _ci, _ci, _pi, _vp]),
    # evaluation: top-k errors of a batch, the epoch's row store, mean average precision
    "sf_topk_errors": (_ci, [_vp, _ci, _vp, _ci, _ci, _ci, _vp, _pi, _ci, _vp]),
    "sf_rows_append": (_ci, [_vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _pi, _ci, _vp]),
    "sf_map_ws_bytes": (_cl, [_ci, _ci]),
    "sf_map": (_ci, [_vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp]),
    # per-class evaluation: confusion matrix and per-class hits of a batch, the class report
    "sf_confusion_small_kmax": (_ci, []),
    "sf_confusion_update": (_ci, [_vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp]),
    "sf_class_report": (_ci, [_vp, _vp, _ci, _vp, _vp, _vp]),
    "sf_class_weights": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp]),
    # detection evaluation: AVA frame-mAP — true-positive matching, per-class average precision
    "sf_ava_ws_bytes": (_cl, [_ci, _ci, _ci]),
    "sf_ava_match": (_ci, [_vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _ci, _vp, _ci, _ci] + [_vp] * 5),
    "sf_ava_ap": (_ci, [_vp, _ci, _vp, _vp, _ci, _ci, _vp, _vp, _ci] + [_vp] * 4),
}
EXPORTS = list(_SIGNATURES)


def lib_path():
    return _LIB_PATH


def lib():
    """Load libsfhip.so (built by `make -C efficient-slowfast_amd/csrc` / __graft_entry__.build()) and hand ctypes the
    signature of every entry point."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise SfhipError(
                "libsfhip.so not found at %s — build it with `make -C efficient-slowfast_amd/csrc` "
                "(there is no CPU fallback for the SlowFast hot path)" % _LIB_PATH)
        L = ctypes.CDLL(_LIB_PATH)
        for name, (restype, argtypes) in _SIGNATURES.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise SfhipError("%s does not export %s — rebuild it with `make -C efficient-slowfast_amd/csrc`" % (
                    _LIB_PATH, name))
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise SfhipError("%s failed: %s" % (what, _ERR.get(rc, rc)))


CALLS = 0  # C-ABI calls issued by this process (every entry point takes the stream: counted there; bench.py's launch_bound block)


def _stream():
    global CALLS
    CALLS += 1
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _slice_base(a):  # slice base pointer: buffer pointer + channel offset
    return ctypes.c_void_p(a.buf.data_ptr() + 4 * a.coff)


EVENT_TRACE = None  # bench.py sets this to a list: (tag, start_event, end_event) per traced launch


def _traced(tag, fn):
    """Run `fn` (the launches of one C-ABI call on the current stream) between two HIP events when tracing is on."""
    if EVENT_TRACE is None:
        return fn()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn()
    e1.record()
    EVENT_TRACE.append((tag, e0, e1))
    return rc


def _call(name, *args, tag=None, what=None, allow=()):
    """One stream-taking entry point: `name`(*args, the current stream), under _traced when `tag` is given.  A code other
    than 0 raises SfhipError labelled `what` (default: the symbol) unless it is in `allow`; the code is returned."""
    fn = getattr(lib(), name)
    if tag is None:
        rc = fn(*args, _stream())
    else:
        rc = _traced(tag, lambda: fn(*args, _stream()))
    if rc not in allow:
        _check(rc, what or name)
    return rc


def _require_gpu(t, what):
    if not t.is_cuda:
        raise SfhipError("%s: tensor is on %s — the SlowFast hot path only runs on an MI355X GPU "
                         "(no CPU fallback)" % (what, t.device))
    if t.dtype != torch.float32:
        raise SfhipError("%s: expected float32, got %s" % (what, t.dtype))
    if t.device.index != torch.cuda.current_device():
        # kernels are enqueued on the CURRENT device's stream: a tensor of another GPU would be launched on the wrong one
        raise SfhipError("%s: tensor is on %s but the current device is cuda:%d — call torch.cuda.set_device(%d) (one "
                         "process per GPU)" % (what, t.device, torch.cuda.current_device(), t.device.index))


# ------------------------------------------------------------------------------------------------ Act
class Act(object):
    """NDHWC activation view: `buf` is a contiguous [N, T, H, W, pitch] tensor, the view is channels
    [coff, coff + C)."""
    __slots__ = ("buf", "coff", "C")

    def __init__(self, buf, coff=0, C=None):
        assert buf.dim() == 5 and buf.is_contiguous()
        self.buf = buf
        self.coff = coff
        self.C = buf.shape[4] - coff if C is None else C

    N = property(lambda s: s.buf.shape[0])
    T = property(lambda s: s.buf.shape[1])
    H = property(lambda s: s.buf.shape[2])
    W = property(lambda s: s.buf.shape[3])
    cs = property(lambda s: s.buf.shape[4])
    rows = property(lambda s: s.buf.shape[0] * s.buf.shape[1] * s.buf.shape[2] * s.buf.shape[3])

    def slice(self, off, C):
        assert 0 <= off and off + C <= self.C
        return Act(self.buf, self.coff + off, C)

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr())

    @property
    def shape_ncthw(self):
        return (self.N, self.C, self.T, self.H, self.W)

    def __repr__(self):
        return "Act(N=%d,T=%d,H=%d,W=%d,C=%d@%d/%d)" % (self.N, self.T, self.H, self.W, self.C, self.coff, self.cs)


def new_act(like_or_dev, N, T, H, W, C, before=0, after=0):
    """Allocate [N,T,H,W,before+C+after] and return the middle C-channel view."""
    dev = like_or_dev.buf.device if isinstance(like_or_dev, Act) else like_or_dev
    buf = torch.empty((N, T, H, W, before + C + after), dtype=torch.float32, device=dev)
    return Act(buf, before, C)


def from_ncthw(x, cpad=None, ph=0, pw=0, wp=None):
    """NCTHW torch tensor -> (optionally channel/border padded) NDHWC Act."""
    _require_gpu(x, "from_ncthw")
    x = x.contiguous()
    N, C, T, H, W = x.shape
    cpad = C if cpad is None else cpad
    wp = W + 2 * pw if wp is None else wp
    buf = torch.empty((N, T, H + 2 * ph, wp, cpad), dtype=torch.float32, device=x.device)
    _call("sf_ncthw_to_ndhwc", _ptr(x), _ptr(buf), N, C, T, H, W, cpad, ph, pw, wp)
    return Act(buf, 0, cpad)


class PackedClip(object):
    """A pathway input already in the stem's layout: buf [N, T, H+2*ph, Wp, 4] fp32 (channels padded to 4, zero
    H/W borders) — or, for a one-channel (grayscale) clip, [N, T, H+2*ph, Wp, 1]: one float per pixel.  Produced by
    `clip_prologue`; accepted by the model in place of an NCTHW tensor."""

    def __init__(self, buf, channels, H, W, ph, pw):
        if buf.dim() != 5 or buf.shape[4] != (1 if channels == 1 else 4):
            raise ValueError("PackedClip: a %d-channel clip is packed as [N, T, H+2ph, Wp, %d], got %s" % (
                channels, 1 if channels == 1 else 4, tuple(buf.shape)))
        self.buf, self.C, self.H, self.W, self.ph, self.pw = buf, channels, H, W, ph, pw

    @property
    def shape(self):  # the logical NCTHW shape the reference's tensor would have
        return (self.buf.shape[0], self.C, self.buf.shape[1], self.H, self.W)

    @property
    def Wp(self):
        return self.buf.shape[3]

    def to_ncthw(self):
        v = self.buf[:, :, self.ph:self.ph + self.H, self.pw:self.pw + self.W, :self.C]
        return v.permute(0, 4, 1, 2, 3).contiguous()


def clip_prologue(clip_u8, dst, new_hw, yx, crop, flip, mean, std, frame_idx=None, reverse=False, ph=0, pw=0):
    """One decoded clip (uint8 [T,H,W,3], device) -> dst (float [n_frames, crop+2ph, Wp, 4] view of a PackedClip
    buffer): normalise, bilinear short-side scale, crop, flip, frame selection in one kernel.  A grayscale clip (uint8
    [T,H,W] or [T,H,W,1], one-element mean / std) -> dst [n_frames, crop+2ph, Wp, 1], the one-channel stem layout."""
    _require_gpu(dst, "clip_prologue")
    if not clip_u8.is_cuda:
        raise SfhipError("clip_prologue: the uint8 clip is on %s — copy it to the GPU first" % clip_u8.device)
    assert clip_u8.dtype == torch.uint8 and clip_u8.dim() in (3, 4) and clip_u8.is_contiguous()
    gray = clip_u8.dim() == 3 or clip_u8.shape[3] == 1
    assert gray or clip_u8.shape[3] == 3
    assert dst.dtype == torch.float32 and dst.is_contiguous() and dst.dim() == 4 and dst.shape[3] == (1 if gray else 4)
    T, H, W = clip_u8.shape[:3]
    n = dst.shape[0]
    assert dst.shape[1] == crop + 2 * ph
    head = (_ptr(clip_u8), T, H, W, int(new_hw[0]), int(new_hw[1]), int(yx[0]), int(yx[1]), int(crop), 1 if flip else 0)
    tail = (_ptr(frame_idx), n, _ptr(dst), ph, pw, dst.shape[2])
    if gray:
        assert len(mean) == 1 and len(std) == 1, "a one-channel clip takes a one-element mean / std"
        assert not reverse, "DATA.REVERSE_INPUT_CHANNEL has no meaning for a one-channel clip"
        _call("sf_clip_prologue_gray", *head, float(mean[0]), float(std[0]), *tail)
        return dst
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
    _call("sf_clip_prologue", *head, 1 if reverse else 0, m3, s3, *tail)
    return dst


def clip_views(video_u8, table_host, table, n_slow, crop, mean, std, fast, slow=None, reverse=False, ph=0, pw=0):
    """All V views of one decoded video (uint8 [T,H,W,3], or [T,H,W] / [T,H,W,1] grayscale, device) in one launch ->
    fast [V, n_fast, crop+2ph, Wp, 4 | 1] and slow [V, n_slow, ...] (None with n_slow == 0: single pathway), the
    PackedClip layouts `clip_prologue` writes.  table_host: the int32 CPU view table (V rows new_h, new_w, y0, x0, flip;
    V * n_fast frame indices; n_slow Slow positions), table: its device copy."""
    _require_gpu(fast, "clip_views")
    if not (video_u8.is_cuda and table.is_cuda) or table_host.is_cuda:
        raise SfhipError("clip_views: the video and the view table's copy live on the GPU, table_host on the host")
    assert video_u8.dtype == torch.uint8 and video_u8.dim() in (3, 4) and video_u8.is_contiguous()
    gray = video_u8.dim() == 3 or video_u8.shape[3] == 1
    assert gray or video_u8.shape[3] == 3
    assert fast.is_contiguous() and fast.dim() == 5 and fast.shape[4] == (1 if gray else 4)
    V, n_fast = fast.shape[:2]
    assert table_host.dtype == torch.int32 and table.dtype == torch.int32 and table_host.is_contiguous()
    assert table.is_contiguous() and table_host.numel() == table.numel() == V * (5 + n_fast) + n_slow
    if slow is not None:
        _require_gpu(slow, "clip_views")
        assert slow.is_contiguous() and tuple(slow.shape) == (V, n_slow) + tuple(fast.shape[2:])
    T, H, W = video_u8.shape[:3]
    head = (_ptr(video_u8), T, H, W, _ptr(table_host), _ptr(table), V, n_fast, int(n_slow), int(crop))
    tail = (_ptr(fast), _ptr(slow), ph, pw, fast.shape[3])
    if gray:
        assert len(mean) == 1 and len(std) == 1, "a one-channel video takes a one-element mean / std"
        assert not reverse, "DATA.REVERSE_INPUT_CHANNEL has no meaning for a one-channel video"
        _call("sf_clip_views_gray", *head, float(mean[0]), float(std[0]), *tail)
    else:
        m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
        s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
        _call("sf_clip_views", *head, 1 if reverse else 0, ctypes.cast(m3, _vp), ctypes.cast(s3, _vp), *tail)
    return fast, slow


def clip_batch(table_host, table, n_slow, crop, mean, std, fast, slow=None, gray=False, reverse=False, ph=0, pw=0):
    """All B clips of one training batch (B separate uint8 device spans, named by address in the table) in one launch ->
    fast [B, n_fast, crop+2ph, Wp, 4 | 1] and slow [B, n_slow, ...] (None with n_slow == 0: single pathway), the
    PackedClip layouts `clip_prologue` writes.  table_host: the int64 CPU batch table (B rows address, T, H, W, new_h,
    new_w, y0, x0, flip; B * n_fast frame indices; n_slow Slow positions), table: its device copy.  The caller keeps the
    spans alive until the launch has run.  gray: one-channel spans (the buffers' last extent is 1)."""
    _require_gpu(fast, "clip_batch")
    if not table.is_cuda or table_host.is_cuda:
        raise SfhipError("clip_batch: the batch table's copy lives on the GPU, table_host on the host")
    assert fast.is_contiguous() and fast.dim() == 5 and fast.shape[4] == (1 if gray else 4)
    B, n_fast = fast.shape[:2]
    assert table_host.dtype == torch.int64 and table.dtype == torch.int64 and table_host.is_contiguous()
    assert table.is_contiguous() and table_host.numel() == table.numel() == B * (9 + n_fast) + n_slow
    if slow is not None:
        _require_gpu(slow, "clip_batch")
        assert slow.is_contiguous() and tuple(slow.shape) == (B, n_slow) + tuple(fast.shape[2:])
    head = (_ptr(table_host), _ptr(table), B, n_fast, int(n_slow), int(crop))
    tail = (_ptr(fast), _ptr(slow), ph, pw, fast.shape[3])
    if gray:
        assert len(mean) == 1 and len(std) == 1, "one-channel clips take a one-element mean / std"
        assert not reverse, "DATA.REVERSE_INPUT_CHANNEL has no meaning for one-channel clips"
        _call("sf_clip_batch_gray", *head, float(mean[0]), float(std[0]), *tail)
    else:
        m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
        s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
        _call("sf_clip_batch", *head, 1 if reverse else 0, ctypes.cast(m3, _vp), ctypes.cast(s3, _vp), *tail)
    return fast, slow


SF_MIX_ROW = 7  # include/sfhip.h: partner row, mode, lam as float32 bits, y0, x0, y1, x1 (int64 each)


def clip_batch_mix(table_host, table, n_slow, crop, mean, std, fast, slow=None, gray=False, reverse=False, ph=0, pw=0):
    """`clip_batch` with mixup / CutMix inside the launch (`sf_clip_batch_mix` / `sf_clip_batch_mix_gray`): the table is
    clip_batch's followed by B mix rows (partner row, mode 0 none / 1 mixup / 2 CutMix, lam as float32 bits, the box y0,
    x0, y1, x1 in output crop coordinates).  Everything else — buffers, layouts, the caller keeping the spans alive — is
    clip_batch's."""
    _require_gpu(fast, "clip_batch_mix")
    if not table.is_cuda or table_host.is_cuda:
        raise SfhipError("clip_batch_mix: the batch table's copy lives on the GPU, table_host on the host")
    assert fast.is_contiguous() and fast.dim() == 5 and fast.shape[4] == (1 if gray else 4)
    B, n_fast = fast.shape[:2]
    assert table_host.dtype == torch.int64 and table.dtype == torch.int64 and table_host.is_contiguous()
    assert table.is_contiguous() and table_host.numel() == table.numel() == B * (9 + n_fast + SF_MIX_ROW) + n_slow
    if slow is not None:
        _require_gpu(slow, "clip_batch_mix")
        assert slow.is_contiguous() and tuple(slow.shape) == (B, n_slow) + tuple(fast.shape[2:])
    head = (_ptr(table_host), _ptr(table), B, n_fast, int(n_slow), int(crop))
    tail = (_ptr(fast), _ptr(slow), ph, pw, fast.shape[3])
    if gray:
        assert len(mean) == 1 and len(std) == 1, "one-channel clips take a one-element mean / std"
        assert not reverse, "DATA.REVERSE_INPUT_CHANNEL has no meaning for one-channel clips"
        _call("sf_clip_batch_mix_gray", *head, float(mean[0]), float(std[0]), *tail)
    else:
        m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
        s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
        _call("sf_clip_batch_mix", *head, 1 if reverse else 0, ctypes.cast(m3, _vp), ctypes.cast(s3, _vp), *tail)
    return fast, slow


SF_JITTER_ROW = 3  # include/sfhip.h: brightness, contrast and colour factors as float32 bits (int64 each)


def _jitter_table(table_host, table, B, n_fast, n_slow, means, what):
    """The checks the two jitter entries share: the table pair, its length, and `means` int32 [B, n_fast] on the GPU."""
    if not means.is_cuda:
        raise SfhipError("%s: means is on %s — the SlowFast hot path only runs on an MI355X GPU (no CPU fallback)" % (
            what, means.device))
    if not table.is_cuda or table_host.is_cuda:
        raise SfhipError("%s: the batch table's copy lives on the GPU, table_host on the host" % what)
    assert means.dtype == torch.int32 and means.is_contiguous() and tuple(means.shape) == (B, n_fast)
    assert table_host.dtype == torch.int64 and table.dtype == torch.int64 and table_host.is_contiguous()
    assert table.is_contiguous() and table_host.numel() == table.numel() == B * (9 + n_fast + SF_JITTER_ROW) + n_slow


def frame_grey_means(table_host, table, n_slow, means):
    """The grey mean of every (clip, Fast frame) of a batch after the clip's brightness stage (`sf_frame_grey_means`):
    what ImageEnhance.Contrast blends against.  The table is clip_batch's followed by B jitter rows (brightness,
    contrast, colour as float32 bits); means: int32 [B, n_fast] on the GPU, every element written."""
    B, n_fast = means.shape
    _jitter_table(table_host, table, B, n_fast, n_slow, means, "frame_grey_means")
    _call("sf_frame_grey_means", _ptr(table_host), _ptr(table), B, n_fast, int(n_slow), _iptr(means))
    return means


def clip_batch_jitter(table_host, table, n_slow, crop, mean, std, means, fast, slow=None, reverse=False, ph=0, pw=0):
    """`clip_batch` with Jester's colour jitter (PIL's ImageEnhance.Brightness, Contrast, Color) inside the launch
    (`sf_clip_batch_jitter`): the table is clip_batch's followed by B jitter rows, `means` an int32 [B, n_fast] device
    scratch the call fills first (one launch) and the clip launch reads.  RGB spans only.  Everything else — buffers,
    layouts, the caller keeping the spans alive — is clip_batch's."""
    _require_gpu(fast, "clip_batch_jitter")
    assert fast.is_contiguous() and fast.dim() == 5 and fast.shape[4] == 4
    B, n_fast = fast.shape[:2]
    _jitter_table(table_host, table, B, n_fast, n_slow, means, "clip_batch_jitter")
    if slow is not None:
        _require_gpu(slow, "clip_batch_jitter")
        assert slow.is_contiguous() and tuple(slow.shape) == (B, n_slow) + tuple(fast.shape[2:])
    assert len(mean) == 3 and len(std) == 3, "the colour jitter is three-channel"
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
    _call("sf_clip_batch_jitter", _ptr(table_host), _ptr(table), B, n_fast, int(n_slow), int(crop), 1 if reverse else 0,
          ctypes.cast(m3, _vp), ctypes.cast(s3, _vp), _iptr(means), _ptr(fast), _ptr(slow), ph, pw, fast.shape[3])
    return fast, slow


def clip_batch_det(table_host, table, n_slow, win_hw, mean, std, fast, slow=None, reverse=False, ph=0, pw=0):
    """All B clips of one detection (AVA) batch — B separate uint8 BGR device spans, named by address in the table — in
    one launch -> fast [B, n_fast, win_h+2ph, Wp, 4] and slow [B, n_slow, ...] (None with n_slow == 0: single pathway),
    the PackedClip layout.  The arithmetic is the AVA loader's (resample u / 255, + lighting offset, normalise, then
    BGR -> RGB with `reverse`), not clip_batch's.  table_host: the int64 CPU table (B rows address, T, H, W, new_h, new_w,
    y0, x0, flip, three lighting offsets as float32 bits; B * n_fast frame indices; n_slow Slow positions; a tail the
    kernel does not read may follow), table: its device copy.  win_hw: the output window (win_h, win_w), shared by the
    batch.  mean / std: three values in source (BGR) order.  The caller keeps the spans alive until the launch has run."""
    _require_gpu(fast, "clip_batch_det")
    if not table.is_cuda or table_host.is_cuda:
        raise SfhipError("clip_batch_det: the batch table's copy lives on the GPU, table_host on the host")
    win_h, win_w = int(win_hw[0]), int(win_hw[1])
    assert fast.is_contiguous() and fast.dim() == 5 and fast.shape[4] == 4 and fast.shape[2] == win_h + 2 * ph
    B, n_fast = fast.shape[:2]
    assert table_host.dtype == torch.int64 and table.dtype == torch.int64 and table_host.is_contiguous()
    assert table.is_contiguous() and table_host.numel() == table.numel() >= B * (12 + n_fast) + n_slow
    if slow is not None:
        _require_gpu(slow, "clip_batch_det")
        assert slow.is_contiguous() and tuple(slow.shape) == (B, n_slow) + tuple(fast.shape[2:])
    assert len(mean) == 3 and len(std) == 3, "the AVA path is three-channel"
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
    _call("sf_clip_batch_det", _ptr(table_host), _ptr(table), B, n_fast, int(n_slow), win_h, win_w, 1 if reverse else 0,
          ctypes.cast(m3, _vp), ctypes.cast(s3, _vp), _ptr(fast), _ptr(slow), ph, pw, fast.shape[3])
    return fast, slow


def _iptr(t):  # a device int32 array where the header says `int*`
    return ctypes.cast(ctypes.c_void_p(t.data_ptr()), _pi)


def stream_push(frame_u8, ring, slot, new_hw, mean, std, ph=0, pw=0):
    """One camera frame (uint8 [H, W, 3], device, BGR) -> slot `slot` of ring [S, new_h+2ph, Wp, 4]: BGR -> RGB, bilinear
    scale to new_hw, normalise, the whole padded plane written (the PackedClip layout).  mean / std: three values in RGB
    order."""
    _require_gpu(ring, "stream_push")
    if not frame_u8.is_cuda:
        raise SfhipError("stream_push: the uint8 frame is on %s — copy it to the GPU first" % frame_u8.device)
    assert frame_u8.dtype == torch.uint8 and frame_u8.dim() == 3 and frame_u8.shape[2] == 3 and frame_u8.is_contiguous()
    new_h, new_w = int(new_hw[0]), int(new_hw[1])
    assert ring.is_contiguous() and ring.dim() == 4 and ring.shape[3] == 4 and ring.shape[1] == new_h + 2 * ph
    assert len(mean) == 3 and len(std) == 3, "the streaming demo is three-channel"
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
    _call("sf_stream_push", _ptr(frame_u8), frame_u8.shape[0], frame_u8.shape[1], new_h, new_w, ctypes.cast(m3, _vp),
          ctypes.cast(s3, _vp), _ptr(ring), ring.shape[0], int(slot), ph, pw, ring.shape[2])
    return ring


def stream_window(ring, head, fast_idx, slow_idx, fast, slow=None):
    """Both pathways of the window whose oldest frame is in ring slot `head`, in one launch: fast [n_fast, Hp, Wp, 4]
    frame j = ring slot (head + fast_idx[j]) % S, slow [n_slow, Hp, Wp, 4] frame j = Fast frame slow_idx[j] (slow None and
    slow_idx None or empty: single pathway).  fast_idx / slow_idx: int32 device tensors."""
    _require_gpu(ring, "stream_window")
    _require_gpu(fast, "stream_window")
    assert ring.is_contiguous() and ring.dim() == 4 and ring.shape[3] == 4
    assert fast.is_contiguous() and fast.dim() == 4 and tuple(fast.shape[1:]) == tuple(ring.shape[1:])
    assert fast_idx.is_cuda and fast_idx.dtype == torch.int32 and fast_idx.is_contiguous()
    n_fast, n_slow = fast.shape[0], 0
    assert fast_idx.numel() == n_fast
    if slow is not None:
        _require_gpu(slow, "stream_window")
        n_slow = slow.shape[0]
        assert slow.is_contiguous() and tuple(slow.shape[1:]) == tuple(ring.shape[1:])
        assert slow_idx.is_cuda and slow_idx.dtype == torch.int32 and slow_idx.is_contiguous()
        assert slow_idx.numel() == n_slow
    _call("sf_stream_window", _ptr(ring), ring.shape[0], int(head), _ptr(fast_idx), n_fast,
          _ptr(slow_idx) if n_slow else None, n_slow, _ptr(fast), _ptr(slow), ring.shape[1], ring.shape[2])
    return fast, slow


def label_select(preds, thr, out):
    """preds [R, C] fp32 -> out int32 [R, 2 + C]: per row count, argmax (first maximal index, -1 for a row of NaNs), then
    the `count` class indices with preds > thr in ascending order (torch.nonzero's); entries past them are left as they
    were.  No allocation, no synchronisation."""
    _require_gpu(preds, "label_select")
    assert preds.dim() == 2 and preds.is_contiguous()
    R, C = preds.shape
    assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (R, 2 + C)
    _call("sf_label_select", _ptr(preds), R, C, float(thr), _iptr(out))
    return out


def ensemble_update(preds, video_idx, labels, video_preds, video_labels, clip_count, bad_count, mode):
    """TestMeter.update_stats on the device: preds [B,K] fp32, video_idx / labels int32 [B] (labels may be None) folded
    into video_preds [Nv,K], video_labels / clip_count int32 [Nv]; mode 0 sum, 1 max.  bad_count: int32 [1], the number
    of clips skipped because their video index was outside [0, Nv)."""
    _require_gpu(preds, "ensemble_update")
    _require_gpu(video_preds, "ensemble_update")
    ints = (video_idx, video_labels, clip_count, bad_count) + (() if labels is None else (labels,))
    assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in ints)
    assert preds.dim() == 2 and preds.is_contiguous() and video_preds.dim() == 2 and video_preds.is_contiguous()
    B, K = preds.shape
    Nv = video_preds.shape[0]
    assert video_preds.shape[1] == K and video_idx.numel() == B and (labels is None or labels.numel() == B)
    assert video_labels.numel() == Nv and clip_count.numel() == Nv and bad_count.numel() == 1
    _call("sf_ensemble_update", _ptr(preds), _ptr(video_idx), _ptr(labels), _ptr(video_preds), _iptr(video_labels),
          _iptr(clip_count), _iptr(bad_count), B, K, Nv, int(mode))


def _rows(t, what):
    """A [N, K] fp32 GPU tensor as the kernels read it: unit column stride, row stride >= K.  Returns (tensor, stride)."""
    _require_gpu(t, what)
    N, K = t.shape
    if t.stride(1) != 1 or (N > 1 and t.stride(0) < K):
        t = t.contiguous()
    return t, (t.stride(0) if N > 1 else K)


def ensemble_update_ml(preds, video_idx, labels, video_preds, video_labels, clip_count, bad_count, mode):
    """The multi-label TestMeter.update_stats on the device: preds / labels fp32 [B,K], video_idx int32 [B] folded into
    video_preds / video_labels fp32 [Nv,K] and clip_count int32 [Nv]; mode 0 sum, 1 max.  bad_count: int32 [2], clips
    whose video index was outside [0, Nv) and label rows that differed from the ones their video already held."""
    _require_gpu(preds, "ensemble_update_ml")
    _require_gpu(video_preds, "ensemble_update_ml")
    _require_gpu(video_labels, "ensemble_update_ml")
    assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in (video_idx, clip_count, bad_count))
    assert preds.dim() == 2 and preds.is_contiguous() and video_preds.dim() == 2 and video_preds.is_contiguous()
    B, K = preds.shape
    Nv = video_preds.shape[0]
    assert video_preds.shape[1] == K and video_idx.numel() == B and tuple(labels.shape) == (B, K)
    assert video_labels.is_contiguous() and tuple(video_labels.shape) == (Nv, K)
    assert clip_count.numel() == Nv and bad_count.numel() == 2
    labels, ldl = _rows(labels, "ensemble_update_ml")
    _call("sf_ensemble_update_ml", _ptr(preds), _ptr(video_idx), _ptr(labels), int(ldl), _ptr(video_preds),
          _ptr(video_labels), _iptr(clip_count), _iptr(bad_count), B, K, Nv, int(mode))


def rows_append(preds, labels, store_preds, store_labels, cursor):
    """ValMeter.update_predictions on the device: preds / labels fp32 [N,K] (row views) are copied to rows cursor[0]..
    of store_preds / store_labels fp32 [cap,K]; cursor int32 [2] = {rows filled, rows refused for want of room}."""
    if preds.dim() != 2 or tuple(labels.shape) != tuple(preds.shape):
        raise ValueError("rows_append: preds [N, K] and labels [N, K], got %s and %s" % (tuple(preds.shape),
                                                                                         tuple(labels.shape)))
    N, K = preds.shape
    preds, ldp = _rows(preds, "rows_append")
    labels, ldl = _rows(labels, "rows_append")
    for t in (store_preds, store_labels):
        _require_gpu(t, "rows_append")
        assert t.is_contiguous() and t.dim() == 2 and t.shape[1] == K and t.shape[0] == store_preds.shape[0]
    assert cursor.is_cuda and cursor.dtype == torch.int32 and cursor.is_contiguous() and cursor.numel() == 2
    _call("sf_rows_append", _ptr(preds), int(ldp), _ptr(labels), int(ldl), N, K, _ptr(store_preds), _ptr(store_labels),
          _iptr(cursor), store_preds.shape[0], tag="rows_append")


def mean_ap(scores, labels, out=None, per_class=False):
    """One `sf_map` call (two launches, no host read): scores / labels fp32 [N,C] (row views) -> out fp64 [3] = {mAP,
    classes with a positive, refused elements}, and the per-class AP fp64 [C] (-1: left out) when asked for."""
    if scores.dim() != 2 or tuple(labels.shape) != tuple(scores.shape):
        raise ValueError("mean_ap: scores [N, C] and labels [N, C], got %s and %s" % (tuple(scores.shape),
                                                                                       tuple(labels.shape)))
    N, C = scores.shape
    scores, lds = _rows(scores, "mean_ap")
    labels, ldl = _rows(labels, "mean_ap")
    nbytes = lib().sf_map_ws_bytes(N, C)
    if nbytes <= 0:
        raise SfhipError("mean_ap: %d x %d is outside the kernel's range" % (N, C))
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=scores.device)
    if out is None:
        out = torch.empty((3,), dtype=torch.float64, device=scores.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == 3
    ap = torch.empty((C,), dtype=torch.float64, device=scores.device) if per_class else None
    _call("sf_map", _ptr(scores), int(lds), _ptr(labels), int(ldl), N, C, _ptr(ws), _ptr(out), _ptr(ap), tag="map")
    return (out, ap) if per_class else out


def _counters(t, shape, dtype, what):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise SfhipError("%s: expected a contiguous %s GPU tensor of shape %s, got %s %s on %s" % (
            what, dtype, tuple(shape), t.dtype, tuple(t.shape), t.device))


def confusion_update(preds, labels, k_hi, conf, hits, refused):
    """One `sf_confusion_update` launch (no host read): preds fp32 [N,K] (a row view), labels int64 [N] are ADDED to conf
    int64 [K,K] ([true, predicted]), hits int64 [K,2] (label within the top 1 / top k_hi, per true class) and refused
    int64 [2] (rows with a label outside [0, K); rows holding a NaN or an infinity)."""
    if preds.dim() != 2 or labels.dim() != 1 or labels.shape[0] != preds.shape[0]:
        raise ValueError("confusion_update: preds [N, K] and labels [N], got %s and %s" % (tuple(preds.shape),
                                                                                           tuple(labels.shape)))
    N, K = preds.shape
    preds, ld = _rows(preds, "confusion_update")
    if labels.dtype != torch.int64 or not labels.is_cuda:
        raise ValueError("confusion_update: labels must be int64 on the GPU, got %s on %s" % (labels.dtype,
                                                                                              labels.device))
    labels = labels.contiguous()
    _counters(conf, (K, K), torch.int64, "confusion_update: conf")
    _counters(hits, (K, 2), torch.int64, "confusion_update: hits")
    _counters(refused, (2,), torch.int64, "confusion_update: refused")
    _call("sf_confusion_update", _ptr(preds), int(ld), _ptr(labels), N, K, int(k_hi), _ptr(conf), _ptr(hits),
          _ptr(refused), tag="confusion_update")


def class_report(conf, hits, out=None, per_class=None):
    """One `sf_class_report` launch (no host read): conf int64 [K,K], hits int64 [K,2] -> out fp64 [8] = {samples,
    accuracy, mean-class accuracy, macro precision, macro recall, macro F1, classes with support, classes never
    predicted} and per_class fp64 [K,6] = {support, precision, recall, F1, top-1 accuracy, top-k accuracy}."""
    if conf.dim() != 2 or conf.shape[0] != conf.shape[1]:
        raise ValueError("class_report: conf [K, K], got %s" % (tuple(conf.shape),))
    K = conf.shape[0]
    _counters(conf, (K, K), torch.int64, "class_report: conf")
    _counters(hits, (K, 2), torch.int64, "class_report: hits")
    if out is None:
        out = torch.empty((8,), dtype=torch.float64, device=conf.device)
    if per_class is None:
        per_class = torch.empty((K, 6), dtype=torch.float64, device=conf.device)
    _counters(out, (8,), torch.float64, "class_report: out")
    _counters(per_class, (K, 6), torch.float64, "class_report: per_class")
    _call("sf_class_report", _ptr(conf), _ptr(hits), K, _ptr(out), _ptr(per_class), tag="class_report")
    return out, per_class


WEIGHT_SCHEMES = {"balanced": 0, "effective": 1}  # SF_WEIGHTS_BALANCED, SF_WEIGHTS_EFFECTIVE


def class_weights(conf, scheme="balanced", beta=None, out=None):
    """One `sf_class_weights` launch (no host read): conf int64 [K,K] -> fp32 [K] class weights for the weighted losses.
    "balanced": samples / (classes with support * support[c]); "effective": (1 - beta) / (1 - beta^support[c]) rescaled to
    sum to the number of classes with support, `beta` a float in (0, 1).  A class without support gets 0."""
    if scheme not in WEIGHT_SCHEMES:
        raise ValueError("class_weights: scheme must be one of %s, got %r" % (sorted(WEIGHT_SCHEMES), scheme))
    if scheme == "effective":
        if beta is None or not 0.0 < float(beta) < 1.0:
            raise ValueError("class_weights: scheme 'effective' needs beta in (0, 1), got %r" % (beta,))
    elif beta is not None:
        raise ValueError("class_weights: beta belongs to scheme 'effective', got %r with %r" % (beta, scheme))
    if conf.dim() != 2 or conf.shape[0] != conf.shape[1]:
        raise ValueError("class_weights: conf [K, K], got %s" % (tuple(conf.shape),))
    K = conf.shape[0]
    _counters(conf, (K, K), torch.int64, "class_weights: conf")
    if out is None:
        out = torch.empty((K,), dtype=torch.float32, device=conf.device)
    _counters(out, (K,), torch.float32, "class_weights: out")
    b = ctypes.c_double(float(beta)) if beta is not None else None
    _call("sf_class_weights", _ptr(conf), K, WEIGHT_SCHEMES[scheme], ctypes.byref(b) if b is not None else None,
          _ptr(out), tag="class_weights")
    return out


def ava_frame_map(preds, boxes, metadata, gt, flags=False):
    """One `sf_ava_match` and one `sf_ava_ap` call (five launches, no host read): preds fp32 [K,C], boxes fp32 [K,5]
    (batch index, x1, y1, x2, y2), metadata fp32 [K,2] (video index, second) against the device tables `gt` (an object
    with gt_box fp64 [G,4], gt_cls / gt_off int32, lut int32 [V,S], whitelist uint8 [C], num_gt int32 [C]) -> out fp64
    [4 + C] = {mAP, classes counted, refused scores, rows with a video index outside the table, AP per class (-1: left
    out)}; with `flags` also tp uint8 [K,C] and valid uint8 [K]."""
    if preds.dim() != 2 or boxes.dim() != 2 or metadata.dim() != 2 or boxes.shape[1] < 5 or metadata.shape[1] < 2 or \
            not (preds.shape[0] == boxes.shape[0] == metadata.shape[0]):
        raise ValueError("ava_frame_map: preds [K, C], boxes [K, 5] and metadata [K, 2], got %s, %s and %s" % (
            tuple(preds.shape), tuple(boxes.shape), tuple(metadata.shape)))
    K, C = preds.shape
    if gt.whitelist.numel() != C or gt.num_gt.numel() != C:
        raise ValueError("ava_frame_map: the ground-truth tables were built for %d classes, preds has %d" % (
            gt.whitelist.numel(), C))
    preds, ld = _rows(preds, "ava_frame_map")
    boxes, ldb = _rows(boxes, "ava_frame_map")
    metadata, ldm = _rows(metadata, "ava_frame_map")
    G, I = gt.gt_cls.numel(), gt.gt_off.numel() - 1
    V, S = gt.lut.shape
    _counters(gt.gt_box, (G, 4), torch.float64, "ava_frame_map: gt_box")
    _counters(gt.gt_cls, (G,), torch.int32, "ava_frame_map: gt_cls")
    _counters(gt.gt_off, (I + 1,), torch.int32, "ava_frame_map: gt_off")
    _counters(gt.lut, (V, S), torch.int32, "ava_frame_map: lut")
    _counters(gt.whitelist, (C,), torch.uint8, "ava_frame_map: whitelist")
    _counters(gt.num_gt, (C,), torch.int32, "ava_frame_map: num_gt")
    nbytes = lib().sf_ava_ws_bytes(K, C, G)
    if nbytes <= 0:
        raise SfhipError("ava_frame_map: %d rows x %d classes is outside the kernels' range (K * C < 2^31, K <= "
                         "16776960)" % (K, C))
    dev = preds.device
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    tp = torch.empty((K, C), dtype=torch.uint8, device=dev)
    valid = torch.empty((K,), dtype=torch.uint8, device=dev)
    out = torch.empty((4 + C,), dtype=torch.float64, device=dev)
    _call("sf_ava_match", _ptr(boxes), int(ldb), _ptr(metadata), int(ldm), K, C, _ptr(gt.gt_box) if G else None,
          _ptr(gt.gt_cls) if G else None, _ptr(gt.gt_off), G, I, _ptr(gt.lut), V, S, _ptr(gt.whitelist), _ptr(ws),
          _ptr(tp), _ptr(valid), tag="ava_match")
    _call("sf_ava_ap", _ptr(preds), int(ld), _ptr(tp), _ptr(valid), K, C, _ptr(gt.whitelist), _ptr(gt.num_gt), G,
          _ptr(ws), _ptr(out), ctypes.c_void_p(out.data_ptr() + 32), tag="ava_ap")
    return (out, tp, valid) if flags else out


# ------------------------------------------------------------------------------------------------ one-channel stem
def ncthw1_pack(x, ph, pw, wp):
    """[N,1,T,H,W] tensor -> the one-channel stem layout [N, T, H+2ph, Wp, 1] (zero borders)."""
    _require_gpu(x, "ncthw1_pack")
    x = x.contiguous()
    N, C, T, H, W = x.shape
    assert C == 1
    buf = torch.empty((N, T, H + 2 * ph, wp, 1), dtype=torch.float32, device=x.device)
    _call("sf_ncthw1_pack", _ptr(x), _ptr(buf), N, T, H, W, ph, pw, wp)
    return buf


def stem1_accepts(Hp, Wp, cout, kernel, stride, dilation=(1, 1, 1), groups=1):
    """Is nn.Conv3d(1, cout, kernel, stride) over rows of Wp floats in the range of sf_stem1_fwd / sf_stem1_wgrad?"""
    return (tuple(kernel[1:]) == (7, 7) and tuple(stride) == (1, 2, 2) and tuple(dilation) == (1, 1, 1) and
            groups == 1 and bool(lib().sf_stem1_accepts(int(Hp), int(Wp), int(cout), int(kernel[0]))))


def stem1_out_thw(buf, kT, pT):
    return buf.shape[1] + 2 * pT - kT + 1, (buf.shape[2] - 7) // 2 + 1, (buf.shape[3] - 7) // 2 + 1


def stem1_fwd(buf, w, pT, scale=None, bias=None, relu=False, out=None, out_reserve=(0, 0)):
    """Stem conv of a one-channel clip in the packed layout `buf` [N,T,Hp,Wp,1]; w: the nn.Conv3d weight
    [Cout,1,kT,7,7] (stride (1,2,2), H/W padding in the layout).  -> Act [N,To,Ho,Wo,Cout]."""
    _require_gpu(buf, "stem1_fwd")
    _require_gpu(w, "stem1_fwd")
    assert buf.dim() == 5 and buf.shape[4] == 1 and buf.is_contiguous()
    assert w.dim() == 5 and w.shape[1] == 1 and tuple(w.shape[3:]) == (7, 7) and w.is_contiguous()
    cout, kT = w.shape[0], w.shape[2]
    N, T, Hp, Wp = buf.shape[:4]
    To, Ho, Wo = stem1_out_thw(buf, kT, pT)
    if out is None:
        out = new_act(buf.device, N, To, Ho, Wo, cout, out_reserve[0], out_reserve[1])
    assert (out.N, out.T, out.H, out.W, out.C) == (N, To, Ho, Wo, cout), (out, (N, To, Ho, Wo, cout))
    for v in (scale, bias):
        assert v is None or (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == cout)
    _call("sf_stem1_fwd", _ptr(buf), N, T, Hp, Wp, _ptr(w), cout, kT, int(pT), _ptr(scale), _ptr(bias), _act(relu),
          out.ptr(), out.cs, out.coff, tag="stem1_fwd")
    return out


def stem1_wgrad(buf, dz, kT, pT, into=None):
    """dL/d(weight) [Cout,1,kT,7,7] of stem1_fwd from dz (Act shaped like its output); `into`: accumulate into this
    contiguous gradient tensor instead of returning a new one.  Fixed summation order: bitwise reproducible."""
    _require_gpu(buf, "stem1_wgrad")
    assert buf.dim() == 5 and buf.shape[4] == 1 and buf.is_contiguous()
    N, T, Hp, Wp = buf.shape[:4]
    cout = dz.C
    assert (dz.N, dz.T, dz.H, dz.W) == (N,) + stem1_out_thw(buf, kT, pT), (dz, tuple(buf.shape))
    n_ws = lib().sf_stem1_wgrad_ws_floats(N, T, Hp, Wp, cout, int(kT), int(pT))
    if n_ws <= 0:
        raise SfhipError("stem1_wgrad: shape outside the one-channel stem kernels' range (sfhip.stem1_accepts)")
    ws = torch.empty(n_ws, dtype=torch.float32, device=buf.device)
    if into is not None:
        assert into.is_cuda and into.dtype == torch.float32 and into.is_contiguous() and \
            into.numel() == cout * kT * 49
    dw = into if into is not None else torch.empty((cout, 1, kT, 7, 7), dtype=torch.float32, device=buf.device)
    _call("sf_stem1_wgrad", _ptr(buf), N, T, Hp, Wp, dz.ptr(), dz.cs, dz.coff, cout, int(kT), int(pT), _ptr(dw),
          1 if into is not None else 0, _ptr(ws), tag="stem1_wgrad")
    return dw


def to_ncthw(a):
    out = torch.empty(a.shape_ncthw, dtype=torch.float32, device=a.buf.device)
    _call("sf_ndhwc_to_ncthw", a.ptr(), a.cs, a.coff, _ptr(out), a.N, a.C, a.T, a.H, a.W)
    return out


# ------------------------------------------------------------------------------------------------ conv
def _out_dim(i, k, s, p, d):
    return (i + 2 * p - d * (k - 1) - 1) // s + 1


def _out_thw(x, kernel, stride, padding, dilation=(1, 1, 1)):
    """(To, Ho, Wo) of a conv / pool window over the view x."""
    return tuple(_out_dim(i, k, s, p, d) for i, k, s, p, d in zip((x.T, x.H, x.W), kernel, stride, padding, dilation))


def _pad16(c):
    """Channel count rounded up to the packed weights' multiple of 16."""
    return (c + 15) // 16 * 16


def _conv_desc(x, out_thw, out_cs, out_coff, cout, kernel, stride, padding, dilation=(1, 1, 1), *, cin_pad, cin=None,
               act=ACT_NONE, res=None, out_cmul=1, transposed=0, scatter=()):
    """sf_conv_desc, filled in the header's field order — the one place that is done.  x: the input view (dL/dz for a
    data gradient); out_thw / out_cs / out_coff / cout: the output (pitch and offset 0 for the weight gradients, which
    have none); cin: channels read per tap (default x.C); res: the residual view, whose pitch / offset the descriptor
    carries (None: 0, 0); scatter: (os_T, os_H, os_W, oo_T, oo_H, oo_W, ob_T, ob_H, ob_W) of one residue class of a
    strided data gradient (empty: a dense store)."""
    kT, kH, kW = kernel
    return ConvDesc(x.N, x.T, x.H, x.W, x.C if cin is None else cin, x.cs, x.coff, out_thw[0], out_thw[1], out_thw[2],
                    cout, out_cs, out_coff, out_cmul, kT, kH, kW, stride[0], stride[1], stride[2],
                    padding[0], padding[1], padding[2], dilation[0], dilation[1], dilation[2], cin_pad, act,
                    res.cs if res is not None else 0, res.coff if res is not None else 0, transposed, *scatter)


def pack_conv_weight(w, cin_pad=None):
    """[Cout, Cin, kT, kH, kW] -> [Cout, kT*kH*kW, cin_pad] (zero padded), contiguous."""
    cout, cin = w.shape[0], w.shape[1]
    taps = w.shape[2] * w.shape[3] * w.shape[4]
    cin_pad = _pad16(cin) if cin_pad is None else cin_pad
    wp = torch.zeros((cout, taps, cin_pad), dtype=torch.float32, device=w.device)
    wp[:, :, :cin] = w.detach().reshape(cout, cin, taps).permute(0, 2, 1)
    return wp.contiguous()


def bx_planes(t, rows, C, cs=None, coff=0):
    """The bf16 piece planes [3][rows + 1][C] (uint16 tensor) of a [rows][cs] fp32 operand: sf_bx_split."""
    planes = torch.empty((lib().sf_bx_planes_elems(rows, C),), dtype=torch.int16, device=t.device)
    _call("sf_bx_split", _ptr(t), C if cs is None else cs, coff, rows, C, _ptr(planes))
    return planes


def _weight_planes(wp):
    """Planes of a packed conv weight [Cout][taps][cin_pad], cached ON the tensor object (pack_conv_weight_pairs
    refreshes them when it overwrites the packed weight in place)."""
    pl = wp.__dict__.get("_sf_bx")
    # torch's version counter of the packed tensor: the library's own in-place re-pack (a raw kernel launch) does not
    # move it and refreshes the planes itself; any OTHER in-place write (wp.copy_(...)) does, and the planes are re-made
    if pl is None or wp.__dict__.get("_sf_bx_ver") != wp._version:
        if pl is None:
            pl = bx_planes(wp, wp.shape[0], wp.shape[1] * wp.shape[2])
        else:  # same storage: pack_conv_weight_pairs' device-side tables keep pointing at it
            _call("sf_bx_split", _ptr(wp), wp.shape[1] * wp.shape[2], 0, wp.shape[0], wp.shape[1] * wp.shape[2],
                  _ptr(pl))
        wp.__dict__["_sf_bx"] = pl
        wp.__dict__["_sf_bx_ver"] = wp._version
    return pl


def act_planes(a):
    """bf16 piece planes of an activation view (all rows, its C channels): what conv_bx.hip's kernels read."""
    return bx_planes(a.buf, a.rows, a.C, cs=a.cs, coff=a.coff)


def _conv_launch(d, x_ptr, w_ptr, scale, bias, res_ptr, out_ptr, device, what, w_tensor=None, in_planes=None):
    """sf_conv_fwd, through the split-K schedule when the shape asks for it (workspace from the caching allocator).
    Trace tag: ("conv", output positions, taps * Cin, Cout) — 2 * product = the launch's algorithmic FLOPs.
    w_tensor: the packed weight as a tensor — lets the bf16-piece path (conv_bx.hip) keep its planes across calls.
    in_planes: act_planes of the input view when the caller already has them."""
    tag = ("conv", d.N * d.To * d.Ho * d.Wo, d.kT * d.kH * d.kW * d.Cin, d.Cout)
    if SPLIT_K and w_tensor is not None and w_tensor.shape[2] == d.Cin:
        n = lib().sf_conv_pw_ws_floats(ctypes.byref(d), 1)
        if n > 0:  # pointwise layers: activations split in registers, only the weight's planes are kept
            planes = _weight_planes(w_tensor)
            ws = torch.empty((n,), dtype=torch.float32, device=device)
            # _REFUSED: declined before any launch -> the f32 kernels below (SF_EINVAL — a genuinely inconsistent
            # descriptor or a null pointer — raises)
            if _call("sf_conv_fwd_pw", ctypes.byref(d), x_ptr, w_ptr, _ptr(planes), scale, bias, res_ptr, out_ptr,
                     _ptr(ws), None, None, tag=tag, what=what, allow=_REFUSED) == 0:
                return
        n = lib().sf_conv_bx_ws_floats(ctypes.byref(d), 1 if in_planes is not None else 0, 1)
        if n > 0:
            planes = _weight_planes(w_tensor)
            ws = torch.empty((n,), dtype=torch.float32, device=device)
            if _call("sf_conv_fwd_bx", ctypes.byref(d), x_ptr, _ptr(in_planes), w_ptr, _ptr(planes), scale, bias,
                     res_ptr, out_ptr, _ptr(ws), tag=tag, what=what, allow=_REFUSED) == 0:
                return
    n = lib().sf_conv_fwd_ws_floats(ctypes.byref(d)) if SPLIT_K else 0
    if n > 0:
        ws = torch.empty((n,), dtype=torch.float32, device=device)
        _call("sf_conv_fwd_ws", ctypes.byref(d), x_ptr, w_ptr, scale, bias, res_ptr, out_ptr, _ptr(ws), tag=tag,
              what=what)
    else:
        _call("sf_conv_fwd", ctypes.byref(d), x_ptr, w_ptr, scale, bias, res_ptr, out_ptr, tag=tag, what=what)


SPLIT_K = True  # False: one-pass f32 kernels only (tests compare the two schedules)


def pack_conv_weight_pair(w):
    """(wp [Cout][taps][cin_pad], wtp [Cin][taps][cout_pad]) of an nn.Conv3d weight on the GPU in one launch."""
    _require_gpu(w, "pack_conv_weight_pair")
    w = w.detach().contiguous()
    cout, cin = w.shape[0], w.shape[1]
    taps = w.shape[2] * w.shape[3] * w.shape[4]
    cin_pad, cout_pad = _pad16(cin), _pad16(cout)
    wp = torch.empty((cout, taps, cin_pad), dtype=torch.float32, device=w.device)
    wtp = torch.empty((cin, taps, cout_pad), dtype=torch.float32, device=w.device)
    _call("sf_pack_conv_weight", _ptr(w), cout, cin, taps, _ptr(wp), cin_pad, _ptr(wtp), cout_pad)
    return wp, wtp


def pack_grouped_weight_pair(w, groups):
    """Packed weights of nn.Conv3d(groups = G) for sf_conv_fwd_grouped: (wp [Cout][taps][pad(Cin / G)], wtp
    [Cin][taps][pad(Cout / G)]) = the G per-group (forward, transposed) packs one after the other, written in place
    into two tensors (one sf_pack_conv_weight launch per group, once per parameter version)."""
    _require_gpu(w, "pack_grouped_weight_pair")
    w = w.detach().contiguous()
    cout, cin_g = w.shape[0], w.shape[1]
    assert cout % groups == 0, (w.shape, groups)
    cout_g = cout // groups
    taps = w.shape[2] * w.shape[3] * w.shape[4]
    cin_pad, cout_pad = _pad16(cin_g), _pad16(cout_g)
    wp = torch.empty((cout, taps, cin_pad), dtype=torch.float32, device=w.device)
    wtp = torch.empty((cin_g * groups, taps, cout_pad), dtype=torch.float32, device=w.device)
    for g in range(groups):
        _call("sf_pack_conv_weight", _ptr(w[g * cout_g:(g + 1) * cout_g]), cout_g, cin_g, taps,
              _ptr(wp[g * cout_g:(g + 1) * cout_g]), cin_pad, _ptr(wtp[g * cin_g:(g + 1) * cin_g]), cout_pad)
    return wp, wtp


_PACK_TABLES = {}


_SPLIT_TABLES = {}


def pack_conv_weight_pairs(weights, outs):
    """pack_conv_weight_pair for many weights in ONE launch.  outs: per weight the (wp, wtp) tensors to fill (None =
    allocate).  Returns the list of (wp, wtp).  The device-side table of pointers is cached per pointer set."""
    import struct
    import numpy as np
    res, recs, blk0, nb = [], [], [0], 0
    for w, o in zip(weights, outs):
        _require_gpu(w, "pack_conv_weight_pairs")
        assert w.is_contiguous() and w.dtype == torch.float32
        cout, cin = w.shape[0], w.shape[1]
        taps = w.shape[2] * w.shape[3] * w.shape[4]
        cin_pad, cout_pad = _pad16(cin), _pad16(cout)
        ok = (o is not None and o[0] is not None and o[1] is not None and
              all(t.device == w.device and t.dtype == torch.float32 and t.is_contiguous() for t in o) and
              tuple(o[0].shape) == (cout, taps, cin_pad) and tuple(o[1].shape) == (cin, taps, cout_pad))
        if not ok:  # e.g. the (wp, None) a CPU forward cached, or a pair left on another GPU by .to(device)
            o = (torch.empty((cout, taps, cin_pad), dtype=torch.float32, device=w.device),
                 torch.empty((cin, taps, cout_pad), dtype=torch.float32, device=w.device))
        res.append(o)
        n_wp = cout * taps * cin_pad
        total = n_wp + cin * taps * cout_pad
        recs.append((w.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), cout, cin, taps, cin_pad, cout_pad, 0, n_wp, total))
        # workgroups of this weight (sfhip.h): the forward layout element-wise, the transposed one in 32 x 32 tiles
        nbw = ((cout + 7) // 8) * ((cin_pad + 31) // 32) if 1 < taps <= 9 else (n_wp + 255) // 256
        nb += nbw + ((cin * taps + 31) // 32) * ((cout_pad + 31) // 32)
        blk0.append(nb)
    key = tuple(r[:8] for r in recs)  # pointers AND dims: a freed buffer's address may come back with another shape
    dev = weights[0].device
    tab = _PACK_TABLES.get(dev)
    if (tab is None or tab[0] != key) and torch.cuda.is_current_stream_capturing():
        # a new pointer set while a hipGraph is being captured (e.g. the first training step after an eval pass re-packed
        # the weights one by one): the device-side table would need a host-to-device copy, which a capture refuses —
        # one launch per weight (and per plane set) instead, all of them capturable
        for w, o in zip(weights, res):
            cout, cin = w.shape[0], w.shape[1]
            taps = w.shape[2] * w.shape[3] * w.shape[4]
            _call("sf_pack_conv_weight", _ptr(w), cout, cin, taps, _ptr(o[0]), o[0].shape[2], _ptr(o[1]),
                  o[1].shape[2])
            for t in o:
                pl = t.__dict__.get("_sf_bx")
                if pl is not None:
                    c = t.shape[1] * t.shape[2]
                    _call("sf_bx_split", _ptr(t), c, 0, t.shape[0], c, _ptr(pl))
                t.__dict__.pop("_sf_classes", None)
        return res
    if tab is None or tab[0] != key:
        raw = b"".join(struct.pack("<QQQiiiiiiqq", *r) for r in recs)
        items = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev)
        starts = torch.tensor(blk0, dtype=torch.int32).to(dev)
        tab = (key, items, starts)
        _PACK_TABLES[dev] = tab
    _call("sf_pack_conv_weights", _ptr(tab[1]), _ptr(tab[2]), len(recs), nb)
    # packed weights overwritten in place: their bf16 piece planes (conv_bx.hip) follow, all in ONE launch
    recs, blk0, nb = [], [0], 0
    for o in res:
        for t in o:
            pl = t.__dict__.get("_sf_bx")
            if pl is not None:
                rows, c = t.shape[0], t.shape[1] * t.shape[2]
                recs.append((t.data_ptr(), pl.data_ptr(), rows, c, 0))
                nb += ((rows + 1) * (c // 8) + 255) // 256
                blk0.append(nb)
            t.__dict__.pop("_sf_classes", None)  # tap-subset copies of the previous contents (strided data gradients)
    if len(recs) == 1:
        r = recs[0]
        _call("sf_bx_split", r[0], r[3], 0, r[2], r[3], r[1])
    elif recs:
        key = tuple(recs)
        tab = _SPLIT_TABLES.get(dev)
        if tab is None or tab[0] != key:
            raw = b"".join(struct.pack("<QQqii", *r) for r in recs)
            tab = (key, torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev),
                   torch.tensor(blk0, dtype=torch.int32).to(dev))
            _SPLIT_TABLES[dev] = tab
        _call("sf_bx_split_batched", _ptr(tab[1]), _ptr(tab[2]), len(recs), nb)
    return res


def pack_dw_weight(w):
    """depthwise [C, 1, kT, kH, kW] -> [taps, C]."""
    c = w.shape[0]
    return w.detach().reshape(c, -1).t().contiguous()


def conv(x, wp, kernel, stride=(1, 1, 1), padding=(0, 0, 0), dilation=(1, 1, 1), scale=None, bias=None,
         relu=False, res=None, out=None, cin=None, out_cmul=1, out_reserve=(0, 0), out_thw=None, stats=False):
    """Dense conv (implicit GEMM, sf_conv_fwd).  `wp` = pack_conv_weight(...).  `out`: Act to write into
    (a slice of a wider buffer) or None to allocate [.., before + Cout + after].
    stats=True returns (out, parts) with parts = (workspace, rows) of per-tile channel statistics of the output taken
    in the conv's epilogue (sf_conv_fwd_stats) for bn_train_stats_merge, or None when this shape produces none."""
    _require_gpu(x.buf, "conv")
    cout, taps, cin_pad = wp.shape
    cin = x.C if cin is None else cin
    To, Ho, Wo = _out_thw(x, kernel, stride, padding, dilation)
    if out_thw is not None:  # caller restricts the output extent (stem trick: trailing columns are padding)
        assert out_thw[0] <= To and out_thw[1] <= Ho and out_thw[2] <= Wo
        To, Ho, Wo = out_thw
    if out is None:
        out = new_act(x, x.N, To, Ho, Wo, cout, out_reserve[0], out_reserve[1])
    else:
        assert (out.N, out.T, out.H, out.W) == (x.N, To, Ho, Wo), (out, (x.N, To, Ho, Wo))
        assert out.coff + (cout - 1) * out_cmul < out.cs and (out_cmul > 1 or out.C == cout), (out, cout)
    d = _conv_desc(x, (To, Ho, Wo), out.cs, out.coff, cout, kernel, stride, padding, dilation, cin=cin,
                   cin_pad=cin_pad, act=_act(relu), res=res, out_cmul=out_cmul)
    if res is not None:
        assert res.rows == out.rows and res.C == cout
    if stats and SPLIT_K and scale is None and res is None and not relu and out_cmul == 1 and \
            wp.shape[2] == cin:
        n = lib().sf_conv_pw_stats_floats(ctypes.byref(d))
        if n > 0:  # pointwise layer on the bf16 pipe, statistics from its epilogue
            planes = _weight_planes(wp)
            ws = torch.empty((lib().sf_conv_pw_ws_floats(ctypes.byref(d), 1),), dtype=torch.float32, device=x.buf.device)
            st = torch.empty((n,), dtype=torch.float32, device=x.buf.device)
            parts = ctypes.c_int(0)
            _call("sf_conv_fwd_pw", ctypes.byref(d), x.ptr(), _ptr(wp), _ptr(planes), None, _ptr(bias), None,
                  out.ptr(), _ptr(ws), _ptr(st), ctypes.byref(parts),
                  tag=("conv", d.N * d.To * d.Ho * d.Wo, d.Cin, d.Cout))
            return out, ((st, parts.value) if parts.value > 0 else None)
    if stats:
        n = lib().sf_conv_stats_ws_floats(ctypes.byref(d)) if (scale is None and res is None and not relu
                                                              and out_cmul == 1) else 0
        if n > 0:
            ws = torch.empty((n,), dtype=torch.float32, device=x.buf.device)
            parts = ctypes.c_int(0)
            _call("sf_conv_fwd_stats", ctypes.byref(d), x.ptr(), _ptr(wp), None, _ptr(bias), None, out.ptr(),
                  _ptr(ws), ctypes.byref(parts),
                  tag=("conv", d.N * d.To * d.Ho * d.Wo, d.kT * d.kH * d.kW * d.Cin, d.Cout))
            return out, ((ws, parts.value) if parts.value > 0 else None)
    _conv_launch(d, x.ptr(), _ptr(wp), _ptr(scale), _ptr(bias), res.ptr() if res is not None else None, out.ptr(),
                 x.buf.device, "sf_conv_fwd", w_tensor=wp)
    return (out, None) if stats else out


def dwconv(x, wp, kernel, stride=(1, 1, 1), padding=(0, 0, 0), scale=None, bias=None, relu=False, res=None,
           out=None, cout=None, out_cmul=1):
    """Depthwise conv (sf_dwconv_fwd); wp = pack_dw_weight(...) [taps, C], or [taps, pitch >= C] (the transposed
    half of pack_conv_weight_pair of the [C, 1, kT, kH, kW] parameter)."""
    _require_gpu(x.buf, "dwconv")
    taps, wpitch = wp.shape
    c = x.C
    assert wpitch >= c, (wp.shape, x)
    cout = c if cout is None else cout
    To, Ho, Wo = _out_thw(x, kernel, stride, padding)
    if out is None:
        out = new_act(x, x.N, To, Ho, Wo, cout)
    else:
        assert (out.N, out.T, out.H, out.W) == (x.N, To, Ho, Wo)
    d = _conv_desc(x, (To, Ho, Wo), out.cs, out.coff, cout, kernel, stride, padding, cin_pad=wpitch, act=_act(relu),
                   res=res, out_cmul=out_cmul)
    # trace tag: ("dwconv", algorithmic HBM bytes = input + output (+ residual) rows once)
    nbytes = 4 * (x.rows * c + out.rows * cout * (2 if res is not None else 1))
    _call("sf_dwconv_fwd", ctypes.byref(d), x.ptr(), _ptr(wp), _ptr(scale), _ptr(bias),
          res.ptr() if res is not None else None, out.ptr(), tag=("dwconv", nbytes, taps, c))
    return out


def _pool_desc(x, out_thw, out_cs, out_coff, kernel, stride, padding, avg):
    """sf_pool_desc in the header's field order; x: the input view."""
    return PoolDesc(x.N, x.T, x.H, x.W, x.C, x.cs, x.coff, out_thw[0], out_thw[1], out_thw[2], out_cs, out_coff,
                    kernel[0], kernel[1], kernel[2], stride[0], stride[1], stride[2],
                    padding[0], padding[1], padding[2], 1 if avg else 0)


def pool(x, kernel, stride, padding=(0, 0, 0), avg=False, out=None, out_reserve=(0, 0), want_arg=False):
    """want_arg (max pooling): also return the byte map of window winners for maxpool_bwd_arg — (out, arg), arg None
    when the views are not float4-addressable or the window has more than 255 taps."""
    _require_gpu(x.buf, "pool")
    To, Ho, Wo = _out_thw(x, kernel, stride, padding)
    if out is None:
        out = new_act(x, x.N, To, Ho, Wo, x.C, out_reserve[0], out_reserve[1])
    else:
        assert (out.N, out.T, out.H, out.W, out.C) == (x.N, To, Ho, Wo, x.C)
    d = _pool_desc(x, (To, Ho, Wo), out.cs, out.coff, kernel, stride, padding, avg)
    if want_arg and not avg:
        ok = (x.C % 4 == 0 and x.cs % 4 == 0 and x.coff % 4 == 0 and out.cs % 4 == 0 and out.coff % 4 == 0 and
              kernel[0] * kernel[1] * kernel[2] <= 255 and x.buf.data_ptr() % 16 == 0 and out.buf.data_ptr() % 16 == 0)
        if ok:
            arg = torch.empty((out.rows, x.C), dtype=torch.uint8, device=x.buf.device)
            _call("sf_maxpool_fwd_arg", ctypes.byref(d), x.ptr(), out.ptr(), _ptr(arg))
            return out, arg
    _call("sf_pool_fwd", ctypes.byref(d), x.ptr(), out.ptr())
    return (out, None) if want_arg else out


def tmax_mean(x, alpha):
    """pooled[b,c] = mean_{t',h,w} max_{r<alpha} x[b,t'*alpha+r,h,w,c]  ->  torch [N, C]."""
    _require_gpu(x.buf, "tmax_mean")
    pooled = torch.empty((x.N, x.C), dtype=torch.float32, device=x.buf.device)
    ws = torch.empty((lib().sf_tmax_mean_ws_floats(x.N, x.C),), dtype=torch.float32, device=x.buf.device)
    _call("sf_tmax_mean", x.ptr(), x.cs, x.coff, x.N, x.T, x.H, x.W, x.C, alpha, _ptr(pooled), _ptr(ws))
    return pooled


def gate_apply(x, alpha, pooled, w3=None, scale=None, bias=None, relu=False, out=None):
    _require_gpu(x.buf, "gate_apply")
    if out is None:
        out = new_act(x, x.N, x.T // alpha, x.H, x.W, x.C)
    else:
        assert (out.N, out.T, out.H, out.W, out.C) == (x.N, x.T // alpha, x.H, x.W, x.C), (out, x)
    _call("sf_gate_apply", x.ptr(), x.cs, x.coff, x.N, x.T, x.H, x.W, x.C, alpha, _ptr(pooled), _ptr(w3),
          _ptr(scale), _ptr(bias), ACT_RELU if relu else ACT_NONE, out.ptr(), out.cs, out.coff)
    return out


def attention(q, k, v, x, gamma, scale=None, bias=None, relu=False, alpha=1, out=None, save=None):
    """Flash SpatialAttention + gamma-residual + (BN affine, ReLU) + nearest T-upsample x alpha.
    save: optional dict that receives 'o' ([B,N,C] tensor, O = P v) and 'lse' ([B,N]) for the backward pass."""
    _require_gpu(x.buf, "attention")
    if out is None:
        out = new_act(x, x.N, x.T * alpha, x.H, x.W, x.C)
    else:
        assert (out.N, out.T, out.H, out.W, out.C) == (x.N, x.T * alpha, x.H, x.W, x.C), (out, x)
    o_save = lse_save = None
    if save is not None:
        n = x.T * x.H * x.W
        o_save = save["o"] = torch.empty((x.N, n, x.C), dtype=torch.float32, device=x.buf.device)
        lse_save = save["lse"] = torch.empty((x.N, n), dtype=torch.float32, device=x.buf.device)
    # workspace for the key-range parts the launcher may cut the sweep into (sf_sweep_parts: fills the last round)
    ws = torch.empty((lib().sf_attn_fwd_ws_floats(x.N, x.T * x.H * x.W, x.C),), dtype=torch.float32,
                     device=x.buf.device)
    _call("sf_attn_fwd_ws", _slice_base(q), q.cs, _slice_base(k), k.cs, _slice_base(v), v.cs, _slice_base(x), x.cs,
          _ptr(gamma), _ptr(scale), _ptr(bias), ACT_RELU if relu else ACT_NONE, out.ptr(), out.cs, out.coff,
          x.N, x.T, x.H, x.W, x.C, alpha, _ptr(o_save), _ptr(lse_save), _ptr(ws),
          tag=("attn", x.N, x.T * x.H * x.W, x.C))
    return out


def head_act_mean(logits, act):
    """logits Act [N,T,H,W,K] (dense) -> torch [N, K] = mean_{t,h,w} act(logits)."""
    assert logits.coff == 0 and logits.C == logits.cs
    out = torch.empty((logits.N, logits.C), dtype=torch.float32, device=logits.buf.device)
    _call("sf_head_act_mean", logits.ptr(), logits.N, logits.T * logits.H * logits.W, logits.C, act, _ptr(out))
    return out


def copy_channels(x, out, out_cmul=1):
    assert x.rows == out.rows
    _call("sf_copy_channels", x.ptr(), x.cs, x.coff, out.ptr(), out.cs, out.coff, out_cmul, x.rows, x.C)
    return out


def channel_shuffle(x, out, groups, accumulate=False):
    """out[.., j*G + g] (+)= x[.., g*(C/G) + j] in one launch (sf_channel_shuffle); groups = C/G inverts it."""
    assert x.rows == out.rows and x.C == out.C and x.C % groups == 0
    _call("sf_channel_shuffle", x.ptr(), x.cs, x.coff, out.ptr(), out.cs, out.coff, groups, x.rows, x.C,
          1 if accumulate else 0)
    return out


def channel_stats(x):
    """Per-channel (mean, biased variance) over all N*T*H*W rows of the view -> two torch [C] tensors."""
    _require_gpu(x.buf, "channel_stats")
    dev = x.buf.device
    mean = torch.empty((x.C,), dtype=torch.float32, device=dev)
    var = torch.empty((x.C,), dtype=torch.float32, device=dev)
    ws = torch.empty((lib().sf_channel_stats_ws_floats(x.C),), dtype=torch.float32, device=dev)
    _call("sf_channel_stats", x.ptr(), x.cs, x.coff, x.rows, x.C, _ptr(mean), _ptr(var), _ptr(ws))
    return mean, var


def affine(x, scale=None, bias=None, res=None, relu=False, rep=1, out=None, out_reserve=(0, 0), out_cmul=1,
           nsplit=1, mask=None):
    """out = act(x*scale + bias + res), repeated `rep` times along T (nearest upsample).  nsplit > 1: scale/bias
    hold nsplit*C entries and sample n uses block n % nsplit (SubBatchNorm3d).
    mask: optional dict (training, ReLU / ReLU6 layers): when the layer qualifies for the flat float4 kernel it
    receives 'bytes', a uint8 tensor [rows * C/4] with one pass-through bit per channel, which bn_bwd(mask=...)
    reads instead of the activation."""
    _require_gpu(x.buf, "affine")
    if out is None:
        out = new_act(x, x.N, x.T * rep, x.H, x.W, x.C, out_reserve[0], out_reserve[1])
    else:
        assert (out.N, out.T, out.H, out.W) == (x.N, x.T * rep, x.H, x.W), (out, x, rep)
        assert out.coff + (x.C - 1) * out_cmul < out.cs and (out_cmul > 1 or out.C == x.C), (out, x)
    if res is not None:
        assert res.rows == x.rows and res.C == x.C
    head = (x.ptr(), x.cs, x.coff, x.N, x.T, x.H, x.W, x.C)
    mid = (_ptr(scale), _ptr(bias), res.ptr() if res is not None else None, res.cs if res is not None else 0,
           res.coff if res is not None else 0, _act(relu))
    if (mask is not None and relu and rep == 1 and nsplit == 1 and out_cmul == 1 and x.C % 4 == 0 and
            x.cs % 4 == 0 and x.coff % 4 == 0 and out.cs % 4 == 0 and out.coff % 4 == 0 and
            x.rows * (x.C // 4) < 2 ** 31 - 1 and scale is not None and
            (res is None or (res.cs % 4 == 0 and res.coff % 4 == 0))):
        mk = torch.empty((x.rows * (x.C // 4),), dtype=torch.uint8, device=x.buf.device)
        _call("sf_affine_fwd_mask", *head, *mid, out.ptr(), out.cs, out.coff, _ptr(mk))
        mask["bytes"] = mk
        return out
    tail = mid + (rep, out.ptr(), out.cs, out.coff, out_cmul)
    if nsplit == 1:
        _call("sf_affine_fwd", *head, *tail)
    else:
        _call("sf_affine_fwd_split", *head, nsplit, *tail)
    return out


def conv_dgrad(dz, wt_packed, x_like, kernel, stride=(1, 1, 1), padding=(0, 0, 0), dilation=(1, 1, 1),
               out=None, accumulate=False, dz_planes=None):
    """Data gradient of a dense conv: dL/dx[N,Ti,Hi,Wi,Cin] (+)= conv^T(dL/dz, W).  `wt_packed` =
    pack_conv_weight(W.transpose(0, 1)) i.e. [Cin][tap][Cout_pad]; `x_like` gives the forward input's dims."""
    _require_gpu(dz.buf, "conv_dgrad")
    cin, taps, cout_pad = wt_packed.shape
    if out is None:
        out = new_act(dz, x_like.N, x_like.T, x_like.H, x_like.W, cin)
        accumulate = False
    assert (out.N, out.T, out.H, out.W, out.C) == (x_like.N, x_like.T, x_like.H, x_like.W, cin), (out, x_like)
    if max(stride) > 1 and tuple(dilation) == (1, 1, 1) and (accumulate or (out.coff == 0 and out.cs == out.C)):
        return _conv_dgrad_strided(dz, wt_packed, out, kernel, stride, padding, accumulate, dz_planes)
    # the residual is the output itself, and only when accumulating
    d = _conv_desc(dz, (out.T, out.H, out.W), out.cs, out.coff, cin, kernel, stride, padding, dilation,
                   cin_pad=cout_pad, res=out if accumulate else None, transposed=1)
    _conv_launch(d, dz.ptr(), _ptr(wt_packed), None, None, out.ptr() if accumulate else None, out.ptr(),
                 dz.buf.device, "sf_conv_fwd(transposed)", w_tensor=wt_packed, in_planes=dz_planes)
    return out



def _residue_taps(k, s, p, a):
    """Taps kk of a stride-s, pad-p, size-k kernel that reach input positions = a (mod s), as (offsets, taps):
    input position s*i + a receives dz[i + off] through tap kk, off = (a + p - kk) / s; returned in ascending
    off order so that they form a dense stride-1 kernel over dz."""
    pairs = sorted(((a + p - kk) // s, kk) for kk in range(k) if (a + p - kk) % s == 0)
    return [o for o, _ in pairs], [kk for _, kk in pairs]


_TAP_INDEX = {}


def _class_weights(wt_packed, store, kernel, stride, padding):
    """The tap-subset copies of a packed data-gradient weight [Cin][taps][cout_pad] for EVERY residue class of a strided
    layer, by ONE gather launch per weight and optimizer step: the rows (ci, tap) of all classes are gathered class by
    class into one tensor, and a class's weight [Cin][its taps][cout_pad] is a contiguous slice of it (a gather per
    class was 30 small launches per step of cfg #3, each in front of its class's conv; a torch.stack of tap slices ~190
    copy kernels).  The row index is built once per (Cin, layer geometry, device) — during warm-up, so nothing is copied
    from the host inside a hipGraph capture.  Fills `store` (key = (a_t, a_h, a_w, kernel, stride, padding))."""
    cin, taps, cout_pad = wt_packed.shape
    kT, kH, kW = kernel
    fam = (tuple(kernel), tuple(stride), tuple(padding))
    classes = []
    for at in range(stride[0]):
        tt = _residue_taps(kT, stride[0], padding[0], at)[1]
        for ah in range(stride[1]):
            th = _residue_taps(kH, stride[1], padding[1], ah)[1]
            for aw in range(stride[2]):
                tw = _residue_taps(kW, stride[2], padding[2], aw)[1]
                if tt and th and tw:
                    classes.append(((at, ah, aw) + fam, [(a * kH + b) * kW + c for a in tt for b in th for c in tw]))
    ikey = (cin, taps, fam, str(wt_packed.device))
    idx = _TAP_INDEX.get(ikey)
    if idx is None:
        rows = [ci * taps + t for _, sel in classes for ci in range(cin) for t in sel]
        idx = _TAP_INDEX[ikey] = torch.tensor(rows, dtype=torch.long, device=wt_packed.device)
    allrows = wt_packed.view(cin * taps, cout_pad).index_select(0, idx)
    off = 0
    for key, sel in classes:
        n = cin * len(sel)
        store[key] = allrows[off:off + n].view(cin, len(sel), cout_pad)
        off += n
    return store


def _conv_dgrad_strided(dz, wt_packed, out, kernel, stride, padding, accumulate, dz_planes=None):
    """Data gradient of a strided conv as one DENSE small conv over dL/dz per residue class of the input position
    (the transposed-gather formulation evaluates every tap at every input position and predicates s^2-1 of s^2
    of them away).  Class (a_t, a_h, a_w): dx[s*i + a] = sum_j dz[i - pad' + j] * W[tap_j]; stores are scattered
    to the class's positions by the conv kernel's epilogue."""
    cin, _, cout_pad = wt_packed.shape
    kT, kH, kW = kernel
    # without accumulation every class WRITES its own positions; only when some class gets no tap at all (1x1x1
    # stride-2 shortcuts: 3 of 4) does the buffer need zeros underneath
    every = all(_residue_taps(k, s, p, a)[1] and (full - a + s - 1) // s > 0
                for k, s, p, full in zip(kernel, stride, padding, (out.T, out.H, out.W)) for a in range(s))
    add = accumulate or not every
    if not accumulate and not every:
        out.buf.zero_()
    for at in range(stride[0]):
        ot, tt = _residue_taps(kT, stride[0], padding[0], at)
        for ah in range(stride[1]):
            oh, th = _residue_taps(kH, stride[1], padding[1], ah)
            for aw in range(stride[2]):
                ow, tw = _residue_taps(kW, stride[2], padding[2], aw)
                dims = [(full - a + s - 1) // s for full, a, s in zip((out.T, out.H, out.W), (at, ah, aw), stride)]
                if not (tt and th and tw) or min(dims) <= 0:
                    continue  # no tap reaches this class: its gradient is zero
                # tap-subset weights, cached ON the packed tensor (they must die with it: the next optimizer step's
                # packed copy may land at the same address)
                store = wt_packed.__dict__.setdefault("_sf_classes", {})
                key = (at, ah, aw, tuple(kernel), tuple(stride), tuple(padding))
                wsub = store.get(key)
                if wsub is None:
                    wsub = _class_weights(wt_packed, store, kernel, stride, padding)[key]
                # a dense stride-1 conv of the class's taps; the descriptor always carries the output's pitch / offset
                # as the residual's (the pointer decides whether it is read)
                d = _conv_desc(dz, dims, out.cs, out.coff, cin, (len(tt), len(th), len(tw)), (1, 1, 1),
                               (-ot[0], -oh[0], -ow[0]), cin_pad=cout_pad, res=out,
                               scatter=(stride[0], stride[1], stride[2], at, ah, aw, out.T, out.H, out.W))
                _conv_launch(d, dz.ptr(), _ptr(wsub), None, None, out.ptr() if add else None, out.ptr(),
                             dz.buf.device, "sf_conv_fwd(strided dgrad class)", w_tensor=wsub, in_planes=dz_planes)
    return out


# ------------------------------------------------------------------------------------------------ backward
# Forward / data-gradient launches of conv_bx.hip take their activation operand as fp32 rows and split it after the LDS
# fragment read — no activation planes on those paths; the weight gradient (whose transposing LDS reads need 16-bit
# elements) makes the planes of x and dz itself, inside its own launch sequence on the companion stream.


def conv_wgrad(x, dz, cout, kernel, stride=(1, 1, 1), padding=(0, 0, 0), dilation=(1, 1, 1), cin=None,
               cin_pad=None, finish_into=None, x_planes=None, dz_planes=None):
    """dW packed [Cout, taps, cin_pad] = sum over positions of dz (x) x (split partials summed in fixed order).
    finish_into=(dst, Cin, fold_kw): instead of returning the packed gradient, sum the partials and ACCUMULATE
    them into dst, a contiguous tensor in nn.Conv3d's [Cout, Cin, kT, kH, kW] layout (e.g. the weight's .grad)."""
    _require_gpu(x.buf, "conv_wgrad")
    cin = x.C if cin is None else cin
    cin_pad = _pad16(cin) if cin_pad is None else cin_pad
    kT, kH, kW = kernel
    d = _conv_desc(x, (dz.T, dz.H, dz.W), 0, 0, cout, kernel, stride, padding, dilation, cin=cin, cin_pad=cin_pad)
    tag = ("conv", dz.rows, kT * kH * kW * cin, cout)
    nws = lib().sf_conv_wgrad_bx_ws_floats(ctypes.byref(d), 1 if x_planes is not None else 0,
                                           1 if dz_planes is not None else 0) if cin_pad == cin else 0
    if nws > 0:  # long reductions: the bf16-piece kernel of conv_bx.hip (operand planes handed in or made in ws)
        S = lib().sf_conv_wgrad_bx_splits(ctypes.byref(d))
        part = torch.empty((S, cout, kT * kH * kW, cin_pad), dtype=torch.float32, device=x.buf.device)
        ws = torch.empty((nws,), dtype=torch.float32, device=x.buf.device)
        # _REFUSED: a dz view the shape-only plan cannot see (odd channel offset / pitch)
        if _call("sf_conv_wgrad_bx", ctypes.byref(d), x.ptr(), _ptr(x_planes), dz.ptr(), dz.cs, dz.coff,
                 _ptr(dz_planes), _ptr(part), _ptr(ws), tag=tag, allow=_REFUSED) != 0:
            nws = 0
    if nws <= 0:
        S = lib().sf_conv_wgrad_splits(ctypes.byref(d))
        part = torch.empty((S, cout, kT * kH * kW, cin_pad), dtype=torch.float32, device=x.buf.device)
        _call("sf_conv_wgrad", ctypes.byref(d), x.ptr(), dz.ptr(), dz.cs, dz.coff, _ptr(part), tag=tag)
    if finish_into is not None:
        dst, real_cin, fold_kw = finish_into
        assert dst.is_contiguous() and dst.dtype == torch.float32
        if S > 128 and cout * kT * kH * kW * cin_pad > 65536:  # long split lists of large weights (does not occur
            part, S = part.sum(0, keepdim=True), 1  # in the shipped models): a parallel tree sum first
        assert dst.numel() == cout * real_cin * kT * kH * kW * max(fold_kw, 1), (dst.shape, cout, real_cin, kernel)
        _call("sf_conv_wgrad_finish", _ptr(part), S, cout, kT * kH * kW, cin_pad, real_cin, fold_kw, _ptr(dst), 1)
        return None
    return part.sum(0) if S > 1 else part[0]


# ------------------------------------------------------------------------------------------------ grouped convs
def conv_grouped(x, wp, groups, kernel, stride=(1, 1, 1), padding=(0, 0, 0), dilation=(1, 1, 1), scale=None,
                 bias=None, relu=False, res=None, out=None, shuffle=False, out_reserve=(0, 0)):
    """nn.Conv3d(groups = G), 1 < G < channels, as ONE launch (sf_conv_fwd_grouped: group = grid z of the LDS-tiled
    kernel).  wp = the packed weight [Cout][taps][pad(Cin / G)] (pack_conv_weight_pair of the grouped parameter: the G
    per-group packs one after the other).  shuffle: group g's channel j is stored at channel j*G + g."""
    _require_gpu(x.buf, "conv_grouped")
    cout, taps, cin_pad = wp.shape
    To, Ho, Wo = _out_thw(x, kernel, stride, padding, dilation)
    if out is None:
        out = new_act(x, x.N, To, Ho, Wo, cout, out_reserve[0], out_reserve[1])
    assert (out.N, out.T, out.H, out.W, out.C) == (x.N, To, Ho, Wo, cout), (out, (x.N, To, Ho, Wo, cout))
    assert x.C % groups == 0 and cout % groups == 0 and cin_pad >= x.C // groups, (x, wp.shape, groups)
    d = _conv_desc(x, (To, Ho, Wo), out.cs, out.coff, cout, kernel, stride, padding, dilation, cin_pad=cin_pad,
                   act=_act(relu), res=res)
    if res is not None:
        assert res.rows == out.rows and res.C == cout
    _call("sf_conv_fwd_grouped", ctypes.byref(d), groups, 1 if shuffle else 0, x.ptr(), _ptr(wp), _ptr(scale),
          _ptr(bias), res.ptr() if res is not None else None, out.ptr(),
          tag=("conv", d.N * d.To * d.Ho * d.Wo, taps * (x.C // groups), cout))
    return out


def conv_dgrad_grouped(dz, wtp, groups, x_like, kernel, stride=(1, 1, 1), padding=(0, 0, 0), dilation=(1, 1, 1),
                       out=None, accumulate=False):
    """Data gradient of a grouped conv in ONE launch: wtp = [Cin][taps][pad(Cout / G)], the G transposed per-group
    packs one after the other (group g: rows [g*Cin/G, (g+1)*Cin/G), reading dz channels [g*Cout/G, (g+1)*Cout/G)).
    Strided layers run the transposed gather with its taps predicated (no residue-class launches)."""
    _require_gpu(dz.buf, "conv_dgrad_grouped")
    cin, taps, cout_pad = wtp.shape
    if out is None:
        out = new_act(dz, x_like.N, x_like.T, x_like.H, x_like.W, cin)
        accumulate = False
    assert (out.N, out.T, out.H, out.W, out.C) == (x_like.N, x_like.T, x_like.H, x_like.W, cin), (out, x_like)
    assert dz.C % groups == 0 and cin % groups == 0 and cout_pad >= dz.C // groups
    d = _conv_desc(dz, (out.T, out.H, out.W), out.cs, out.coff, cin, kernel, stride, padding, dilation,
                   cin_pad=cout_pad, res=out if accumulate else None, transposed=1)
    _call("sf_conv_fwd_grouped", ctypes.byref(d), groups, 0, dz.ptr(), _ptr(wtp), None, None,
          out.ptr() if accumulate else None, out.ptr(), tag=("conv", dz.rows, taps * (dz.C // groups), cin),
          what="sf_conv_fwd_grouped(transposed)")
    return out


def conv_wgrad_grouped(x, dz, groups, kernel, stride=(1, 1, 1), padding=(0, 0, 0), dilation=(1, 1, 1),
                       cin_pad=None, finish_into=None):
    """Weight gradient of a grouped conv in ONE launch (+ the finish): packed [Cout][taps][cin_pad] with cin_pad =
    pad(Cin / G), or accumulated into finish_into = a contiguous tensor in nn.Conv3d's grouped layout
    [Cout][Cin / G][kT][kH][kW] (the parameter's gradient)."""
    _require_gpu(x.buf, "conv_wgrad_grouped")
    cin_g, cout = x.C // groups, dz.C
    assert x.C % groups == 0 and cout % groups == 0
    cin_pad = _pad16(cin_g) if cin_pad is None else cin_pad
    kT, kH, kW = kernel
    d = _conv_desc(x, (dz.T, dz.H, dz.W), 0, 0, cout, kernel, stride, padding, dilation, cin_pad=cin_pad)
    S = lib().sf_conv_wgrad_grouped_splits(ctypes.byref(d), groups)
    if S <= 0:
        raise SfhipError("sf_conv_wgrad_grouped_splits: %d -> %d channels in %d groups" % (x.C, cout, groups))
    part = torch.empty((S, cout, kT * kH * kW, cin_pad), dtype=torch.float32, device=x.buf.device)
    _call("sf_conv_wgrad_grouped", ctypes.byref(d), groups, x.ptr(), dz.ptr(), dz.cs, dz.coff, _ptr(part),
          tag=("conv", dz.rows, kT * kH * kW * cin_g, cout))
    if finish_into is not None:
        dst = finish_into
        assert dst.is_contiguous() and dst.dtype == torch.float32 and dst.numel() == cout * cin_g * kT * kH * kW
        _call("sf_conv_wgrad_finish", _ptr(part), S, cout, kT * kH * kW, cin_pad, cin_g, 0, _ptr(dst), 1)
        return None
    return part.sum(0) if S > 1 else part[0]


def unpack_conv_weight_grad(dwp, shape):
    """[Cout, taps, cin_pad] -> [Cout, Cin, kT, kH, kW]."""
    cout, cin, kT, kH, kW = shape
    return dwp[:, :, :cin].permute(0, 2, 1).reshape(cout, cin, kT, kH, kW).contiguous()


def _bn_bwd_y(who, y, z, relu, mask, plain):
    """(pointer, pitch, channel offset, activation code) of what a BN backward kernel takes its ReLU mask from: the
    activation y, or — code 3 — the byte mask affine(mask=...) left, read instead of it.  plain: the layer is neither
    T-repeated nor split, the only form a byte mask is made for."""
    if mask is not None and relu:
        if not plain or mask.numel() != z.rows * (z.C // 4) or not mask.is_cuda:
            raise SfhipError("%s: the byte mask holds rows * C/4 bytes of an un-repeated, un-split layer" % who)
        return _ptr(mask), z.C // 4, 0, 3
    code = 2 if relu == 6 else (1 if relu else 0)
    return (y.ptr(), y.cs, y.coff, code) if y is not None else (None, 0, 0, code)


def bn_bwd(dy, y, z, mean, invstd, gamma, relu, rep=1, dres=None, dz_out=None, dgamma_out=None, nsplit=1,
           sync=None, grad_sink=None, mask=None, dres_overwrite=False):
    """Training BN backward (+ReLU mask, + residual fan-out, + upsample-copy sum).  Returns (dz, dgamma, dbeta);
    dz is written over z unless dz_out is given.
    nsplit > 1 (SubBatchNorm3d): mean/invstd/gamma and the returned sums hold nsplit*C entries [split*C + c].
    sync (NaiveSyncBatchNorm3d): callable (dbeta, dgamma) -> (dbeta', dgamma') applied between the reduction and
    the normalisation pass (the cross-rank sum, already divided by the number of ranks); the LOCAL sums are
    returned for the parameter gradients."""
    C = z.C
    dev = z.buf.device
    mean, invstd, gamma = mean.contiguous(), invstd.contiguous(), gamma.detach().contiguous()
    dbeta = torch.empty((nsplit * C,), dtype=torch.float32, device=dev)
    dgamma = torch.empty((nsplit * C,), dtype=torch.float32, device=dev)
    ws = torch.empty((lib().sf_bn_bwd_ws_floats(C),), dtype=torch.float32, device=dev)
    yp, ycs, yco, code = _bn_bwd_y("bn_bwd", y, z, relu, mask, rep == 1 and nsplit == 1)
    head = (dy.ptr(), dy.cs, dy.coff, yp, ycs, yco, z.ptr(), z.cs, z.coff, z.N, z.T, z.H, z.W, C)
    tail = (rep, code, _ptr(mean), _ptr(invstd))
    split = (nsplit,) if nsplit > 1 else ()
    reduce_fn = "sf_bn_bwd_reduce_split" if nsplit > 1 else "sf_bn_bwd_reduce"
    apply_fn = "sf_bn_bwd_apply_split" if nsplit > 1 else "sf_bn_bwd_apply"
    if dres_overwrite:  # dres is an uninitialised buffer this call is the first writer of (dres = g, not +=)
        assert dres is not None and nsplit == 1
        apply_fn = "sf_bn_bwd_apply_first"
    if grad_sink is not None:  # (weight.grad[:C], bias.grad[:C]) accumulated by the reduction's final kernel
        assert nsplit == 1 and dgamma_out is None
        _call("sf_bn_bwd_reduce_acc", *head, *tail, _ptr(dbeta), _ptr(dgamma), _ptr(ws), _ptr(grad_sink[1]),
              _ptr(grad_sink[0]))
    else:
        _call(reduce_fn, *head, *split, *tail, _ptr(dbeta), _ptr(dgamma), _ptr(ws))
    db_apply, dg_apply = (dbeta, dgamma) if sync is None else sync(dbeta, dgamma)
    out = z if dz_out is None else dz_out
    _call(apply_fn, *head, *split, *tail, _ptr(gamma), _ptr(db_apply), _ptr(dg_apply), out.ptr(), out.cs, out.coff,
          dres.ptr() if dres is not None else None, dres.cs if dres is not None else 0,
          dres.coff if dres is not None else 0)
    if dgamma_out is not None:  # scatter into full-width parameter gradients (sliced BN, GhostModule)
        if nsplit > 1:
            dgamma_out[0][:C] = dgamma.view(nsplit, C).sum(0)
            dgamma_out[1][:C] = dbeta.view(nsplit, C).sum(0)
        else:
            dgamma_out[0][:C] = dgamma
            dgamma_out[1][:C] = dbeta
    return out, dgamma, dbeta


def bn_frozen_bwd(dy, y, z, mean, invstd, gamma, relu, rep=1, dres=None, dres_overwrite=False, dz_out=None,
                  grads=None, mask=None):
    """Backward of an eval-mode (frozen) BatchNorm3d epilogue y = act(gamma * (z - mean) * invstd + beta + res) under a
    training tape, ONE pass (sf_bn_frozen_bwd): dz = gamma * invstd * g over z (or into dz_out), dres (= | +=) g,
    g = sum over the `rep` T-copies of dy * mask.  mean / invstd: the running statistics as [C] tensors; gamma None: a BN
    without affine.  grads = (dgamma, dbeta): [>= C] float32 tensors the per-channel sums are ACCUMULATED into (zero-filled
    temporaries, or the parameters' .grad under the gradient sink); None: no parameter gradients.  relu: False / True /
    6; mask: the byte mask affine(mask=...) left, read instead of y.  Returns dz."""
    if dy is None or z is None or (relu and mask is None and y is None):
        raise SfhipError("bn_frozen_bwd: dy, z and (with an activation) y or its mask are required")
    for name, a in (("dy", dy), ("z", z), ("dz", dz_out), ("dres", dres), ("y", y if (relu and mask is None) else None)):
        if a is not None:
            _require_gpu(a.buf, "bn_frozen_bwd(%s)" % name)
    C, dev = z.C, z.buf.device
    if dres is not None and rep != 1:
        raise SfhipError("bn_frozen_bwd: the residual's gradient is only defined without a T repeat (rep = %d)" % rep)
    if (dy.N, dy.T, dy.H, dy.W, dy.C) != (z.N, z.T * rep, z.H, z.W, C):
        raise SfhipError("bn_frozen_bwd: dy %r does not match z %r repeated %d times" % (dy, z, rep))
    vecs = [("mean", mean), ("invstd", invstd)] + ([("gamma", gamma)] if gamma is not None else [])
    for name, v in vecs:
        _require_gpu(v, "bn_frozen_bwd(%s)" % name)
        if v.numel() < C or not v.is_contiguous():
            raise SfhipError("bn_frozen_bwd: %s must be a contiguous tensor of at least %d floats" % (name, C))
    dgp = dbp = ws = None
    if grads is not None:
        for name, v in (("dgamma", grads[0]), ("dbeta", grads[1])):
            _require_gpu(v, "bn_frozen_bwd(%s)" % name)
            if v.numel() < C or not v.is_contiguous():
                raise SfhipError("bn_frozen_bwd: %s must be a contiguous tensor of at least %d floats" % (name, C))
        dgp, dbp = _ptr(grads[0]), _ptr(grads[1])
        ws = torch.empty((lib().sf_bn_bwd_ws_floats(C),), dtype=torch.float32, device=dev)
    yp, ycs, yco, code = _bn_bwd_y("bn_frozen_bwd", y if relu else None, z, relu, mask, rep == 1)
    out = z if dz_out is None else dz_out
    _call("sf_bn_frozen_bwd", dy.ptr(), dy.cs, dy.coff, yp, ycs, yco, z.ptr(), z.cs, z.coff, z.N, z.T, z.H, z.W, C,
          rep, code, _ptr(mean.detach()), _ptr(invstd.detach()), _ptr(gamma.detach()) if gamma is not None else None,
          out.ptr(), out.cs, out.coff, dres.ptr() if dres is not None else None,
          dres.cs if dres is not None else 0, dres.coff if dres is not None else 0, 0 if dres_overwrite else 1,
          dbp, dgp, _ptr(ws))
    return out


def maxpool_bwd(x, y, dy, dx, kernel, stride, padding=(0, 0, 0), overwrite=False):
    """dx (+)= gathered dy; overwrite: dx is an uninitialised buffer this call is the first writer of."""
    d = _pool_desc(x, (y.T, y.H, y.W), y.cs, y.coff, kernel, stride, padding, False)
    _call("sf_maxpool_bwd_first" if overwrite else "sf_maxpool_bwd", ctypes.byref(d), x.ptr(), y.ptr(), dy.ptr(),
          dy.cs, dy.coff, dx.ptr(), dx.cs, dx.coff)
    return dx


def maxpool_bwd_arg(x_like, arg, dy, dx, kernel, stride, padding=(0, 0, 0), overwrite=False):
    """dx (+)= dy gathered through the winner map `arg` of pool(..., want_arg=True); x_like gives the input dims.
    Returns False (nothing launched) when the gradient views are not float4-addressable."""
    if not (dy.cs % 4 == 0 and dy.coff % 4 == 0 and dx.cs % 4 == 0 and dx.coff % 4 == 0 and
            dy.buf.data_ptr() % 16 == 0 and dx.buf.data_ptr() % 16 == 0):
        return False
    d = _pool_desc(x_like, (dy.T, dy.H, dy.W), dy.cs, dy.coff, kernel, stride, padding, False)
    _call("sf_maxpool_bwd_arg", ctypes.byref(d), _ptr(arg), dy.ptr(), dy.cs, dy.coff, dx.ptr(), dx.cs, dx.coff,
          1 if overwrite else 0)
    return True


def tmax_dot(x, alpha, dz):
    out = torch.empty((x.N, x.C), dtype=torch.float32, device=x.buf.device)
    ws = torch.empty((lib().sf_tmax_mean_ws_floats(x.N, x.C),), dtype=torch.float32, device=x.buf.device)
    _call("sf_tmax_dot", x.ptr(), x.cs, x.coff, x.N, x.T, x.H, x.W, x.C, alpha, dz.ptr(), dz.cs, dz.coff,
          _ptr(out), _ptr(ws))
    return out


def eca_bwd_apply(x, alpha, dz, gate, dpool, dx):
    _call("sf_eca_bwd_apply", x.ptr(), x.cs, x.coff, x.N, x.T, x.H, x.W, x.C, alpha, dz.ptr(), dz.cs, dz.coff,
          _ptr(gate), _ptr(dpool), dx.ptr(), dx.cs, dx.coff)
    return dx


def eca_gate_bwd(dg, pooled, w3, dpool_scale, dw3):
    """(gate, dpool) of the ECA gate's backward on [N, C] vectors; dw3 (3 floats) is accumulated in place."""
    n, c = pooled.shape
    gate = torch.empty_like(pooled)
    dpool = torch.empty_like(pooled)
    _call("sf_eca_gate_bwd", _ptr(dg), _ptr(pooled), _ptr(w3), n, c, float(dpool_scale), _ptr(gate), _ptr(dpool),
          _ptr(dw3))
    return gate, dpool


def bcast_add(g, v, scale):
    _call("sf_bcast_add", g.ptr(), g.cs, g.coff, g.N, g.T * g.H * g.W, g.C, _ptr(v), float(scale))
    return g


def rowdot(a, b, scale=1.0):
    out = torch.empty((a.rows,), dtype=torch.float32, device=a.buf.device)
    _call("sf_rowdot", a.ptr(), a.cs, a.coff, b.ptr(), b.cs, b.coff, a.rows, a.C, float(scale), _ptr(out))
    return out


def axpy(a, out, alpha=1.0, accumulate=True):
    assert a.rows == out.rows and a.C == out.C
    _call("sf_axpy", a.ptr(), a.cs, a.coff, float(alpha), out.ptr(), out.cs, out.coff, a.rows, a.C,
          1 if accumulate else 0)
    return out


def row_softmax(x, scale=1.0):
    """x <- softmax(scale * x) over the channel dimension, in place (one wavefront per row)."""
    _require_gpu(x.buf, "row_softmax")
    _call("sf_row_softmax_fwd", x.ptr(), x.cs, x.coff, x.rows, x.C, float(scale))
    return x


def row_softmax_bwd(p, dp, scale=1.0):
    """dp <- scale * p * (dp - <p, dp>) in place."""
    assert p.rows == dp.rows and p.C == dp.C
    _call("sf_row_softmax_bwd", p.ptr(), p.cs, p.coff, dp.ptr(), dp.cs, dp.coff, p.rows, p.C, float(scale))
    return dp


def act_bwd(dy, y, relu, dx, accumulate=True):
    """dx (+)= dy * [0 < y (< 6)] — backward of a bare ReLU (relu=True) / ReLU6 (relu=6)."""
    assert dy.rows == y.rows == dx.rows and dy.C == y.C == dx.C
    _call("sf_act_bwd", dy.ptr(), dy.cs, dy.coff, y.ptr(), y.cs, y.coff, _act(relu), dx.ptr(), dx.cs, dx.coff,
          dy.rows, dy.C, 1 if accumulate else 0)
    return dx


def attention_bwd(q, k, v, dz, o, lse, gamma, dq, dk, dv, workspace=True):
    """dq/dk/dv (Act slices, overwritten) of the flash SpatialAttention; returns dvec[i] = <dz_i, O_i>
    (its sum is dL/dgamma).  workspace: the single-sweep backward where it has one (16 < C <= 64: 5 GB scratch at
    N = 25088); False, or no workspace for the shape, takes the two-kernel form (no scratch)."""
    B, n, C = o.shape
    o_act = Act(o.view(B, 1, 1, n, C))
    dvec = rowdot(Act(dz.buf.view(B, 1, 1, n, dz.cs), dz.coff, C), o_act)
    args = (_slice_base(q), q.cs, _slice_base(k), k.cs, _slice_base(v), v.cs, _slice_base(dz), dz.cs, _ptr(lse),
            _ptr(dvec), _ptr(gamma), _slice_base(dq), dq.cs, _slice_base(dk), dk.cs, _slice_base(dv), dv.cs, B, n, C)
    nws = lib().sf_attn_bwd_fused_ws_floats(B, n, C) if workspace else 0
    if nws > 0:  # one sweep: S and dP are recomputed once (5 products), dQ summed over key-block planes
        ws = torch.empty((nws,), dtype=torch.float32, device=o.device)
        _call("sf_attn_bwd_fused", *args, _ptr(ws), tag=("attn_bwd_fused", B, n, C))
        return dvec
    for which, tag in ((1, "attn_bwd_dq"), (2, "attn_bwd_dkv")):
        _call("sf_attn_bwd", *args, which, tag=(tag, B, n, C))
    return dvec


def xattn_accepts(q, k, v):
    """True when the streaming cross-length kernels (attn_cross.hip) serve these views: shape inside
    sf_xattn_accepts and float4-addressable rows."""
    nq, nk = q.T * q.H * q.W, k.T * k.H * k.W
    if not lib().sf_xattn_accepts(nq, nk, q.C, v.C):
        return False
    return all(a.cs % 4 == 0 and a.coff % 4 == 0 and a.buf.data_ptr() % 16 == 0 for a in (q, k, v))


def cross_attention(q, k, v, sm_scale, save=None):
    """Y = softmax(sm_scale q k^T) v per sample, streaming (no score matrix): q [N, ., d] queries, k [N, ., d] keys,
    v [N, ., dv] values (any N_q, N_k).  Returns Y shaped like q with dv channels.
    save: optional dict that receives 'lse' ([N, N_q], log2 domain) for cross_attention_bwd."""
    _require_gpu(q.buf, "cross_attention")
    B, nq, nk, d, dv = q.N, q.T * q.H * q.W, k.T * k.H * k.W, q.C, v.C
    assert k.N == B and v.N == B and k.C == d and v.T * v.H * v.W == nk, (q, k, v)
    y = new_act(q, B, q.T, q.H, q.W, dv)
    lse = torch.empty((B, nq), dtype=torch.float32, device=q.buf.device)
    if save is not None:
        save["lse"] = lse
    _call("sf_xattn_fwd", _slice_base(q), q.cs, _slice_base(k), k.cs, _slice_base(v), v.cs, _slice_base(y), y.cs,
          _ptr(lse), B, nq, nk, d, dv, float(sm_scale), tag=("xattn_fwd", B, nq, nk, d, dv))
    return y


def cross_attention_bwd(q, k, v, y, dy, lse, sm_scale, dq, dk, dv, accumulate=(False, False, False)):
    """dq / dk / dv (Act views) of cross_attention from y, dy and the saved lse; accumulate[i] True adds to the view,
    False overwrites it.  Two launches (key-stationary dk, dv; query-stationary dq) after the <dy, y> row dots."""
    B, nq, nk, d, dvw = q.N, q.T * q.H * q.W, k.T * k.H * k.W, q.C, v.C
    dvec = rowdot(dy, y)
    nws = lib().sf_xattn_bwd_ws_floats(B, nq, nk, d, dvw)
    ws = torch.empty((nws,), dtype=torch.float32, device=q.buf.device) if nws > 0 else None
    mask = sum(1 << i for i, on in enumerate(accumulate) if on)
    _call("sf_xattn_bwd", _slice_base(q), q.cs, _slice_base(k), k.cs, _slice_base(v), v.cs, _slice_base(dy), dy.cs,
          _ptr(lse), _ptr(dvec), _slice_base(dq), dq.cs, _slice_base(dk), dk.cs, _slice_base(dv), dv.cs, mask, B, nq,
          nk, d, dvw, float(sm_scale), _ptr(ws), tag=("xattn_bwd", B, nq, nk, d, dvw))
    return dvec


def assoc_accepts(theta, phi, g):
    """True when the associative "dot_product" kernels (attn_assoc.hip) serve these views: shape inside
    sf_assoc_accepts and float4-addressable rows."""
    nq, nk = theta.T * theta.H * theta.W, phi.T * phi.H * phi.W
    if not lib().sf_assoc_accepts(nq, nk, theta.C, g.C):
        return False
    return all(a.cs % 4 == 0 and a.coff % 4 == 0 and a.buf.data_ptr() % 16 == 0 for a in (theta, phi, g))


def gram(a, b, alpha, transposed=False):
    """G[n] = alpha a[n]^T b[n] over the positions of the views a [N, ., da] and b [N, ., db]: a dense [N, da, db]
    tensor, or (G, Gt) with Gt = G^T as [N, db, da] from the same launch when `transposed` is set."""
    _require_gpu(a.buf, "gram")
    B, R, da, db = a.N, a.T * a.H * a.W, a.C, b.C
    assert b.N == B and b.T * b.H * b.W == R, (a, b)
    dev = a.buf.device
    G = torch.empty((B, da, db), dtype=torch.float32, device=dev)
    Gt = torch.empty((B, db, da), dtype=torch.float32, device=dev) if transposed else None
    nws = lib().sf_gram_ws_floats(B, R, da, db)
    ws = torch.empty((nws,), dtype=torch.float32, device=dev) if nws > 0 else None
    _call("sf_gram", _slice_base(a), a.cs, _slice_base(b), b.cs, _ptr(G), _ptr(Gt), B, R, da, db, float(alpha),
          _ptr(ws), tag=("gram", B, R, da, db))
    return (G, Gt) if transposed else G


def rowmat(x, w, alpha, out=None, accumulate=False):
    """Y[n, r, j] = alpha sum_i x[n, r, i] w[n, j, i]: x [N, ., k] view, w dense [N, n, k]; `out` (a view shaped like
    x with n channels, made when None) is overwritten, or added to when `accumulate` is set.  Returns it."""
    _require_gpu(x.buf, "rowmat")
    B, R, k = x.N, x.T * x.H * x.W, x.C
    assert w.dim() == 3 and w.shape[0] == B and w.shape[2] == k and w.is_contiguous(), (x, tuple(w.shape))
    _require_gpu(w, "rowmat")
    n = w.shape[1]
    if out is None:
        assert not accumulate
        out = new_act(x, B, x.T, x.H, x.W, n)
    assert out.N == B and out.T * out.H * out.W == R and out.C == n, (x, out)
    _call("sf_rowmat", _slice_base(x), x.cs, _ptr(w), _slice_base(out), out.cs, B, R, k, n, float(alpha),
          int(bool(accumulate)), tag=("rowmat", B, R, k, n))
    return out


def bn_train_stats(x, gamma, beta, eps, momentum, run_mean, run_var, nsplit=1):
    """Training BN statistics of the view + scale/shift + in-place running-stat update in two launches.
    Returns (mean, invstd, scale, shift).  nsplit > 1 (SubBatchNorm3d): sample n belongs to split n % nsplit and
    every array has nsplit*C entries laid out [split*C + c]."""
    _require_gpu(x.buf, "bn_train_stats")
    dev = x.buf.device
    o = torch.empty((5, nsplit * x.C), dtype=torch.float32, device=dev)
    ws = torch.empty((lib().sf_channel_stats_ws_floats(x.C),), dtype=torch.float32, device=dev)
    tail = (_ptr(gamma), _ptr(beta), float(eps), float(momentum), _ptr(run_mean), _ptr(run_var), _ptr(o[0]),
            _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), _ptr(o[4]), _ptr(ws))
    if nsplit == 1:
        _call("sf_bn_train_stats", x.ptr(), x.cs, x.coff, x.rows, x.C, *tail)
    else:
        _call("sf_bn_train_stats_split", x.ptr(), x.cs, x.coff, x.N, x.T * x.H * x.W, x.C, nsplit, *tail)
    return o[0], o[2], o[3], o[4]


def bn_train_stats_merge(parts, C, gamma, beta, eps, momentum, run_mean, run_var):
    """bn_train_stats from the per-tile rows a conv epilogue left (conv(..., stats=True)): one small launch, no pass
    over the activation.  Returns (mean, invstd, scale, shift)."""
    ws, rows = parts
    o = torch.empty((5, C), dtype=torch.float32, device=ws.device)
    _call("sf_bn_train_stats_merge", _ptr(ws), rows, C, _ptr(gamma), _ptr(beta), float(eps), float(momentum),
          _ptr(run_mean), _ptr(run_var), _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), _ptr(o[4]))
    return o[0], o[2], o[3], o[4]


def _dw_desc(x, dz, kernel, stride, padding, wpitch=None):
    return _conv_desc(x, (dz.T, dz.H, dz.W), 0, 0, x.C, kernel, stride, padding,
                      cin_pad=x.C if wpitch is None else wpitch)


def dwconv_bwd(x, dz, wp, kernel, stride, padding, dx=None, into=None):
    """Depthwise conv backward: returns dw [taps, C]; accumulates the data gradient into dx (if given).
    into: a contiguous tensor in the parameter's own layout [C, 1, kT, kH, kW] (its .grad) — the weight gradient is
    ACCUMULATED there by the reduction's final step (sf_dwconv_wgrad_param) and None is returned."""
    d = _dw_desc(x, dz, kernel, stride, padding, wp.shape[1])
    C = x.C
    ws = torch.empty((lib().sf_dwconv_wgrad_ws_floats(ctypes.byref(d), C),), dtype=torch.float32,
                     device=x.buf.device)
    if into is not None:
        assert into.is_contiguous() and into.dtype == torch.float32 and \
            into.numel() == C * kernel[0] * kernel[1] * kernel[2], (into.shape, C, kernel)
        dw = None
        _call("sf_dwconv_wgrad_param", ctypes.byref(d), x.ptr(), dz.ptr(), dz.cs, dz.coff, C, _ptr(into), 1, _ptr(ws))
    else:
        dw = torch.empty((kernel[0] * kernel[1] * kernel[2], C), dtype=torch.float32, device=x.buf.device)
        _call("sf_dwconv_wgrad", ctypes.byref(d), x.ptr(), dz.ptr(), dz.cs, dz.coff, C, _ptr(dw), _ptr(ws))
    if dx is not None:
        _call("sf_dwconv_dgrad", ctypes.byref(d), dz.ptr(), dz.cs, dz.coff, _ptr(wp), dx.ptr(), dx.cs, dx.coff, C)
    return dw


def dwconv_dgrad(x, dz, wp, kernel, stride, padding, dx):
    """dx += transposed depthwise conv of dz (data gradient only: constant-weight pooling)."""
    d = _dw_desc(x, dz, kernel, stride, padding, wp.shape[1])
    _call("sf_dwconv_dgrad", ctypes.byref(d), dz.ptr(), dz.cs, dz.coff, _ptr(wp), dx.ptr(), dx.cs, dx.coff, x.C)
    return dx


def gather_add(src, src_cmul, out, accumulate=True):
    """out[r, c] (+)= src[r, src.coff + c*src_cmul]."""
    _call("sf_gather_add", src.ptr(), src.cs, src.coff, src_cmul, out.ptr(), out.cs, out.coff, out.rows, out.C,
          1 if accumulate else 0)
    return out


# ------------------------------------------------------------------------------------------------ RoI head, windowed pool
def check_boxes(boxes, x):
    """boxes: [K, 5] float32 on x's device, rows (batch_idx, x1, y1, x2, y2).  Checks metadata only (no sync)."""
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] != 5:
        raise SfhipError("RoI boxes must be a [K, 5] tensor (batch_idx, x1, y1, x2, y2), got %s" % (
            tuple(boxes.shape) if isinstance(boxes, torch.Tensor) else type(boxes).__name__))
    if boxes.dtype != torch.float32:
        raise SfhipError("RoI boxes: expected float32, got %s" % boxes.dtype)
    if boxes.device != x.buf.device:
        raise SfhipError("RoI boxes are on %s, the features on %s" % (boxes.device, x.buf.device))
    return boxes.contiguous()


def roi_tpool(x):
    """AvgPool3d([T,1,1], stride 1) + squeeze: Act [N,T,H,W,C] -> dense Act [N,1,H,W,C]."""
    _require_gpu(x.buf, "roi_tpool")
    out = new_act(x, x.N, 1, x.H, x.W, x.C)
    _call("sf_roi_tpool_fwd", x.ptr(), x.cs, x.coff, x.N, x.T, x.H, x.W, x.C, out.ptr())
    return out


def roi_align_max(x, boxes, resolution, spatial_scale, aligned, out):
    """RoIAlign(resolution, spatial_scale, sampling_ratio 0, aligned) + MaxPool2d(resolution) in one launch.
    x: dense Act [N,1,H,W,C]; out: Act [K,1,1,1,C] (a slice of the head's concat buffer).  Returns the winner map
    (uint8 [K, C]) the backward routes through."""
    _require_gpu(x.buf, "roi_align_max")
    assert x.T == 1 and x.coff == 0 and x.cs == x.C, x
    boxes = check_boxes(boxes, x)
    K = boxes.shape[0]
    assert (out.N, out.T, out.H, out.W, out.C) == (K, 1, 1, 1, x.C), (out, K, x)
    arg = torch.empty((K, x.C), dtype=torch.uint8, device=x.buf.device)
    if K > 0:
        _call("sf_roi_align_max_fwd", x.ptr(), x.N, x.H, x.W, x.C, _ptr(boxes), K, int(resolution),
              float(spatial_scale), 1 if aligned else 0, out.ptr(), out.cs, out.coff, _ptr(arg))
    return arg


def roi_align_max_bwd(dy, arg, boxes, resolution, spatial_scale, aligned, dx, accumulate=True):
    """dx [N,T,H,W,C] (+)= (1/T) * dL/d(map): the backward of roi_tpool -> roi_align_max (T = 1: of roi_align_max
    alone).  dy: Act [K,1,1,1,C]; arg: roi_align_max's winner map.  Bitwise reproducible (gather form)."""
    _require_gpu(dx.buf, "roi_align_max_bwd")
    boxes = check_boxes(boxes, dx)
    K = boxes.shape[0]
    assert arg.dtype == torch.uint8 and tuple(arg.shape) == (K, dx.C) and arg.device == dx.buf.device
    assert (dy.N, dy.T, dy.H, dy.W, dy.C) == (K, 1, 1, 1, dx.C), (dy, dx)
    if K == 0 and accumulate:
        return dx
    _call("sf_roi_align_max_bwd", dy.ptr() if K else None, dy.cs, dy.coff, _ptr(arg), _ptr(boxes), K, dx.N, dx.T,
          dx.H, dx.W, dx.C, int(resolution), float(spatial_scale), 1 if aligned else 0, dx.ptr(), dx.cs, dx.coff,
          1 if accumulate else 0)
    return dx


def _window_desc(x, kernel, out_cs=0, out_coff=0):
    kernel = tuple(int(k) for k in kernel)
    return _pool_desc(x, _out_thw(x, kernel, (1, 1, 1), (0, 0, 0)), out_cs, out_coff, kernel, (1, 1, 1), (0, 0, 0),
                      True)


def avgpool_window(x, kernel, out=None):
    """nn.AvgPool3d(kernel, stride=1) of the fully-convolutional head: Act [N,T,H,W,C] -> Act [N,T-kt+1,H-kh+1,W-kw+1,C]
    (`out`: the pathway's slice of the concat buffer).  x is read once; bitwise reproducible."""
    _require_gpu(x.buf, "avgpool_window")
    assert len(kernel) == 3 and all(1 <= int(k) <= e for k, e in zip(kernel, (x.T, x.H, x.W))), (x, kernel)
    d = _window_desc(x, kernel)
    if out is None:
        out = new_act(x, x.N, d.To, d.Ho, d.Wo, x.C)
    else:
        _require_gpu(out.buf, "avgpool_window")
        assert (out.N, out.T, out.H, out.W, out.C) == (x.N, d.To, d.Ho, d.Wo, x.C), (x, kernel, out)
    d.out_cs, d.out_coff = out.cs, out.coff
    # trace tag: ("avgpool_window", algorithmic HBM bytes = the input once + the output once)
    nbytes = 4 * (x.rows + out.rows) * x.C
    _call("sf_avgpool_win_fwd", ctypes.byref(d), x.ptr(), out.ptr(), tag=("avgpool_window", nbytes))
    return out


def avgpool_window_bwd(dy, dx, kernel, overwrite=False):
    """dx [N,T,H,W,C] (+)= the backward of avgpool_window: 1/|kernel| * the sum of dy [N,T-kt+1,H-kh+1,W-kw+1,C] over
    the windows that hold each element.  overwrite: dx is an uninitialised buffer this call is the first writer of
    (every element is written, none read).  Bitwise reproducible (gather form)."""
    _require_gpu(dx.buf, "avgpool_window_bwd")
    _require_gpu(dy.buf, "avgpool_window_bwd")
    assert len(kernel) == 3 and all(1 <= int(k) <= e for k, e in zip(kernel, (dx.T, dx.H, dx.W))), (dx, kernel)
    d = _window_desc(dx, kernel, dy.cs, dy.coff)
    assert (dy.N, dy.T, dy.H, dy.W, dy.C) == (dx.N, d.To, d.Ho, d.Wo, dx.C), (dy, dx, kernel)
    # trace tag: algorithmic HBM bytes = dy once + dx written (read and written when accumulating)
    nbytes = 4 * (dy.rows + dx.rows * (1 if overwrite else 2)) * dx.C
    _call("sf_avgpool_win_bwd", ctypes.byref(d), dy.ptr(), dy.cs, dy.coff, dx.ptr(), dx.cs, dx.coff,
          1 if overwrite else 0, tag=("avgpool_window_bwd", nbytes))
    return dx


def sigmoid_bwd(y, dy, dx, accumulate=True):
    """dx (+)= dy * y * (1 - y) over dense tensors of one shape."""
    _require_gpu(y, "sigmoid_bwd")
    assert y.shape == dy.shape == dx.shape and y.is_contiguous() and dy.is_contiguous() and dx.is_contiguous()
    _call("sf_sigmoid_bwd", _ptr(y), _ptr(dy), _ptr(dx), y.numel(), 1 if accumulate else 0)
    return dx


# ------------------------------------------------------------------------------------------------ Grad-CAM
def epilogue_bwd(dy, y, dz, scale=None, relu=False, rep=1, dz_accumulate=False, dres=None, dres_accumulate=False,
                 act=None, groups=1):
    """Backward of the folded eval epilogue y = act(scale*z + bias + res) (repeated `rep` times along T):
    dz (=|+=) scale * sum_r dy*m(y); dres (=|+=) dy*m(y) in the same pass (rep 1 only).  dy / y: Acts with dz.T * rep
    frames; y is only read when there is an activation.  relu: False / True, the call sf_epilogue_bwd serves.  act
    (False / True / 6 for ReLU6, overrides relu) or groups > 1 — dy and y hold the channel-shuffled store of a grouped
    conv, dz channel g * C/groups + j reads channel j * groups + g — go to sf_epilogue_bwd_act."""
    _require_gpu(dy.buf, "epilogue_bwd")
    _require_gpu(dz.buf, "epilogue_bwd")
    extended = act is not None or groups != 1
    if act is None:
        assert relu in (False, True), "relu is a flag: ReLU6 is act=6"
        act = bool(relu)
    assert act in (False, True, 6), act
    assert groups >= 1 and dz.C % groups == 0 and (groups == 1 or (rep == 1 and dres is None)), (groups, dz, rep)
    assert (dy.N, dy.T, dy.H, dy.W, dy.C) == (dz.N, dz.T * rep, dz.H, dz.W, dz.C), (dy, dz, rep)
    if act:
        _require_gpu(y.buf, "epilogue_bwd")
        assert (y.N, y.T, y.H, y.W, y.C) == (dy.N, dy.T, dy.H, dy.W, dy.C), (y, dy)
    if dres is not None:
        _require_gpu(dres.buf, "epilogue_bwd")
        assert rep == 1 and (dres.N, dres.T, dres.H, dres.W, dres.C) == (dz.N, dz.T, dz.H, dz.W, dz.C), (dres, dz)
    assert scale is None or (scale.is_cuda and scale.dtype == torch.float32 and scale.is_contiguous() and
                             scale.numel() == dz.C)
    nbytes = 4 * dz.C * (dy.rows * (2 if act else 1) + dz.rows * (2 if dz_accumulate else 1) +
                         (dz.rows * (2 if dres_accumulate else 1) if dres is not None else 0))
    head = (dy.ptr(), dy.cs, dy.coff, y.ptr() if act else None, y.cs if act else 0, y.coff if act else 0,
            dz.N, dz.T, dz.H, dz.W, dz.C, rep, _ptr(scale))
    tail = (dz.ptr(), dz.cs, dz.coff, 1 if dz_accumulate else 0, dres.ptr() if dres is not None else None,
            dres.cs if dres is not None else 0, dres.coff if dres is not None else 0, 1 if dres_accumulate else 0)
    if extended:
        _call("sf_epilogue_bwd_act", *head, _act(act), groups, *tail, tag=("epilogue_bwd", nbytes))
    else:
        _call("sf_epilogue_bwd", *head, 1 if act else 0, *tail, tag=("epilogue_bwd", nbytes))
    return dz


def dwconv_dgrad_epi(x, dy, y, wp, kernel, stride, padding, dx, scale=None, relu=False, accumulate=True):
    """dx (=|+=) the data gradient of the depthwise conv that made y [= act(scale * dwconv(x) + bias)] from x, given
    dy = dL/dy: sf_dwconv_dgrad_epi masks and scales dy as it gathers it, so no dL/dz tensor is made.  x gives the input
    geometry only; wp [taps, pitch >= C] as dwconv takes it; relu: False / True / 6; y is read only with an activation.
    accumulate False: every element of dx is written (dx may be uninitialised)."""
    _require_gpu(dy.buf, "dwconv_dgrad_epi")
    _require_gpu(dx.buf, "dwconv_dgrad_epi")
    assert relu in (False, True, 6), relu
    assert (dx.N, dx.T, dx.H, dx.W, dx.C) == (x.N, x.T, x.H, x.W, x.C) and dy.C == x.C and dy.N == x.N, (dx, x, dy)
    assert wp.is_cuda and wp.dtype == torch.float32 and wp.is_contiguous() and \
        tuple(wp.shape) == (kernel[0] * kernel[1] * kernel[2], wp.shape[1]) and wp.shape[1] >= x.C, (wp.shape, x)
    if relu:
        _require_gpu(y.buf, "dwconv_dgrad_epi")
        assert (y.N, y.T, y.H, y.W, y.C) == (dy.N, dy.T, dy.H, dy.W, dy.C), (y, dy)
    assert scale is None or (scale.is_cuda and scale.dtype == torch.float32 and scale.is_contiguous() and
                             scale.numel() == x.C)
    d = _dw_desc(x, dy, kernel, stride, padding, wp.shape[1])
    # trace tag: algorithmic HBM bytes = dy (and y) once + dx written (read and written when accumulating)
    nbytes = 4 * x.C * (dy.rows * (2 if relu else 1) + dx.rows * (2 if accumulate else 1))
    _call("sf_dwconv_dgrad_epi", ctypes.byref(d), dy.ptr(), dy.cs, dy.coff, y.ptr() if relu else None,
          y.cs if relu else 0, y.coff if relu else 0, _ptr(wp), _ptr(scale), _act(relu), dx.ptr(), dx.cs, dx.coff, x.C,
          1 if accumulate else 0, tag=("dwconv_dgrad_epi", nbytes))
    return dx


def head_act_mean_bwd(logits, dout, act, dl, accumulate=False):
    """dl (Act shaped like `logits`, dense) (=|+=) the backward of head_act_mean given dout [N, K]."""
    _require_gpu(logits.buf, "head_act_mean_bwd")
    _require_gpu(dout, "head_act_mean_bwd")
    _require_gpu(dl.buf, "head_act_mean_bwd")
    assert logits.coff == 0 and logits.C == logits.cs and dl.coff == 0 and dl.C == dl.cs
    assert dl.buf.shape == logits.buf.shape and dout.is_contiguous() and tuple(dout.shape) == (logits.N, logits.C)
    _call("sf_head_act_mean_bwd", logits.ptr(), _ptr(dout), logits.N, logits.T * logits.H * logits.W, logits.C, act,
          dl.ptr(), 1 if accumulate else 0)
    return dl


def cam_weights(g):
    """w[n,t,c] = mean over h,w of the gradient view g -> torch [N, T, C]."""
    _require_gpu(g.buf, "cam_weights")
    w = torch.empty((g.N, g.T, g.C), dtype=torch.float32, device=g.buf.device)
    _call("sf_cam_weights", g.ptr(), g.cs, g.coff, g.N, g.T, g.H, g.W, g.C, _ptr(w))
    return w


def cam_map(a, w, want_raw=False):
    """Per-frame class-activation maps of the activation view `a` under the weights w [N,T,C]: torch [N,T,H,W] in
    [0, 1] (min-max normalised per frame, zero-range frames give zeros); want_raw: (cam, the map before normalisation)."""
    _require_gpu(a.buf, "cam_map")
    _require_gpu(w, "cam_map")
    assert w.is_contiguous() and tuple(w.shape) == (a.N, a.T, a.C), (tuple(w.shape), a)
    dev = a.buf.device
    ws = torch.empty((lib().sf_cam_map_ws_floats(a.N, a.H, a.W, a.C),), dtype=torch.float32, device=dev)
    cam = torch.empty((a.N, a.T, a.H, a.W), dtype=torch.float32, device=dev)
    raw = torch.empty_like(cam) if want_raw else None
    _call("sf_cam_map", a.ptr(), a.cs, a.coff, _ptr(w), a.N, a.T, a.H, a.W, a.C, _ptr(ws), _ptr(raw), _ptr(cam))
    return (cam, raw) if want_raw else cam


# ------------------------------------------------------------------------------------------------ context pooling
def _vec_nc(v, n, c, what):
    """A dense [N, C] float32 device vector set (or None)."""
    if v is not None:
        _require_gpu(v, what)
        if not v.is_contiguous() or v.numel() != n * c:
            raise SfhipError("%s: expected a contiguous tensor of %d x %d floats, got %s" % (what, n, c, tuple(v.shape)))
    return v


def ctx_pool(x, w, b=None):
    """Global-context pooling of ContextBlock3D ('att'): per sample softmax over the T*H*W positions of the logits
    w . x[pos] + b, ctx[n, c] = sum_pos p[pos] * x[n, pos, c] — ONE pass over the view x (sf_ctx_pool_fwd).
    w: [C] (any shape of C floats), b: [1] or None.  -> (ctx [N, C], lse [N])."""
    _require_gpu(x.buf, "ctx_pool")
    _vec_nc(w, 1, x.C, "ctx_pool(w)")
    _vec_nc(b, 1, 1, "ctx_pool(b)")
    dev, rows = x.buf.device, x.T * x.H * x.W
    ctx = torch.empty((x.N, x.C), dtype=torch.float32, device=dev)
    lse = torch.empty((x.N,), dtype=torch.float32, device=dev)
    ws = torch.empty((lib().sf_ctx_pool_ws_floats(x.N, rows, x.C),), dtype=torch.float32, device=dev)
    _call("sf_ctx_pool_fwd", x.ptr(), x.cs, x.coff, x.N, rows, x.C, _ptr(w), _ptr(b), _ptr(ctx), _ptr(lse), _ptr(ws),
          tag="ctx_pool")
    return ctx, lse


def ctx_pool_bwd(x, w, b, lse, ctx, dctx, dx, accumulate=True, dw=None, db=None, dw_accumulate=False, want_dw=True):
    """Backward of ctx_pool in ONE pass (sf_ctx_pool_bwd): dx (+)= dL/dx (accumulate=False: dx is written, the first
    writer needs no zero fill).  want_dw: also dL/dw, into `dw` ([C] floats; dw_accumulate: added to it, e.g. a
    parameter's .grad) or a new tensor; `db` (one float) receives the exact 0 the shift-invariant softmax leaves.
    Returns dw (None without want_dw)."""
    _require_gpu(x.buf, "ctx_pool_bwd")
    _require_gpu(dx.buf, "ctx_pool_bwd(dx)")
    n, c, dev, rows = x.N, x.C, x.buf.device, x.T * x.H * x.W
    if (dx.N, dx.T, dx.H, dx.W, dx.C) != (x.N, x.T, x.H, x.W, c):
        raise SfhipError("ctx_pool_bwd: dx %r does not match x %r" % (dx, x))
    _vec_nc(w, 1, c, "ctx_pool_bwd(w)")
    _vec_nc(b, 1, 1, "ctx_pool_bwd(b)")
    _vec_nc(lse, n, 1, "ctx_pool_bwd(lse)")
    _vec_nc(ctx, n, c, "ctx_pool_bwd(ctx)")
    _vec_nc(dctx, n, c, "ctx_pool_bwd(dctx)")
    ws = None
    if want_dw:
        if dw is None:
            assert not dw_accumulate
            dw = torch.empty((c,), dtype=torch.float32, device=dev)
        _vec_nc(dw, 1, c, "ctx_pool_bwd(dw)")
        _vec_nc(db, 1, 1, "ctx_pool_bwd(db)")
        ws = torch.empty((lib().sf_ctx_pool_ws_floats(n, rows, c),), dtype=torch.float32, device=dev)
    else:
        dw = db = None
    _call("sf_ctx_pool_bwd", x.ptr(), x.cs, x.coff, n, rows, c, _ptr(w), _ptr(b), _ptr(lse), _ptr(ctx), _ptr(dctx),
          dx.ptr(), dx.cs, dx.coff, 1 if accumulate else 0, _ptr(dw), _ptr(db), 1 if dw_accumulate else 0, _ptr(ws),
          tag="ctx_pool_bwd")
    return dw


def sample_affine(x, mul=None, add=None, out=None):
    """out[n, pos, c] = x[n, pos, c] * mul[n, c] + add[n, c] (mul / add: [N, C] tensors or None = 1 / 0): the broadcast
    of a per-sample channel vector over an activation, one pass (sf_sample_affine_fwd)."""
    _require_gpu(x.buf, "sample_affine")
    if out is None:
        out = new_act(x, x.N, x.T, x.H, x.W, x.C)
    elif (out.N, out.T, out.H, out.W, out.C) != (x.N, x.T, x.H, x.W, x.C):
        raise SfhipError("sample_affine: out %r does not match x %r" % (out, x))
    _require_gpu(out.buf, "sample_affine(out)")
    _vec_nc(mul, x.N, x.C, "sample_affine(mul)")
    _vec_nc(add, x.N, x.C, "sample_affine(add)")
    _call("sf_sample_affine_fwd", x.ptr(), x.cs, x.coff, x.N, x.T * x.H * x.W, x.C, _ptr(mul), _ptr(add), out.ptr(),
          out.cs, out.coff, tag="sample_affine")
    return out


def sample_affine_bwd(dy, dx, x=None, mul=None, accumulate=True, want_dmul=False, want_dadd=False):
    """Backward of sample_affine in one pass over dy (sf_sample_affine_bwd): dx (+)= dy * mul; with want_dmul (needs x)
    dmul[n, c] = sum_pos dy * x; with want_dadd dadd[n, c] = sum_pos dy.  -> (dmul, dadd), None where not wanted."""
    _require_gpu(dy.buf, "sample_affine_bwd")
    _require_gpu(dx.buf, "sample_affine_bwd(dx)")
    n, c, dev, rows = dy.N, dy.C, dy.buf.device, dy.T * dy.H * dy.W
    if (dx.N, dx.T, dx.H, dx.W, dx.C) != (dy.N, dy.T, dy.H, dy.W, c):
        raise SfhipError("sample_affine_bwd: dx %r does not match dy %r" % (dx, dy))
    if want_dmul:
        if x is None or (x.N, x.T, x.H, x.W, x.C) != (dy.N, dy.T, dy.H, dy.W, c):
            raise SfhipError("sample_affine_bwd: dmul needs x shaped like dy %r, got %r" % (dy, x))
        _require_gpu(x.buf, "sample_affine_bwd(x)")
    _vec_nc(mul, n, c, "sample_affine_bwd(mul)")
    dmul = torch.empty((n, c), dtype=torch.float32, device=dev) if want_dmul else None
    dadd = torch.empty((n, c), dtype=torch.float32, device=dev) if want_dadd else None
    ws = None
    if want_dmul or want_dadd:
        ws = torch.empty((lib().sf_sample_affine_ws_floats(n, rows, c),), dtype=torch.float32, device=dev)
    xv = x if want_dmul else None
    _call("sf_sample_affine_bwd", dy.ptr(), dy.cs, dy.coff, xv.ptr() if xv is not None else None,
          xv.cs if xv is not None else 0, xv.coff if xv is not None else 0, n, rows, c, _ptr(mul), dx.ptr(), dx.cs,
          dx.coff, 1 if accumulate else 0, _ptr(dmul), _ptr(dadd), _ptr(ws), tag="sample_affine_bwd")
    return dmul, dadd


# ------------------------------------------------------------------------------------------------ stripe pooling
STRIPE_MODES = {"mean": 0, "max": 1, "meanmax": 2, "sum": 3}  # SF_STRIPE_*


def _stripe_view(a, like, stripes, c, what):
    """None, or the [N, T, S, 1, c] view `a` beside the activation `like`."""
    if a is None:
        return (None, 0, 0)
    _require_gpu(a.buf, what)
    if (a.N, a.T, a.H, a.W, a.C) != (like.N, like.T, stripes, 1, c):
        raise SfhipError("%s: expected a [%d, %d, %d, 1, %d] view, got %r" % (what, like.N, like.T, stripes, c, a))
    return (a.ptr(), a.cs, a.coff)


def stripe_pool(x, stripes, mode="mean", out=None):
    """Pooling over the `stripes` horizontal stripes of every frame of x [N,T,H,W,C] (H % stripes == 0), ONE pass over x
    (sf_stripe_pool_fwd): mode 'mean', 'max', 'meanmax' (2C channels: mean | max) or 'sum'.
    -> (out Act [N, T, stripes, 1, Cout], arg): arg is the int32 [N, T, stripes, C] position of every maximum inside
    its stripe (the first of equal values), None for 'mean' / 'sum'."""
    _require_gpu(x.buf, "stripe_pool")
    if mode not in STRIPE_MODES:
        raise SfhipError("stripe_pool: unknown mode %r" % (mode,))
    stripes = int(stripes)
    if stripes <= 0 or x.H % stripes != 0:
        raise SfhipError("stripe_pool: %d stripes do not divide H = %d" % (stripes, x.H))
    cout = 2 * x.C if mode == "meanmax" else x.C
    if out is None:
        out = new_act(x, x.N, x.T, stripes, 1, cout)
    _stripe_view(out, x, stripes, cout, "stripe_pool(out)")
    arg = None
    if mode in ("max", "meanmax"):
        arg = torch.empty((x.N, x.T, stripes, x.C), dtype=torch.int32, device=x.buf.device)
    _call("sf_stripe_pool_fwd", x.ptr(), x.cs, x.coff, x.N, x.T, x.H, x.W, x.C, stripes, STRIPE_MODES[mode], out.ptr(),
          out.cs, out.coff, _ptr(arg), tag="stripe_pool")
    return out, arg


def stripe_add(x, v, out=None):
    """out[n,t,h,w,c] = x[n,t,h,w,c] + v[n,t,h // (H/S),c] for v [N,T,S,1,C]: the per-stripe broadcast add, one pass
    (sf_stripe_add_fwd).  out: a view shaped like x (a slice of a wider buffer, or x itself), default a new one."""
    _require_gpu(x.buf, "stripe_add")
    _require_gpu(v.buf, "stripe_add(v)")
    stripes = v.H
    if stripes <= 0 or x.H % stripes != 0:
        raise SfhipError("stripe_add: %d stripes do not divide H = %d" % (stripes, x.H))
    vv = _stripe_view(v, x, stripes, x.C, "stripe_add(v)")
    if out is None:
        out = new_act(x, x.N, x.T, x.H, x.W, x.C)
    elif (out.N, out.T, out.H, out.W, out.C) != (x.N, x.T, x.H, x.W, x.C):
        raise SfhipError("stripe_add: out %r does not match x %r" % (out, x))
    _require_gpu(out.buf, "stripe_add(out)")
    _call("sf_stripe_add_fwd", x.ptr(), x.cs, x.coff, *vv, x.N, x.T, x.H, x.W, x.C, stripes, out.ptr(), out.cs,
          out.coff, tag="stripe_add")
    return out


def stripe_pool_bwd(dx, stripes, dz=None, dmean=None, dmax=None, arg=None, accumulate=True):
    """dx (+)= dz + dmean / (hs*W) + [position == arg] * dmax in one pass (sf_stripe_pool_bwd): the gradient of
    z = x + broadcast(f(stripe_pool(x))) with respect to x, given dz (shaped like dx) and the gradients dmean / dmax
    ([N,T,S,1,C] views) of the pooled values; each of the three may be None.  accumulate=False writes every element."""
    _require_gpu(dx.buf, "stripe_pool_bwd(dx)")
    stripes = int(stripes)
    if stripes <= 0 or dx.H % stripes != 0:
        raise SfhipError("stripe_pool_bwd: %d stripes do not divide H = %d" % (stripes, dx.H))
    gz = (None, 0, 0)
    if dz is not None:
        _require_gpu(dz.buf, "stripe_pool_bwd(dz)")
        if (dz.N, dz.T, dz.H, dz.W, dz.C) != (dx.N, dx.T, dx.H, dx.W, dx.C):
            raise SfhipError("stripe_pool_bwd: dz %r does not match dx %r" % (dz, dx))
        gz = (dz.ptr(), dz.cs, dz.coff)
    gm = _stripe_view(dmean, dx, stripes, dx.C, "stripe_pool_bwd(dmean)")
    gx = _stripe_view(dmax, dx, stripes, dx.C, "stripe_pool_bwd(dmax)")
    if dmax is not None:
        if arg is None or arg.dtype != torch.int32 or not arg.is_contiguous() or not arg.is_cuda or \
                tuple(arg.shape) != (dx.N, dx.T, stripes, dx.C):
            raise SfhipError("stripe_pool_bwd: dmax needs the int32 [N, T, S, C] positions stripe_pool returned")
    _call("sf_stripe_pool_bwd", *gz, *gm, *gx, _ptr(arg) if dmax is not None else None, dx.N, dx.T, dx.H, dx.W, dx.C,
          stripes, dx.ptr(), dx.cs, dx.coff, 1 if accumulate else 0, tag="stripe_pool_bwd")
    return dx


SF_TSTATS_BINS, SF_TSTATS_ROW = 24, 58  # include/sfhip.h: exponent bins per sign; 8-byte slots of a tensor's row


def tensor_stats(table_host, table, chunks_host, chunks, ws, ring, cursor):
    """One `sf_tensor_stats` call (two launches): the statistics row of every tensor of the (address, numel) table into
    slot cursor[0] of `ring` (int64 [slots, n_tensors, SF_TSTATS_ROW] on the GPU; fp32 / fp64 fields are views of the
    same slots), cursor (int32 [2] on the GPU: next slot, calls made) advanced by the call itself.  ws: a contiguous GPU
    tensor of at least sf_tensor_stats_ws_bytes(n_chunks) bytes.  The host tensors are what the device ones were uploaded
    from; an address of 0 is an absent tensor (a zero row).  No host read: capturable."""
    for h, d in ((table_host, table), (chunks_host, chunks)):
        assert h.dtype == d.dtype == torch.int64 and h.is_contiguous() and d.is_contiguous() and not h.is_cuda
        assert h.shape == d.shape
    if not (table.is_cuda and chunks.is_cuda and ws.is_cuda and ring.is_cuda and cursor.is_cuda):
        raise SfhipError("tensor_stats: table, chunks, ws, ring and cursor live on the GPU — there is no CPU fallback")
    assert ring.dtype == torch.int64 and ring.is_contiguous() and ring.dim() == 3 and ring.shape[1] == table_host.shape[0]
    assert cursor.dtype == torch.int32 and cursor.is_contiguous() and cursor.numel() == 2 and ws.is_contiguous()
    _call("sf_tensor_stats", _ptr(table_host), _ptr(table), table_host.shape[0], _ptr(chunks_host), _ptr(chunks),
          chunks_host.shape[0], _ptr(ws), ws.numel() * ws.element_size(), _ptr(ring), ring.shape[2], ring.shape[0],
          ctypes.cast(ctypes.c_void_p(cursor.data_ptr()), _pi), tag="tensor_stats")
