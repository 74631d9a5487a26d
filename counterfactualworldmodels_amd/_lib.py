"""ctypes binding of libcwm_hip.so (C ABI: include/cwm_hip.h).

There is no CPU fallback: if the library cannot be loaded every entry point raises.
`import torch` must happen before the library is loaded so that both share one HIP runtime
(libamdhip64.so.7 is resolved by soname to the copy torch already mapped).
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from functools import partial
from typing import Optional

import torch  # noqa: F401  (loads libamdhip64 first; see module docstring)

from . import build as _build

MODE_FAST = 1
MODE_PARITY = 2
ERR_INVALID = -1
ERR_HIP = -2
ERR_MASK = -3
KCLASS_GEMM = 0
KCLASS_ATTENTION = 1
KCLASS_GEMM_WIDE = 2    # 256x256 8-phase kernel launches (booked together with KCLASS_GEMM)
KCLASS_GEMM_NARROW = 3  # 128x128 kernel launches
KCLASS_LAYERNORM, KCLASS_PATCH_GATHER, KCLASS_FILL_MASK, KCLASS_UNEMBED = 4, 5, 6, 7  # HBM-bound: `total_flops` = algorithmic BYTES
KCLASS_CROSS_ATTN, KCLASS_SMALL_ATTN = 8, 9  # IMU-conditioned model

_MODES = {"fast": MODE_FAST, "parity": MODE_PARITY, MODE_FAST: MODE_FAST, MODE_PARITY: MODE_PARITY}


def mode_id(mode) -> int:
    try:
        return _MODES[mode]
    except KeyError:
        raise ValueError("mode must be 'fast' or 'parity', got %r" % (mode,))


RAFT_CORR_ALL_PAIRS, RAFT_CORR_ON_THE_FLY = 0, 1  # include/cwm_hip.h cwm_raft_set_corr
_RAFT_CORRS = {"all_pairs": RAFT_CORR_ALL_PAIRS, "on_the_fly": RAFT_CORR_ON_THE_FLY}


def raft_corr_id(corr) -> int:
    try:
        return _RAFT_CORRS[corr]
    except (KeyError, TypeError):
        raise ValueError("corr must be 'all_pairs' or 'on_the_fly', got %r" % (corr,))


class CwmConfig(C.Structure):
    _fields_ = [
        ("img_h", C.c_int32),
        ("img_w", C.c_int32),
        ("patch", C.c_int32),
        ("num_frames", C.c_int32),
        ("in_chans", C.c_int32),
        ("enc_dim", C.c_int32),
        ("enc_depth", C.c_int32),
        ("enc_heads", C.c_int32),
        ("dec_dim", C.c_int32),
        ("dec_depth", C.c_int32),
        ("dec_heads", C.c_int32),
        ("mlp_ratio", C.c_int32),
        ("ln_eps", C.c_float),
    ]


class CwmForwardArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),  # = C.sizeof(CwmForwardArgs): new_forward_args() sets it
        ("x_dev", C.c_void_p),
        ("x_stride_b", C.c_int64),
        ("x_stride_c", C.c_int64),
        ("x_stride_t", C.c_int64),
        ("normalize", C.c_int32),
        ("mask_dev", C.c_void_p),
        ("batch", C.c_int32),
        ("n_vis", C.c_int32),
        ("y_tokens_dev", C.c_void_p),
        ("y_video_dev", C.c_void_p),
        ("xraw_dev", C.c_void_p),
        ("mode", C.c_int32),
        ("check", C.c_int32),
        ("stream", C.c_void_p),
    ]


class CwmPatchErrorArgs(C.Structure):
    """cwm_patch_error_args (include/cwm_hip.h); new_patch_error_args() sets struct_size"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("y_tokens_dev", C.c_void_p),
        ("x_dev", C.c_void_p),
        ("x_stride_b", C.c_int64),
        ("x_stride_t", C.c_int64),
        ("x_stride_c", C.c_int64),
        ("target_dev", C.c_void_p),
        ("target_stride_b", C.c_int64),
        ("target_stride_t", C.c_int64),
        ("target_stride_c", C.c_int64),
        ("mask_dev", C.c_void_p),
        ("region_dev", C.c_void_p),
        ("batch", C.c_int32),
        ("T", C.c_int32),
        ("C", C.c_int32),
        ("H", C.c_int32),
        ("W", C.c_int32),
        ("P", C.c_int32),
        ("n_vis", C.c_int32),
        ("frame", C.c_int32),
        ("map_dev", C.c_void_p),
        ("mean_dev", C.c_void_p),
        ("scratch_dev", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class CwmTokenResponseArgs(C.Structure):
    """cwm_token_response_args (include/cwm_hip.h): cwm_patch_error_args as `base` (geometry, mask, tokens, per-patch map, scratch and the stream), the
    prediction compared against and the outputs; new_token_response_args() sets struct_size"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmPatchErrorArgs),
        ("y_ref_dev", C.c_void_p),
        ("y_ref_stride_b", C.c_int64),
        ("pixel_map_dev", C.c_void_p),
        ("peak_index_dev", C.c_void_p),
        ("stats_dev", C.c_void_p),
    ]


class CwmUnmaskStepArgs(C.Structure):
    """cwm_unmask_step_args (include/cwm_hip.h): cwm_patch_error_args as `base` (the error map's inputs, the mask and the stream), the frame, the selection rule
    and the outputs; new_unmask_step_args() sets struct_size"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmPatchErrorArgs),
        ("frame", C.c_int32),
        ("num_reveal", C.c_int32),
        ("mode", C.c_int32),
        ("self_mask", C.c_int32),
        ("threshold_dev", C.c_void_p),
        ("e_dev", C.c_void_p),
        ("mask_out_dev", C.c_void_p),
        ("picks_dev", C.c_void_p),
        ("dist_dev", C.c_void_p),
        ("frontier_dev", C.c_void_p),
    ]


class CwmSegmentStepArgs(C.Structure):
    """cwm_segment_step_args (include/cwm_hip.h): cwm_patch_error_args as `base` (batch, T, H, W, P and the stream are read), the flow samples by five strides, the
    seeds, the thresholds, the selection and the outputs; new_segment_step_args() sets struct_size"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmPatchErrorArgs),
        ("flows_dev", C.c_void_p),
        ("flow_strides", C.c_int64 * 5),
        ("C", C.c_int32),
        ("S", C.c_int32),
        ("seeds_dev", C.c_void_p),
        ("dirs_dev", C.c_void_p),
        ("min_seed_mag", C.c_float),
        ("abs_thresh", C.c_float),
        ("rel_thresh", C.c_float),
        ("vote_frac", C.c_float),
        ("cos_min", C.c_float),
        ("inside_frac", C.c_float),
        ("k_active", C.c_int32),
        ("k_passive", C.c_int32),
        ("ring_radius", C.c_int32),
        ("keys_dev", C.c_void_p),
        ("seed_ref_dev", C.c_void_p),
        ("votes_dev", C.c_void_p),
        ("segment_dev", C.c_void_p),
        ("cover_dev", C.c_void_p),
        ("stats_dev", C.c_void_p),
        ("picks_dev", C.c_void_p),
        ("active_out_dev", C.c_void_p),
        ("passive_out_dev", C.c_void_p),
    ]


class CwmSegmentMergeArgs(C.Structure):
    """cwm_segment_merge_args (include/cwm_hip.h): cwm_patch_error_args as `base` (batch, T, H, W, P and the stream are read), the candidate segments by two
    strides, the scores, the thresholds, the workspace and the outputs; new_segment_merge_args() sets struct_size"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmPatchErrorArgs),
        ("K", C.c_int32),
        ("segs_dev", C.c_void_p),
        ("seg_strides", C.c_int64 * 2),
        ("scores_dev", C.c_void_p),
        ("min_area", C.c_int32),
        ("max_area", C.c_int32),
        ("iou_thresh", C.c_float),
        ("contain_thresh", C.c_float),
        ("absorb", C.c_int32),
        ("work_dev", C.c_void_p),
        ("work_bytes", C.c_uint64),
        ("labels_dev", C.c_void_p),
        ("owner_dev", C.c_void_p),
        ("area_dev", C.c_void_p),
        ("label_area_dev", C.c_void_p),
        ("inter_dev", C.c_void_p),
        ("cover_dev", C.c_void_p),
        ("stats_dev", C.c_void_p),
    ]


class CwmSeedSelectArgs(C.Structure):
    """cwm_seed_select_args (include/cwm_hip.h): cwm_patch_error_args as `base` (batch, H, W, P and the stream are read), the score map as pixels by two strides
    or as cells, the free cells, the race's draws, the prior cells, the selection rule, the workspace and the outputs; new_seed_select_args() sets struct_size"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmPatchErrorArgs),
        ("map_dev", C.c_void_p),
        ("cells", C.c_int32),
        ("map_strides", C.c_int64 * 2),
        ("free_dev", C.c_void_p),
        ("e_dev", C.c_void_p),
        ("prior_dev", C.c_void_p),
        ("n_prior", C.c_int32),
        ("K", C.c_int32),
        ("radius", C.c_int32),
        ("peaks_only", C.c_int32),
        ("abs_thresh", C.c_float),
        ("rel_thresh", C.c_float),
        ("work_dev", C.c_void_p),
        ("work_bytes", C.c_uint64),
        ("seeds_dev", C.c_void_p),
        ("cells_dev", C.c_void_p),
        ("values_dev", C.c_void_p),
        ("pooled_dev", C.c_void_p),
        ("peaks_dev", C.c_void_p),
        ("stats_dev", C.c_void_p),
    ]


class CwmSegmentTrackArgs(C.Structure):
    """cwm_segment_track_args (include/cwm_hip.h): cwm_patch_error_args as `base` (batch, H, W and the stream are read), the previous track map and this frame's
    label map by a row stride each, the backward flow by two strides, the state in, the linking rule, the workspace and the outputs; new_segment_track_args()
    sets struct_size"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmPatchErrorArgs),
        ("prev_dev", C.c_void_p),
        ("prev_stride", C.c_int64),
        ("cur_dev", C.c_void_p),
        ("cur_stride", C.c_int64),
        ("flow_dev", C.c_void_p),
        ("flow_strides", C.c_int64 * 2),
        ("track_id_in_dev", C.c_void_p),
        ("age_in_dev", C.c_void_p),
        ("next_id_in_dev", C.c_void_p),
        ("iou_thresh", C.c_float),
        ("min_inter", C.c_int32),
        ("min_area", C.c_int32),
        ("max_age", C.c_int32),
        ("carry", C.c_int32),
        ("work_dev", C.c_void_p),
        ("work_bytes", C.c_uint64),
        ("out_dev", C.c_void_p),
        ("out_stride", C.c_int64),
        ("track_id_out_dev", C.c_void_p),
        ("age_out_dev", C.c_void_p),
        ("next_id_out_dev", C.c_void_p),
        ("area_dev", C.c_void_p),
        ("bbox_dev", C.c_void_p),
        ("moments_dev", C.c_void_p),
        ("slot_of_cur_dev", C.c_void_p),
        ("linked_cur_dev", C.c_void_p),
        ("table_dev", C.c_void_p),
        ("warped_dev", C.c_void_p),
        ("stats_dev", C.c_void_p),
    ]


class CwmFlowConsistencyArgs(C.Structure):
    """cwm_flow_consistency_args (include/cwm_hip.h): cwm_patch_error_args as `base` (batch, H, W, P and the stream are read), the checked flow and the other
    flow by two strides each, the threshold, the `both` flag and the outputs; new_flow_consistency_args() sets struct_size"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmPatchErrorArgs),
        ("a_dev", C.c_void_p),
        ("a_strides", C.c_int64 * 2),
        ("o_dev", C.c_void_p),
        ("o_strides", C.c_int64 * 2),
        ("alpha", C.c_float),
        ("beta", C.c_float),
        ("both", C.c_int32),
        ("code_dev", C.c_void_p),
        ("res_dev", C.c_void_p),
        ("masked_dev", C.c_void_p),
        ("cell_dev", C.c_void_p),
        ("stats_dev", C.c_void_p),
    ]


class CwmObjectMotionArgs(C.Structure):
    """cwm_object_motion_args (include/cwm_hip.h): cwm_patch_error_args as `base` (batch, T, H, W and the stream are read), the slot map, the flow, the codes and
    the other frame's slot map by their batch and frame strides, the thresholds of the fit and the outputs; new_object_motion_args() sets struct_size"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmPatchErrorArgs),
        ("labels_dev", C.c_void_p),
        ("labels_strides", C.c_int64 * 2),
        ("flow_dev", C.c_void_p),
        ("flow_strides", C.c_int64 * 3),
        ("code_dev", C.c_void_p),
        ("code_strides", C.c_int64 * 2),
        ("other_dev", C.c_void_p),
        ("other_strides", C.c_int64 * 2),
        ("min_pixels", C.c_int32),
        ("min_affine", C.c_int32),
        ("min_det", C.c_double),
        ("sums_dev", C.c_void_p),
        ("counts_dev", C.c_void_p),
        ("model_dev", C.c_void_p),
        ("occ_dev", C.c_void_p),
    ]


class CwmPointTrackArgs(C.Structure):
    """cwm_point_track_args (include/cwm_hip.h): cwm_patch_error_args as `base` (batch, T frames, H, W and the stream are read), the pair flows by three strides
    each, the threshold, the slot maps and the model table by their batch and frame strides, the points, their start frames and the outputs;
    new_point_track_args() sets struct_size and the defaults alpha = 0.01, beta = 0.5, max_coast = 8"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmPatchErrorArgs),
        ("fwd_dev", C.c_void_p),
        ("fwd_strides", C.c_int64 * 3),
        ("bwd_dev", C.c_void_p),
        ("bwd_strides", C.c_int64 * 3),
        ("alpha", C.c_float),
        ("beta", C.c_float),
        ("labels_dev", C.c_void_p),
        ("labels_strides", C.c_int64 * 2),
        ("model_dev", C.c_void_p),
        ("model_strides", C.c_int64 * 2),
        ("points_dev", C.c_void_p),
        ("start_dev", C.c_void_p),
        ("K", C.c_int32),
        ("max_coast", C.c_int32),
        ("xy_dev", C.c_void_p),
        ("state_dev", C.c_void_p),
        ("under_dev", C.c_void_p),
        ("owner_dev", C.c_void_p),
    ]


class CwmObjectResponseArgs(C.Structure):
    """cwm_object_response_args (include/cwm_hip.h): cwm_patch_error_args as `base` (batch scenes, T pushes per scene, H, W and the stream are read), the flow
    samples by five strides, the slot maps by their scene and push strides, the pushed slots, the shifts, the thresholds and the outputs;
    new_object_response_args() sets struct_size"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmPatchErrorArgs),
        ("flows_dev", C.c_void_p),
        ("flow_strides", C.c_int64 * 5),
        ("S", C.c_int32),
        ("labels_dev", C.c_void_p),
        ("labels_strides", C.c_int64 * 2),
        ("pushed_dev", C.c_void_p),
        ("dirs_dev", C.c_void_p),
        ("min_q2", C.c_int64),
        ("min_pixels", C.c_int32),
        ("self_frac", C.c_double),
        ("move_frac", C.c_double),
        ("tab_dev", C.c_void_p),
        ("valid_dev", C.c_void_p),
        ("agg_dev", C.c_void_p),
        ("coupling_dev", C.c_void_p),
        ("stats_dev", C.c_void_p),
    ]


class CwmParallaxArgs(C.Structure):
    """cwm_parallax_args (include/cwm_hip.h): cwm_patch_error_args as `base` (batch rows, H, W and the stream are read), the flow samples by five strides, the
    shifts, the slot maps by their row stride, the thresholds and the outputs; new_parallax_args() sets struct_size"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmPatchErrorArgs),
        ("flows_dev", C.c_void_p),
        ("flow_strides", C.c_int64 * 5),
        ("S", C.c_int32),
        ("dirs_dev", C.c_void_p),
        ("labels_dev", C.c_void_p),
        ("labels_stride", C.c_int64),
        ("ref_slot", C.c_int32),
        ("min_pixels", C.c_int32),
        ("min_ref_q", C.c_int64),
        ("min_samples", C.c_int32),
        ("par_dev", C.c_void_p),
        ("spread_dev", C.c_void_p),
        ("off_dev", C.c_void_p),
        ("cnt_dev", C.c_void_p),
        ("ref_dev", C.c_void_p),
        ("hist_dev", C.c_void_p),
        ("slot_tab_dev", C.c_void_p),
    ]


class CwmConjConfig(C.Structure):
    _fields_ = [
        ("main", CwmConfig),
        ("main_max_pad", C.c_int32),
        ("ctx_in_chans", C.c_int32),
        ("ctx_seq_len", C.c_int32),
        ("ctx_tubelet", C.c_int32),
        ("ctx_enc_dim", C.c_int32),
        ("ctx_dec_dim", C.c_int32),
        ("ctx_enc_heads", C.c_int32),
        ("ctx_dec_heads", C.c_int32),
        ("ctx_max_pad", C.c_int32),
        ("n_enc_cross", C.c_int32),
        ("enc_cross", C.c_int32 * 16),
        ("n_dec_cross", C.c_int32),
        ("dec_cross", C.c_int32 * 16),
        ("cross_heads", C.c_int32),
        ("cross_mlp_ratio", C.c_int32),
    ]


class CwmConjForwardArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("x_dev", C.c_void_p),
        ("x_stride_b", C.c_int64),
        ("x_stride_c", C.c_int64),
        ("x_stride_t", C.c_int64),
        ("normalize", C.c_int32),
        ("mask_dev", C.c_void_p),
        ("batch", C.c_int32),
        ("n_vis_max", C.c_int32),
        ("ctx_dev", C.c_void_p),
        ("ctx_mask_dev", C.c_void_p),
        ("n_vis_ctx_max", C.c_int32),
        ("y_tokens_dev", C.c_void_p),
        ("mode", C.c_int32),
        ("check", C.c_int32),
        ("stream", C.c_void_p),
        ("y_ctx_tokens_dev", C.c_void_p),
        ("flow_fwd_dev", C.c_void_p),
        ("flow_fwd_stride_b", C.c_int64),
        ("flow_fwd_stride_c", C.c_int64),
        ("flow_bwd_dev", C.c_void_p),
        ("flow_bwd_stride_b", C.c_int64),
        ("flow_bwd_stride_c", C.c_int64),
    ]


CONJ_INPUT_FRAMES, CONJ_INPUT_FLOWBACK_RGB01 = 0, 1


class CwmConjVariant(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("padded", C.c_int32),
        ("ctx_dummy_token", C.c_int32),
        ("main_input", C.c_int32),
    ]


class CwmRaftForwardArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("image1_dev", C.c_void_p),
        ("image1_stride_b", C.c_int64),
        ("image1_stride_t", C.c_int64),
        ("image1_stride_c", C.c_int64),
        ("image2_dev", C.c_void_p),
        ("image2_stride_b", C.c_int64),
        ("image2_stride_t", C.c_int64),
        ("image2_stride_c", C.c_int64),
        ("batch", C.c_int32),
        ("pairs", C.c_int32),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("input_scale", C.c_float),
        ("iters", C.c_int32),
        ("flow_dev", C.c_void_p),
        ("flow_stride_b", C.c_int64),
        ("flow_stride_t", C.c_int64),
        ("flow_stride_c", C.c_int64),
        ("flow_low_dev", C.c_void_p),
        ("stream", C.c_void_p),
        ("head_dev", C.c_void_p),  # appended in 0.10.1 (the output head)
        ("head_stride_b", C.c_int64),
        ("head_stride_t", C.c_int64),
        ("head_stride_c", C.c_int64),
        ("mode", C.c_int32),  # appended in 0.10.2: 0 or MODE_PARITY = parity, MODE_FAST = bf16-operand convolutions
    ]


def new_args(cls):
    """a zeroed args structure with its struct_size set, and its base's where it embeds another args structure as `base` (the read-outs' cwm_patch_error_args,
    cwm_raft_forward_ex_args' cwm_raft_forward_args)"""
    a = cls()
    a.struct_size = C.sizeof(cls)
    if hasattr(a, "base"):
        a.base.struct_size = C.sizeof(type(a.base))
    return a


new_raft_forward_args = partial(new_args, CwmRaftForwardArgs)


class CwmRaftForwardExArgs(C.Structure):
    """include/cwm_hip.h cwm_raft_forward_ex_args (0.10.4): the frozen cwm_raft_forward_args as `base`, the warm start and the per-iteration outputs"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", CwmRaftForwardArgs),
        ("flow_init_dev", C.c_void_p),
        ("flow_init_stride_b", C.c_int64),
        ("flow_init_stride_t", C.c_int64),
        ("flow_init_stride_c", C.c_int64),
        ("flow_iters_dev", C.c_void_p),
        ("flow_iters_stride_i", C.c_int64),
        ("head_iters_dev", C.c_void_p),
        ("head_iters_stride_i", C.c_int64),
    ]


new_raft_forward_ex_args = partial(new_args, CwmRaftForwardExArgs)


class CwmDevConvSrc(C.Structure):
    _fields_ = [
        ("p", C.c_void_p),
        ("ld", C.c_int32),
        ("C", C.c_int32),
        ("stats", C.c_void_p),
        ("relu", C.c_int32),
        ("gate", C.c_void_p),
        ("gate_ld", C.c_int32),
        ("coords", C.c_void_p),
    ]


class CwmDevConvPart(C.Structure):
    _fields_ = [
        ("w", C.c_void_p),
        ("b", C.c_void_p),
        ("n", C.c_int32),
        ("bn_gamma", C.c_void_p),
        ("bn_beta", C.c_void_p),
        ("bn_mean", C.c_void_p),
        ("bn_var", C.c_void_p),
    ]


DEV_CONV_OPERAND_ONLY, DEV_CONV_KEEP_OPERAND = 1, 2


class CwmDevRaftConvArgs(C.Structure):
    """include/cwm_hip_dev.h cwm_dev_raft_conv_args (development library only)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("nsrc", C.c_int32),
        ("src", CwmDevConvSrc * 2),
        ("image", C.c_void_p * 2),
        ("image_sb", C.c_int64 * 2),
        ("image_st", C.c_int64 * 2),
        ("image_sc", C.c_int64 * 2),
        ("P", C.c_int32),
        ("ppg", C.c_int32),
        ("scale", C.c_float),
        ("img0", C.c_int32),
        ("n_img", C.c_int32),
        ("H", C.c_int32),
        ("W", C.c_int32),
        ("kh", C.c_int32),
        ("kw", C.c_int32),
        ("stride", C.c_int32),
        ("pad_h", C.c_int32),
        ("pad_w", C.c_int32),
        ("nparts", C.c_int32),
        ("part", CwmDevConvPart * 2),
        ("bn_eps", C.c_float),
        ("out", C.c_void_p),
        ("ldc", C.c_int32),
        ("col0", C.c_int32),
        ("mode", C.c_int32),
        ("c_lo", C.c_int32),
        ("c_hi", C.c_int32),
        ("A", C.c_void_p),
        ("flags", C.c_int32),
        ("stream", C.c_void_p),
    ]


DEV_GATHER_PATCH, DEV_GATHER_INDEX, DEV_GATHER_FLOW_RGB, DEV_GATHER_IMU, DEV_GATHER_INDEX_UNFUSED = range(5)


class CwmDevGatherArgs(C.Structure):
    """include/cwm_hip_dev.h cwm_dev_gather_args (development library only)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("kind", C.c_int32),
        ("mode", C.c_int32),
        ("normalize", C.c_int32),
        ("x", C.c_void_p),
        ("sb", C.c_int64),
        ("sc", C.c_int64),
        ("st", C.c_int64),
        ("fwd", C.c_void_p),
        ("bwd", C.c_void_p),
        ("f_sb", C.c_int64),
        ("f_sc", C.c_int64),
        ("b_sb", C.c_int64),
        ("b_sc", C.c_int64),
        ("B", C.c_int32),
        ("C", C.c_int32),
        ("H", C.c_int32),
        ("W", C.c_int32),
        ("P", C.c_int32),
        ("L", C.c_int32),
        ("tubelet", C.c_int32),
        ("Nt", C.c_int32),
        ("n_rows", C.c_int32),
        ("perm_stride", C.c_int32),
        ("n_vis", C.c_int32),
        ("mask", C.c_void_p),
        ("perm", C.c_void_p),
        ("rank", C.c_void_p),
        ("err_rows", C.c_void_p),
        ("out", C.c_void_p),
        ("ld", C.c_int32),
        ("stream", C.c_void_p),
    ]


new_dev_gather_args = partial(new_args, CwmDevGatherArgs)


DEV_CONJ_VALU, DEV_CONJ_MFMA = 0, 1
DEV_CONJ_PAD_MASK, DEV_CONJ_FIX_PAD_ROWS, DEV_CONJ_ZERO_PAD_OUT_ROWS, DEV_CONJ_IMU_APPEND_DUMMY = range(4)


class CwmDevConjCrossAttentionArgs(C.Structure):
    """include/cwm_hip_dev.h cwm_dev_conj_cross_attention_args (development library only)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mode", C.c_int32),
        ("impl", C.c_int32),
        ("roles", C.c_int32),
        ("qk", C.c_void_p),
        ("v", C.c_void_p),
        ("qk_src", C.c_void_p),
        ("v_src", C.c_void_p),
        ("B", C.c_int32),
        ("N", C.c_int32),
        ("M", C.c_int32),
        ("heads", C.c_int32),
        ("head_dim", C.c_int32),
        ("scale", C.c_float),
        ("y", C.c_void_p),
        ("y_src", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class CwmDevConjSmallAttentionArgs(C.Structure):
    """include/cwm_hip_dev.h cwm_dev_conj_small_attention_args (development library only)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mode", C.c_int32),
        ("impl", C.c_int32),
        ("qkv", C.c_void_p),
        ("B", C.c_int32),
        ("n_tok", C.c_int32),
        ("heads", C.c_int32),
        ("head_dim", C.c_int32),
        ("o", C.c_void_p),
        ("ldo", C.c_int32),
        ("stream", C.c_void_p),
    ]


class CwmDevConjPadArgs(C.Structure):
    """include/cwm_hip_dev.h cwm_dev_conj_pad_args (development library only)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("kind", C.c_int32),
        ("B", C.c_int32),
        ("mask", C.c_void_p),
        ("N", C.c_int32),
        ("P", C.c_int32),
        ("vmax", C.c_int32),
        ("ext_mask", C.c_void_p),
        ("x", C.c_void_p),
        ("perm", C.c_void_p),
        ("perm_stride", C.c_int32),
        ("n_rows", C.c_int32),
        ("n_vis", C.c_int32),
        ("n_real", C.c_int32),
        ("D", C.c_int32),
        ("token", C.c_void_p),
        ("imu", C.c_void_p),
        ("dummy", C.c_void_p),
        ("C", C.c_int32),
        ("L", C.c_int32),
        ("T", C.c_int32),
        ("out", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class CwmDevGemmArgs(C.Structure):
    """include/cwm_hip_dev.h cwm_dev_gemm_args (development library only)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mode", C.c_int32),
        ("epi", C.c_int32),
        ("a", C.c_void_p),
        ("w", C.c_void_p),
        ("bias", C.c_void_p),
        ("M", C.c_int32),
        ("N", C.c_int32),
        ("K", C.c_int32),
        ("rows_in", C.c_int32),
        ("rows_out", C.c_int32),
        ("out_row_offset", C.c_int32),
        ("map_stride", C.c_int32),
        ("resid_rowmap", C.c_void_p),
        ("C", C.c_void_p),
        ("ldc", C.c_int32),
        ("resid", C.c_void_p),
        ("ldr", C.c_int32),
        ("out", C.c_void_p),
        ("ldo", C.c_int32),
        ("q_out", C.c_void_p),
        ("k_out", C.c_void_p),
        ("v_out", C.c_void_p),
        ("qk_plane", C.c_int64),
        ("heads", C.c_int32),
        ("head_dim", C.c_int32),
        ("n_tok", C.c_int32),
        ("q_scale", C.c_float),
        ("plan_forms", C.POINTER(C.c_int32)),
        ("stream", C.c_void_p),
    ]


class CwmDevAttentionArgs(C.Structure):
    """include/cwm_hip_dev.h cwm_dev_attention_args (development library only)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mode", C.c_int32),
        ("qkv", C.c_void_p),
        ("B", C.c_int32),
        ("N", C.c_int32),
        ("H", C.c_int32),
        ("q_off", C.c_int32),
        ("n_q", C.c_int32),
        ("o", C.c_void_p),
        ("ldo", C.c_int32),
        ("stream", C.c_void_p),
    ]


class CwmDevLayernormArgs(C.Structure):
    """include/cwm_hip_dev.h cwm_dev_layernorm_args (development library only)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mode", C.c_int32),
        ("x", C.c_void_p),
        ("ldx", C.c_int32),
        ("gamma", C.c_void_p),
        ("beta", C.c_void_p),
        ("eps", C.c_float),
        ("D", C.c_int32),
        ("rows", C.c_int32),
        ("rows_out_per_b", C.c_int32),
        ("rows_in_per_b", C.c_int32),
        ("in_offset", C.c_int32),
        ("out", C.c_void_p),
        ("ldo", C.c_int32),
        ("out_f32", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class CwmDevGemmPlanPart(C.Structure):
    _fields_ = [("m_offset", C.c_int32), ("M", C.c_int32), ("kernel", C.c_int32), ("splitk", C.c_int32)]


class CwmDevGemmPlanOut(C.Structure):
    """include/cwm_hip_dev.h cwm_dev_gemm_plan_out (development library only)"""
    _fields_ = [("cfg", C.c_int32), ("nparts", C.c_int32), ("part", CwmDevGemmPlanPart * 2)]


DEV_GEMM_KERNEL_128, DEV_GEMM_KERNEL_DEEP128, DEV_GEMM_KERNEL_DEEP64, DEV_GEMM_KERNEL_8PHASE = range(4)


class CwmDevFlowFormsOut(C.Structure):
    """include/cwm_hip_dev.h cwm_dev_flow_forms_out (development library only): the kernel form per entry point, DEV_FLOW_* below"""
    _fields_ = [(n, C.c_int32) for n in ("features", "motion", "count", "finish", "zero", "pack")]


DEV_FLOW_REFUSED = -1
DEV_FLOW_FEATURES_SCALAR, DEV_FLOW_FEATURES_VEC4 = range(2)
DEV_FLOW_MOTION_STRIDED, DEV_FLOW_MOTION_TILE, DEV_FLOW_MOTION_ROWS16, DEV_FLOW_MOTION_ROWS32, DEV_FLOW_MOTION_ROWS64 = range(5)
DEV_FLOW_COUNT_PLANES, DEV_FLOW_COUNT_PLANES_VEC, DEV_FLOW_COUNT_PACKED, DEV_FLOW_COUNT_PACKED_VEC = range(4)
DEV_FLOW_FINISH_V1, DEV_FLOW_FINISH_V4 = range(2)
DEV_FLOW_ZERO_PLANES, DEV_FLOW_ZERO_PLANES_VEC, DEV_FLOW_ZERO_SCATTER = range(3)
DEV_FLOW_PACK_TRANSPOSE = 0


new_dev_conj_args = new_args  # (a cwm_dev_*_args of the given structure class: conj, gemm, attention, layernorm)
new_dev_raft_conv_args = partial(new_args, CwmDevRaftConvArgs)
new_forward_args = partial(new_args, CwmForwardArgs)
new_patch_error_args = partial(new_args, CwmPatchErrorArgs)
new_token_response_args = partial(new_args, CwmTokenResponseArgs)
new_unmask_step_args = partial(new_args, CwmUnmaskStepArgs)


def new_segment_step_args() -> CwmSegmentStepArgs:
    a = new_args(CwmSegmentStepArgs)
    a.base.T = 2
    return a


def new_segment_merge_args() -> CwmSegmentMergeArgs:
    a = new_args(CwmSegmentMergeArgs)
    a.base.T = 2
    return a


def new_seed_select_args() -> CwmSeedSelectArgs:
    a = new_args(CwmSeedSelectArgs)
    a.base.T = 1
    return a


def new_segment_track_args() -> CwmSegmentTrackArgs:
    a = new_args(CwmSegmentTrackArgs)
    a.base.T = 1
    return a


def new_flow_consistency_args() -> CwmFlowConsistencyArgs:
    a = new_args(CwmFlowConsistencyArgs)
    a.base.T = 1
    return a


def new_object_motion_args() -> CwmObjectMotionArgs:
    a = new_args(CwmObjectMotionArgs)
    a.base.T = 1
    return a


def new_point_track_args() -> CwmPointTrackArgs:
    a = new_args(CwmPointTrackArgs)
    a.base.T = 2
    a.alpha, a.beta, a.max_coast = 0.01, 0.5, 8
    return a


def new_object_response_args() -> CwmObjectResponseArgs:
    a = new_args(CwmObjectResponseArgs)
    a.base.T = 1
    return a


def new_parallax_args() -> CwmParallaxArgs:
    a = new_args(CwmParallaxArgs)
    a.base.T = 1
    a.ref_slot, a.min_pixels, a.min_ref_q, a.min_samples = -1, 1, 64, 1
    return a


def fill_patch_args(g, *, x=None, target=None, mask=None, region=None, y=None, geometry, n_vis=0, frame=-1, map=None, mean=None, scratch=None, stream):
    """Fills a cwm_patch_error_args -- alone, or the `.base` of the other read-outs' -- from tensors: the one place that knows its field order.  `x` and `target`
    are [B,T,C,H,W]-SHAPED views of any (b, t, c) strides, whatever the order of the tensor beneath ([B,C,T,H,W] permuted, a batch stride of 0); their image
    rows must be contiguous (ValueError otherwise: the kernels address a pixel as y W + x).  geometry = (B, T, C, H, W, P).  Only addresses are stored: the
    caller keeps the tensors alive until the call has been queued.  Returns g."""
    def frames(name, v):
        if v is None:
            return None, 0, 0, 0
        if v.dim() != 5 or v.stride(-1) != 1 or v.stride(-2) != v.shape[-1]:
            raise ValueError("fill_patch_args: %s must be a [B,T,C,H,W]-shaped view with contiguous image rows, got shape %s strides %s" % (
                name, tuple(v.shape), v.stride()))
        return v.data_ptr(), v.stride(0), v.stride(1), v.stride(2)

    g.x_dev, g.x_stride_b, g.x_stride_t, g.x_stride_c = frames("x", x)
    g.target_dev, g.target_stride_b, g.target_stride_t, g.target_stride_c = frames("target", target)
    g.y_tokens_dev, g.mask_dev, g.region_dev = ptr(y), ptr(mask), ptr(region)
    g.batch, g.T, g.C, g.H, g.W, g.P = geometry
    g.n_vis, g.frame = n_vis, frame
    g.map_dev, g.mean_dev, g.scratch_dev, g.stream = ptr(map), ptr(mean), ptr(scratch), stream
    return g


new_conj_forward_args = partial(new_args, CwmConjForwardArgs)


class CwmKernelStats(C.Structure):
    _fields_ = [("launches", C.c_int64), ("total_ms", C.c_double), ("total_flops", C.c_double)]


# name -> (restype, argtypes); must list every symbol declared in include/cwm_hip.h
SIGNATURES = {
    "cwm_model_create": (C.c_int, [C.POINTER(CwmConfig), C.POINTER(C.c_void_p)]),
    "cwm_model_destroy": (None, [C.c_void_p]),
    "cwm_model_load_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "cwm_model_missing_weights": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "cwm_forward": (C.c_int, [C.c_void_p, C.POINTER(CwmForwardArgs)]),
    "cwm_model_set_lanes": (C.c_int, [C.c_void_p, C.c_int]),
    "cwm_model_set_ragged": (C.c_int, [C.c_void_p, C.c_int]),
    "cwm_model_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "cwm_conj_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "cwm_conj_create": (C.c_int, [C.POINTER(CwmConjConfig), C.POINTER(C.c_void_p)]),
    "cwm_conj_create_ex": (C.c_int, [C.POINTER(CwmConjConfig), C.POINTER(CwmConjVariant), C.POINTER(C.c_void_p)]),
    "cwm_conj_destroy": (None, [C.c_void_p]),
    "cwm_conj_load_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "cwm_conj_missing_weights": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "cwm_conj_forward": (C.c_int, [C.c_void_p, C.POINTER(CwmConjForwardArgs)]),
    "cwm_conj_set_lanes": (C.c_int, [C.c_void_p, C.c_int]),
    "cwm_conj_timing_enable": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "cwm_conj_timing_collect": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(CwmKernelStats)]),
    "cwm_timing_enable": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "cwm_timing_collect": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(CwmKernelStats)]),
    "cwm_split_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cwm_linear": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    ),
    "cwm_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cwm_attention_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cwm_layernorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "cwm_mask_to_perm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cwm_unembed": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    ),
    "cwm_patch_error": (C.c_int, [C.POINTER(CwmPatchErrorArgs)]),
    "cwm_token_response": (C.c_int, [C.POINTER(CwmTokenResponseArgs)]),
    "cwm_unmask_step": (C.c_int, [C.POINTER(CwmUnmaskStepArgs)]),
    "cwm_segment_step": (C.c_int, [C.POINTER(CwmSegmentStepArgs)]),
    "cwm_segment_merge": (C.c_int, [C.POINTER(CwmSegmentMergeArgs)]),
    "cwm_segment_merge_work_bytes": (C.c_size_t, [C.c_int] * 4),
    "cwm_seed_select": (C.c_int, [C.POINTER(CwmSeedSelectArgs)]),
    "cwm_seed_select_work_bytes": (C.c_size_t, [C.c_int] * 4),
    "cwm_segment_track": (C.c_int, [C.POINTER(CwmSegmentTrackArgs)]),
    "cwm_segment_track_work_bytes": (C.c_size_t, [C.c_int] * 3),
    "cwm_flow_consistency": (C.c_int, [C.POINTER(CwmFlowConsistencyArgs)]),
    "cwm_object_motion": (C.c_int, [C.POINTER(CwmObjectMotionArgs)]),
    "cwm_point_track": (C.c_int, [C.POINTER(CwmPointTrackArgs)]),
    "cwm_object_response": (C.c_int, [C.POINTER(CwmObjectResponseArgs)]),
    "cwm_parallax": (C.c_int, [C.POINTER(CwmParallaxArgs)]),
    "cwm_mask_row_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cwm_mask_flip_picks": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "cwm_prompt_table_expand": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4),
    "cwm_shift_prompts": (
        C.c_int,
        [C.c_void_p] + [C.c_int] * 9 + [C.c_void_p] * 6,
    ),
    "cwm_multi_shift_prompts": (
        C.c_int,
        [C.c_void_p] + [C.c_int] * 10 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3,
    ),
    "cwm_flow_features": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]),
    "cwm_flow_cov": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4),
    "cwm_flow_transform_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "cwm_flow_transform": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "cwm_flow_motion_work_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "cwm_flow_motion_sum": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)] + [C.c_int] * 6 + [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cwm_flow_map_finish": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_void_p]),
    "cwm_flow_filter_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)] + [C.c_int] * 5 + [C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_int] + [C.c_float] * 3
                              + [C.c_void_p] * 5),
    "cwm_flow_filter_apply": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "cwm_flow_filter_pack": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cwm_comm_load": (C.c_int, [C.c_char_p]),
    "cwm_comm_version": (C.c_int, []),
    "cwm_comm_unique_id": (C.c_int, [C.c_void_p]),
    "cwm_comm_init": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "cwm_comm_destroy": (None, [C.c_void_p]),
    "cwm_comm_rank": (C.c_int, [C.c_void_p]),
    "cwm_comm_size": (C.c_int, [C.c_void_p]),
    "cwm_broadcast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "cwm_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cwm_allgatherv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p]),
    "cwm_allreduce_sum_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cwm_raft_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "cwm_raft_destroy": (None, [C.c_void_p]),
    "cwm_raft_load_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "cwm_raft_missing_weights": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "cwm_raft_forward": (C.c_int, [C.c_void_p, C.POINTER(CwmRaftForwardArgs)]),
    "cwm_raft_forward_ex": (C.c_int, [C.c_void_p, C.POINTER(CwmRaftForwardExArgs)]),
    "cwm_raft_corr_lookup": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cwm_raft_set_corr": (C.c_int, [C.c_void_p, C.c_int]),
    "cwm_raft_workspace_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cwm_raft_set_share_frames": (C.c_int, [C.c_void_p, C.c_int]),
    "cwm_raft_encoder_images": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cwm_raft_corr_lookup_on_the_fly": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cwm_raft_convex_upsample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cwm_raft_head_project": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "cwm_raft_convex_upsample1": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cwm_raft_forward_interpolate": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cwm_last_error": (C.c_char_p, []),
    "cwm_version": (C.c_char_p, []),
    "cwm_source_hash": (C.c_char_p, []),
    "cwm_compiler_version": (C.c_char_p, []),
}
# ... and every symbol of include/cwm_hip_dev.h: only libcwm_hip_dev.so (get_dev_lib) has these
DEV_SIGNATURES = {
    "cwm_gemm_tile_override": (C.c_int, [C.c_int] * 6),
    "cwm_dev_gemm_plan": (C.c_int, [C.c_int] * 8 + [C.POINTER(CwmDevGemmPlanOut)]),
    "cwm_dev_flow_forms": (C.c_int, [C.POINTER(C.c_int64)] + [C.c_int] * 5 + [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_int64), C.c_uint64, C.c_int, C.POINTER(CwmDevFlowFormsOut)]),
    "cwm_bench_gemm": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "cwm_bench_attention": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "cwm_debug_set": (C.c_int, [C.c_char_p, C.c_int]),
    "cwm_debug_get": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "cwm_dev_raft_conv": (C.c_int, [C.POINTER(CwmDevRaftConvArgs)]),
    "cwm_dev_raft_corr_lookup_operand": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cwm_dev_raft_corr_lookup_on_the_fly_operand": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cwm_dev_raft_instnorm_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "cwm_dev_raft_residual_join": (C.c_int, [C.POINTER(CwmDevConvSrc), C.POINTER(CwmDevConvSrc), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cwm_dev_raft_cnet_split": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cwm_dev_raft_frame_slots": (C.c_int, [C.POINTER(CwmRaftForwardArgs), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                           C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cwm_dev_raft_corr_lookup_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                                 C.c_void_p, C.c_void_p]),
    "cwm_dev_raft_fmap_pool_slots": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cwm_dev_raft_corr_lookup_on_the_fly_slots": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                                            C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "cwm_dev_raft_cnet_split_slots": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cwm_dev_raft_motion_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "cwm_dev_raft_gru_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "cwm_dev_raft_flow_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]),
    "cwm_dev_gather": (C.c_int, [C.POINTER(CwmDevGatherArgs)]),
    "cwm_dev_conj_cross_attention": (C.c_int, [C.POINTER(CwmDevConjCrossAttentionArgs)]),
    "cwm_dev_conj_small_attention": (C.c_int, [C.POINTER(CwmDevConjSmallAttentionArgs)]),
    "cwm_dev_conj_pad": (C.c_int, [C.POINTER(CwmDevConjPadArgs)]),
    "cwm_dev_gemm": (C.c_int, [C.POINTER(CwmDevGemmArgs)]),
    "cwm_dev_attention": (C.c_int, [C.POINTER(CwmDevAttentionArgs)]),
    "cwm_dev_layernorm": (C.c_int, [C.POINTER(CwmDevLayernormArgs)]),
    "cwm_dev_fill_mask_tokens": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]),
    "cwm_dev_unembed": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int64] * 3 + [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p]),
    # the launch forms of a ragged batch (tests/test_ragged_kernels_gpu.py)
    "cwm_dev_gather_ragged": (C.c_int, [C.POINTER(CwmDevGatherArgs), C.c_int, C.c_void_p]),
    "cwm_dev_attention_ragged": (C.c_int, [C.POINTER(CwmDevAttentionArgs), C.c_void_p]),
    "cwm_dev_fill_mask_tokens_ragged": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "cwm_dev_unembed_ragged": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int64] * 3 + [C.c_void_p] + [C.c_int] * 8 + [C.c_void_p, C.c_void_p]),
}

# the keys cwm_model_set_option / cwm_conj_set_option know (include/cwm_hip.h; csrc/engine.hip tuning_field)
OPTION_KEYS = ("gemm_tile", "gemm_debug", "gemm_staged", "gemm_direct", "attn_kernel", "attn_remap", "attn_tail", "attn_ksplit", "prune_last_block", "mask_token_tables","index_fused",
               "min_lane_rows", "conj_ctx_stream", "conj_attn")
GEMM_DEBUG_TIMING_ONLY = 1 | 2 | 8  # ablation bits that make a forward return wrong outputs: refused by the production setters (development library: cwm_debug_set)


def validate_option(key: str, value: int) -> None:
    """What the library's setters would refuse, raised BEFORE a model stores the option for a handle it does not have yet (a bad key remembered there
    would fail every later handle creation with an unrelated-looking error)."""
    if key not in OPTION_KEYS:
        raise CwmHipError(-1, "unknown option %s (known: %s)" % (key, ", ".join(OPTION_KEYS)))
    if key == "gemm_debug" and int(value) & GEMM_DEBUG_TIMING_ONLY:
        raise CwmHipError(-1, "gemm_debug bits 1, 2 and 8 are timing-only ablations (wrong outputs): development library only (cwm_debug_set)")


_lib: Optional[C.CDLL] = None
_dev_lib: Optional[C.CDLL] = None
_lock = threading.Lock()


class CwmHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


def library_path() -> str:
    return os.environ.get("CWM_HIP_LIB", _build.LIB_PATH)


def get_lib() -> C.CDLL:
    """Load (building if absent and hipcc is available) libcwm_hip.so.  Raises if impossible."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not os.path.exists(path):
            try:
                _build.build_library()
            except Exception as e:  # no silent fallback
                raise RuntimeError(
                    "libcwm_hip.so is missing at %s and could not be built (%s). "
                    "Run `python -m counterfactualworldmodels_amd.build`." % (path, e)
                )
        lib = _bind(path)
        if path == _build.LIB_PATH and os.path.isdir(_build.CSRC):
            # a stale in-tree library (sources changed after it was built) is rebuilt, never silently bound
            want = _build.source_hash()
            if lib.cwm_source_hash().decode() != want:
                try:
                    _build.build_library(force=False)
                except Exception as e:
                    raise RuntimeError("libcwm_hip.so at %s was built from other sources (%s != %s) and could not be rebuilt: %s"
                                       % (path, lib.cwm_source_hash().decode(), want, e))
                # the dynamic loader returns the already-mapped object for a path it knows: unmap the stale library first (nothing was
                # created through it yet), then map the rebuilt file
                import _ctypes

                _ctypes.dlclose(lib._handle)
                lib = _bind(path)
                if lib.cwm_source_hash().decode() != want:
                    raise RuntimeError("libcwm_hip.so still does not match the sources after a rebuild")
        _warn_if_unlinted_compiler(lib)
        _lib = lib
        return lib


def _warn_if_unlinted_compiler(lib) -> None:
    """The kernels carry hand-counted `s_waitcnt` instructions that are only as right as the ISA the compiler emitted around them (tools/asm_lds_lint.py);
    a library compiled by another hipcc than the one the lint last passed on (csrc/LINT_PASSED.json) says so once, at load time."""
    try:
        rec = _build.lint_record().get("hipcc")
        comp = lib.cwm_compiler_version().decode()
    except Exception:  # a library from before the entry point existed / no record in an installed copy
        return
    if rec and comp and rec != comp:
        import warnings

        warnings.warn("libcwm_hip.so was compiled by `%s`, but the ISA lint of its hand-counted waits last passed on `%s`: run `python tools/asm_lds_lint.py --record` "
                      "(and the GPU soak, tests/test_soak_gpu.py) before trusting this build" % (comp, rec), RuntimeWarning, stacklevel=3)


def dev_library_path() -> str:
    p = library_path()
    return os.environ.get("CWM_HIP_DEV_LIB", _build.DEV_LIB_PATH if p == _build.LIB_PATH else p[:-3] + "_dev.so")


def get_dev_lib() -> C.CDLL:
    """The development library (libcwm_hip_dev.so: the production objects + csrc/dev.hip; include/cwm_hip_dev.h) -- for tools/ and for the tests that
    cross-check kernel variants.  A SEPARATE shared object with its own state: handles created through it are its own; `cwm_debug_set` acts on the
    calling thread's options inside it and never on the production library."""
    global _dev_lib
    if _dev_lib is not None:
        return _dev_lib
    get_lib()  # builds / rebuilds both libraries if the sources changed
    with _lock:
        if _dev_lib is None:
            path = dev_library_path()
            if not os.path.exists(path):
                raise RuntimeError("libcwm_hip_dev.so is missing at %s: run `python -m counterfactualworldmodels_amd.build`" % path)
            lib = _bind(path, dict(SIGNATURES, **DEV_SIGNATURES))
            if path == _build.DEV_LIB_PATH and os.path.isdir(_build.CSRC) and lib.cwm_source_hash().decode() != _build.source_hash():
                raise RuntimeError("libcwm_hip_dev.so at %s was built from other sources than the tree holds: run `python -m counterfactualworldmodels_amd.build`" % path)
            _dev_lib = lib
    return _dev_lib


def _bind(path: str, signatures=None) -> C.CDLL:
    lib = C.CDLL(path)
    for name, (res, args) in (signatures or SIGNATURES).items():
        try:
            fn = getattr(lib, name)  # a missing symbol fails loudly
        except AttributeError:
            if name == "cwm_source_hash":  # a library from before the hash existed: report it as stale
                lib.cwm_source_hash = lambda: b"pre-hash"
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    return lib


def check(rc: int, lib: Optional[C.CDLL] = None) -> None:
    """Raise for a negative return code; `lib` = the library the call went through (default: the production one; a call through the development
    library that fails leaves its message there -- the thread-local error text is per shared object)."""
    if rc != 0:
        msg = (lib or get_lib()).cwm_last_error()
        if not msg and lib is None and _dev_lib is not None:
            msg = _dev_lib.cwm_last_error()
        raise CwmHipError(rc, (msg.decode() if msg else "") + " [cwm_hip rc=%d]" % rc)


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise RuntimeError(
            "counterfactualworldmodels_amd runs its predictor on an AMD GPU through libcwm_hip.so; "
            "no HIP device is visible and there is no CPU fallback."
        )


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def current_stream_handle(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream
