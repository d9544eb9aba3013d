"""ctypes binding of libcenterpose_hip.so (C ABI: include/centerpose_hip.h).

PyTorch-ROCm is only the tensor container / allocator / stream provider here: every call hands raw
``data_ptr()`` device pointers and the current HIP stream to the library.  There is NO fallback:
if the shared library is missing or a call fails, a ``RuntimeError`` is raised.
"""
import contextlib
import ctypes
import enum
import os
from collections import OrderedDict
from collections.abc import Mapping

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# $CENTERPOSE_HIP_LIB selects another build of the same ABI (tuning variants: make -C csrc EXP=n)
LIB_PATH = os.environ.get("CENTERPOSE_HIP_LIB") or os.path.join(_HERE, "libcenterpose_hip.so")

_lib = None
ABI_VERSION = 7  # CP_ABI_VERSION of include/centerpose_hip.h this binding was written against

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_size_t = ctypes.c_size_t
c_char_p = ctypes.c_char_p


class TrackParams(ctypes.Structure):
    """cp_track_params of include/centerpose_hip.h (field for field)."""
    _fields_ = [(n, ctypes.c_double) for n in ("new_thresh", "pre_thresh", "R", "conf_lo", "conf_hi")] + \
               [(n, ctypes.c_int) for n in ("max_age", "kalman", "scale_pool", "use_pnp", "hps_uncertainty", "show_axes",
                                            "cat_rule", "render_hm_mode", "render_hmhp_mode", "pre_hm", "pre_hm_hp", "K",
                                            "cap", "hungarian", "baseline")]


# ---- ObjectPoseLoss (cp_pose_loss_*): names in the order of the CP_PL_H_* / CP_PL_T_* constants ----
POSE_LOSS_MAX_STACKS = 4
POSE_LOSS_HEADS = ("hm", "hm_hp", "hps", "hps_uncertainty", "wh", "reg", "scale", "scale_uncertainty", "hp_offset",
                   "tracking", "tracking_hp")
POSE_LOSS_TERMS = ("hm", "wh", "off", "hp", "hm_hp", "hp_offset", "obj_scale", "tracking", "tracking_hp")
POSE_LOSS_STATS = ("loss", "hm_loss", "hp_loss", "hm_hp_loss", "hp_offset_loss", "wh_loss", "off_loss", "obj_scale_loss",
                   "tracking_loss", "tracking_hp_loss")
PL_VAL, PL_RESIDUAL, PL_HPS_UNCERTAINTY, PL_SCALE_UNCERTAINTY, PL_HM_HP_MAPS = 1, 2, 4, 8, 16
_PL_GT = ("gt_hm", "gt_hm_hp", "ind", "reg_mask", "gt_hps", "hps_mask", "gt_wh", "gt_reg", "gt_scale", "hp_ind", "hp_mask",
          "gt_hp_offset", "gt_tracking", "tracking_mask", "gt_tracking_hp", "tracking_hp_mask")


class PoseLossDesc(ctypes.Structure):
    """cp_pose_loss_desc of include/centerpose_hip.h (field for field)."""
    _fields_ = [(n, c_int) for n in ("B", "S", "K", "H", "W", "num_classes", "num_joints", "num_stacks", "terms", "flags")] + \
               [("weight", ctypes.c_float * 9), ("kl_kps", ctypes.c_float), ("kl_scale", ctypes.c_float),
                ("dimension_ref", ctypes.c_float * 3)] + [(n, c_void_p) for n in _PL_GT] + \
               [("head", (c_void_p * len(POSE_LOSS_HEADS)) * POSE_LOSS_MAX_STACKS),
                ("clamped", (c_void_p * 2) * POSE_LOSS_MAX_STACKS)]


# ---- ObjectPose training targets (cp_pose_targets*): record layouts of include/centerpose_hip.h ----
CP_ERR_INVALID = -1
PT_MAX_OBJS = 64
PT_IMG_STRIDE, PT_OBJ_STRIDE = 32, 64
PT_IMG = dict(trans=0, width=6, height=7, flipped=8, rot=9, num_objs=10, proj=11)
PT_OBJ = dict(nsym=0, cuboid=1, quat=19, loc=23, kps3d=26, scale=53)
PT_FLAGS = ("center_3D", "use_absolute_scale", "obj_scale", "hps_uncertainty", "reg_hp_offset", "hm_hp")
PT_OUTPUTS = ("hm", "hm_hp", "reg_mask", "ind", "hps", "hps_mask", "hps_uncertainty", "wh", "reg", "scale",
              "scale_uncertainty", "hp_offset", "hp_ind", "hp_mask")


class PoseTargetsDesc(ctypes.Structure):
    """cp_pose_targets_desc of include/centerpose_hip.h (field for field)."""
    _fields_ = [(n, c_int) for n in ("B", "S", "R", "max_objs", "num_joints") + PT_FLAGS] + \
               [("images", c_void_p), ("objects", c_void_p)] + [("out_" + n, c_void_p) for n in PT_OUTPUTS]


# ---- the tracking task's targets (cp_pose_targets_track*): record layouts of include/centerpose_hip.h ----
PTK_IMG_STRIDE, PTK_PRE_STRIDE, PTK_CUR_STRIDE = 32, 128, 2
PTK_IMG = dict(trans=0, num_pre=6, proj=7)
PTK_PRE = dict(skip=56, idsym=57, id=58, draws=64)  # 0..52: PT_OBJ's nsym, cuboid, quat, loc, kps3d
PTK_DRAW = dict(ct_noise=0, ct_lost=2, ct_heat=3, ct_fp=4, ct_fp_noise=5, ct_fp_peak=7, joints=8, joint_stride=7,
                j_noise=0, j_lost=2, j_fp=3, j_fp_noise=4, j_fp_peak=6)
PTK_NUM_DRAWS = 64
PTK_CUR = dict(id=0, skip=1)
PTK_GEOMETRY = ("input_w", "input_h", "down_ratio", "max_pre_objs")
PTK_FLAGS = ("hm_heat_random", "hm_hp_heat_random", "tracking_label_mode", "pre_hm", "pre_hm_hp", "tracking", "tracking_hp")
PTK_DISTURB = ("hm_disturb", "lost_disturb", "fp_disturb", "hm_hp_disturb", "hp_lost_disturb", "hp_fp_disturb")
PTK_OUTPUTS = ("pre_hm", "pre_hm_hp", "tracking", "tracking_mask", "tracking_hp", "tracking_hp_mask")


class PoseTargetsTrackDesc(ctypes.Structure):
    """cp_pose_targets_track_desc of include/centerpose_hip.h (field for field)."""
    _fields_ = [("cur", PoseTargetsDesc)] + [(n, c_int) for n in PTK_GEOMETRY + PTK_FLAGS + ("reserved",)] + \
               [(n, ctypes.c_double) for n in PTK_DISTURB] + \
               [(n, c_void_p) for n in ("track_images", "pre_objects", "cur_objects")] + \
               [("out_" + n, c_void_p) for n in PTK_OUTPUTS]


# ---- the same with a detector's boxes (cp_pose_targets_track_det): the host record per image, the render options ----
PTK_GEN_STRIDE = 4
PTK_GEN = dict(mode=0, radius_scale=1)
PTK_DET_MAX_K = 128
PTK_DET_OPTS = ("K_det", "render_hm_mode", "render_hmhp_mode", "cat_rule")
PTK_CAT_RULE = {"camera": 0, "bottle": 0, "cup": 0, "book": 1, "chair": 1, "cereal_box": 1, "bike": 2, "laptop": 2, "shoe": 2}


class PoseTargetsTrackDetDesc(ctypes.Structure):
    """cp_pose_targets_track_det_desc of include/centerpose_hip.h (field for field)."""
    _fields_ = [("track", PoseTargetsTrackDesc)] + [(n, c_void_p) for n in ("det_post", "det_count", "det_pnp")] + \
               [(n, c_int) for n in PTK_DET_OPTS] + [("gen", c_void_p)]


# ---- training input images (cp_train_inputs): record layout of include/centerpose_hip.h ----
TI_STRIDE = 24
TI_IMG = dict(offset=0, height=1, width=2, trans=3, flipped=9, color=10, order=11, alpha=12, shift=15)
TI_ORDERS = ("bcs", "bsc", "cbs", "csb", "sbc", "scb")  # order code -> brightness / contrast / saturation as run


def _sig(fn, restype, *argtypes):
    fn.restype = restype
    fn.argtypes = list(argtypes)


def lib():
    """Load (once) and return the C-ABI library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "centerpose_amd: %s not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C centerpose_amd/csrc`).  There is no CPU fallback." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    # the ABI guard comes before any other symbol is bound: a stale library is exactly the case it exists for, and it must
    # fail with "rebuild", not with ctypes' "undefined symbol"
    if not hasattr(L, "cp_abi_version"):
        raise RuntimeError("centerpose_amd: %s predates the ABI guard (no cp_abi_version): rebuild the library" % LIB_PATH)
    _sig(L.cp_abi_version, c_int)
    if L.cp_abi_version() != ABI_VERSION:
        raise RuntimeError("centerpose_amd: %s has ABI version %d, this binding was written for %d (rebuild the library)"
                           % (LIB_PATH, L.cp_abi_version(), ABI_VERSION))
    _sig(L.cp_version, c_char_p)
    _sig(L.cp_last_error, c_char_p)
    _sig(L.cp_num_kernel_variants, c_int)
    _sig(L.cp_num_roles, c_int)
    _sig(L.cp_dcnv2_workspace_bytes, c_size_t, c_int, c_int, c_int, c_int, c_int)
    _sig(L.cp_dcnv2_forward, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         *([c_int] * 14), c_void_p, c_size_t)
    _sig(L.cp_dcnv2_backward_workspace_bytes, c_size_t, *([c_int] * 14))
    _sig(L.cp_dcnv2_backward, c_int, *([c_void_p] * 11), *([c_int] * 14), c_void_p, c_size_t)
    _sig(L.cp_dcnv2_backward_det_workspace_bytes, c_size_t, *([c_int] * 14))
    _sig(L.cp_dcnv2_backward_det, c_int, *([c_void_p] * 11), *([c_int] * 14), c_void_p, c_size_t)
    _sig(L.cp_pose_heads_chunk_images, c_int, c_int, c_int, c_int, c_int)
    _sig(L.cp_pose_heads_forward_workspace_bytes, c_size_t, *([c_int] * 6), ctypes.POINTER(c_int))
    _sig(L.cp_pose_heads_backward_workspace_bytes, c_size_t, *([c_int] * 6), ctypes.POINTER(c_int))
    _sig(L.cp_pose_heads_forward, c_int, c_void_p, c_void_p, c_int, *([ctypes.POINTER(c_void_p)] * 4), ctypes.POINTER(c_int),
         ctypes.POINTER(c_void_p), *([c_int] * 5), c_void_p, c_size_t)
    _sig(L.cp_pose_heads_backward, c_int, c_void_p, c_void_p, c_int, *([ctypes.POINTER(c_void_p)] * 4), ctypes.POINTER(c_int),
         *([ctypes.POINTER(c_void_p)] * 5), c_void_p, *([c_int] * 5), c_void_p, c_size_t)
    _sig(L.cp_model_features, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_size_t)
    _sig(L.cp_model_create, c_int, c_char_p, c_int, c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_int), c_int,
         ctypes.POINTER(c_void_p))
    _sig(L.cp_model_set_param, c_int, c_void_p, c_char_p, c_void_p, ctypes.c_int64)
    _sig(L.cp_model_finalize, c_int, c_void_p)
    _sig(L.cp_model_destroy, None, c_void_p)
    _sig(L.cp_model_workspace_bytes, c_size_t, c_void_p, c_int, c_int, c_int)
    _sig(L.cp_model_workspace_used, c_size_t, c_void_p)
    _sig(L.cp_model_maxpool_launches, c_int, c_void_p)
    _sig(L.cp_model_forward, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
         ctypes.POINTER(c_void_p), c_int, c_void_p, c_size_t)
    _sig(L.cp_model_forward_tap, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
         c_void_p, ctypes.POINTER(c_void_p), c_int, c_void_p, c_size_t, c_char_p, c_void_p, ctypes.POINTER(c_int))
    _sig(L.cp_conv2d_workspace_bytes, c_size_t, c_int, c_int, c_int, c_int)
    _sig(L.cp_conv_transpose2d_workspace_bytes, c_size_t, c_int, c_int)
    _sig(L.cp_conv_transpose2d_nhwc, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t)
    _sig(L.cp_conv2d_nhwc, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         *([c_int] * 10), c_void_p, c_size_t)
    _sig(L.cp_conv2d_backward_workspace_bytes, c_size_t, *([c_int] * 10))
    _sig(L.cp_conv2d_backward_nhwc, c_int, *([c_void_p] * 8), *([c_int] * 9), c_void_p, c_size_t)
    _sig(L.cp_conv2d_backward_path, c_int, *([c_int] * 9))
    _sig(L.cp_conv_transpose2d_dw_nhwc, c_int, *([c_void_p] * 5), *([c_int] * 5))
    _sig(L.cp_conv_transpose2d_backward_workspace_bytes, c_size_t, *([c_int] * 10))
    _sig(L.cp_conv_transpose2d_backward_nhwc, c_int, *([c_void_p] * 6), *([c_int] * 9), c_void_p, c_size_t)
    _sig(L.cp_batchnorm_workspace_bytes, c_size_t, *([c_int] * 4))
    _sig(L.cp_batchnorm_forward_nhwc, c_int, *([c_void_p] * 10), *([c_int] * 5), ctypes.c_float, ctypes.c_float, c_int, c_void_p,
         c_size_t)
    _sig(L.cp_batchnorm_backward_nhwc, c_int, *([c_void_p] * 11), *([c_int] * 5), c_void_p, c_size_t)
    _sig(L.cp_groupnorm_workspace_bytes, c_size_t, *([c_int] * 5))
    _sig(L.cp_groupnorm_forward_nhwc, c_int, *([c_void_p] * 7), *([c_int] * 5), ctypes.c_float, c_int, c_void_p, c_size_t)
    _sig(L.cp_groupnorm_backward_nhwc, c_int, *([c_void_p] * 10), *([c_int] * 5), c_void_p, c_size_t)
    _sig(L.cp_gru_gate_forward, c_int, *([c_void_p] * 5), c_int, c_int)
    _sig(L.cp_gru_gate_backward, c_int, *([c_void_p] * 8), c_int, c_int)
    _sig(L.cp_maxpool2d_forward_nhwc, c_int, c_void_p, c_void_p, c_void_p, *([c_int] * 7))
    _sig(L.cp_maxpool2d_backward_nhwc, c_int, c_void_p, c_void_p, c_void_p, c_void_p, *([c_int] * 7))
    _sig(L.cp_conv2d_stem_backward_workspace_bytes, c_size_t, *([c_int] * 6))
    _sig(L.cp_conv2d_stem_backward, c_int, *([c_void_p] * 7), c_size_t, *([c_int] * 6))
    _sig(L.cp_decode_workspace_bytes, c_size_t, c_int, c_int)
    _sig(L.cp_decode, c_int, c_void_p, c_int, c_int, c_int, *([c_void_p] * 11), c_int, c_int, c_int, ctypes.c_float,
         c_int, c_int, c_void_p, c_void_p, c_size_t)
    _sig(L.cp_decode_tiled_workspace_bytes, c_size_t, c_int, c_int, c_int, c_int)
    _sig(L.cp_decode_tiled, c_int, c_void_p, c_int, c_int, c_int, *([c_void_p] * 11), c_int, c_int, c_int, ctypes.c_float,
         c_int, c_int, c_void_p, c_void_p, c_size_t)
    _sig(L.cp_model_detect_workspace_bytes, c_size_t, c_void_p, c_int, c_int, c_int, c_int)
    _sig(L.cp_model_detect, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
         ctypes.POINTER(c_void_p), c_int, c_int, c_int, ctypes.c_float, c_int, c_void_p, c_void_p, c_size_t, c_int)
    _sig(L.cp_model_lean_supported, c_int, c_void_p, c_int, c_int, c_int)
    _sig(L.cp_model_detect_lean_workspace_bytes, c_size_t, c_void_p, c_int, c_int, c_int, c_int)
    _sig(L.cp_model_detect_lean, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
         ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_void_p, c_void_p, c_int, c_int, c_int, ctypes.c_float, c_int,
         c_void_p, c_void_p, c_size_t, c_int)
    _sig(L.cp_model_dense_heads, c_int, c_void_p, c_void_p, ctypes.POINTER(c_void_p))
    _sig(L.cp_model_heads_at_workspace_bytes, c_size_t, c_void_p, c_int, c_int)
    _sig(L.cp_model_heads_at, c_int, c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(c_void_p), c_void_p, c_size_t)
    _sig(L.cp_decode_peaks_workspace_bytes, c_size_t, c_int, c_int, c_int, c_int)
    _sig(L.cp_decode_peaks, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
         c_void_p, c_size_t)
    _sig(L.cp_decode_gathered, c_int, c_void_p, c_int, c_int, c_int, *([c_void_p] * 12), c_int, c_int, c_int, ctypes.c_float,
         c_int, c_void_p)
    _sig(L.cp_set_default_precision, c_int, c_int)
    _sig(L.cp_set_debug, c_int, c_int)
    _sig(L.cp_render_gaussians, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int)
    _sig(L.cp_postprocess_workspace_bytes, c_size_t, c_int, c_int)
    _sig(L.cp_postprocess, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, ctypes.c_double, c_int, ctypes.c_float,
         c_void_p, c_void_p, c_void_p, c_size_t)
    _sig(L.cp_preprocess, c_int, c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(ctypes.c_double),
         ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), c_void_p, c_int, c_int)
    _sig(L.cp_preprocess_batch, c_int, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_double),
         ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), c_void_p, c_int, c_int)
    _sig(L.cp_resize_u8, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int)
    _sig(L.cp_model_set_precision, c_int, c_void_p, c_int)
    _sig(L.cp_model_profile, c_int, c_void_p, c_int)
    _sig(L.cp_model_profile_read, c_int, c_void_p, ctypes.POINTER(ctypes.c_double), c_int)
    _sig(L.cp_kernel_variant_name, c_char_p, c_int)
    _sig(L.cp_model_profile_roles, c_int, c_void_p, ctypes.POINTER(ctypes.c_double), c_int)
    _sig(L.cp_role_name, c_char_p, c_int)
    _sig(L.cp_pnp_workspace_bytes, c_size_t, c_int)
    _sig(L.cp_pnp_from_post_workspace_bytes, c_size_t, c_int, c_int)
    _sig(L.cp_pnp_from_post, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t)
    _sig(L.cp_pnp_solve, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t)
    _sig(L.cp_track_state_bytes, c_size_t, c_int, c_int)
    _sig(L.cp_track_workspace_bytes, c_size_t, c_int, c_int, c_int)
    _sig(L.cp_track_reset, c_int, c_void_p, c_void_p, c_int, c_int)
    _sig(L.cp_track_status, c_int, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int))
    _sig(L.cp_track_step, c_int, c_void_p, ctypes.POINTER(TrackParams), c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
         c_void_p, c_void_p, c_size_t)
    _sig(L.cp_track_seed, c_int, c_void_p, ctypes.POINTER(TrackParams), c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
         c_void_p, c_void_p)
    _sig(L.cp_linear_assignment, c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_int))
    _sig(L.cp_box_iou, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p)
    _sig(L.cp_box_eval, c_int, c_void_p, *([c_void_p] * 6), c_int, c_int, c_void_p)
    _sig(L.cp_pose_loss_workspace_bytes, c_size_t, ctypes.POINTER(PoseLossDesc))
    _sig(L.cp_pose_loss_forward, c_int, c_void_p, ctypes.POINTER(PoseLossDesc), c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_size_t)
    _sig(L.cp_pose_loss_backward, c_int, c_void_p, ctypes.POINTER(PoseLossDesc), c_void_p, ctypes.POINTER(c_void_p),
         ctypes.POINTER(c_void_p), c_void_p, c_size_t)
    _sig(L.cp_pose_targets_workspace_bytes, c_size_t, ctypes.POINTER(PoseTargetsDesc))
    _sig(L.cp_pose_targets, c_int, c_void_p, ctypes.POINTER(PoseTargetsDesc), c_void_p, c_size_t)
    _sig(L.cp_pose_targets_track_workspace_bytes, c_size_t, ctypes.POINTER(PoseTargetsTrackDesc))
    _sig(L.cp_pose_targets_track, c_int, c_void_p, ctypes.POINTER(PoseTargetsTrackDesc), c_void_p, c_size_t)
    _sig(L.cp_pose_targets_track_det_workspace_bytes, c_size_t, ctypes.POINTER(PoseTargetsTrackDetDesc))
    _sig(L.cp_pose_targets_track_det, c_int, c_void_p, ctypes.POINTER(PoseTargetsTrackDetDesc), c_void_p, c_size_t)
    _sig(L.cp_train_inputs_workspace_bytes, c_size_t, c_int, c_int, c_int)
    _sig(L.cp_train_inputs, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_int, ctypes.POINTER(ctypes.c_float),
         ctypes.POINTER(ctypes.c_float), c_void_p, c_int, c_int, c_void_p, c_size_t)
    _lib = L
    return L


def linear_assignment(cost, solver=1):
    """The tracker's optimal assignment on the host (cp_linear_assignment; no device involved): ``cost`` [n, m] float64 ->
    int64 array [min(n, m), 2] of (row, column) pairs sorted by row, the return value of scikit-learn 0.22's
    ``linear_assignment`` (tracker.py:157).  solver 1 = that module's Munkres, 2 = scipy's rectangular LSAP."""
    import numpy as np

    cost = np.ascontiguousarray(cost, dtype=np.float64)
    if cost.ndim != 2:
        raise ValueError("linear_assignment: a 2-D cost matrix is expected")
    n, m = cost.shape
    match = (c_int * max(n, 1))()
    _check(lib().cp_linear_assignment(cost.ctypes.data_as(c_void_p), n, m, int(solver), match), "cp_linear_assignment")
    return np.array([(i, match[i]) for i in range(n) if match[i] >= 0], dtype=np.int64).reshape(-1, 2)


def exported_symbols():
    """Names every declaration in include/centerpose_hip.h (+ the test hook of centerpose_hip_testing.h) must resolve to (used by CPU tests)."""
    return ["cp_version", "cp_last_error", "cp_dcnv2_workspace_bytes", "cp_dcnv2_forward", "cp_model_create",
            "cp_model_set_param", "cp_model_finalize", "cp_model_destroy", "cp_model_workspace_bytes", "cp_model_workspace_used",
            "cp_model_maxpool_launches",
            "cp_model_forward", "cp_model_forward_tap", "cp_conv2d_workspace_bytes", "cp_conv2d_nhwc",
            "cp_decode_workspace_bytes", "cp_decode", "cp_pnp_workspace_bytes", "cp_pnp_solve", "cp_model_profile", "cp_model_profile_read",
            "cp_kernel_variant_name", "cp_set_default_precision", "cp_model_set_precision", "cp_model_detect_workspace_bytes", "cp_model_detect", "cp_set_debug", "cp_preprocess", "cp_preprocess_batch", "cp_postprocess_workspace_bytes", "cp_postprocess", "cp_render_gaussians",
            "cp_model_profile_roles", "cp_role_name", "cp_pnp_from_post_workspace_bytes", "cp_pnp_from_post", "cp_resize_u8",
            "cp_abi_version", "cp_num_kernel_variants", "cp_num_roles", "cp_track_state_bytes", "cp_track_workspace_bytes",
            "cp_track_reset", "cp_track_step", "cp_track_status", "cp_track_seed", "cp_linear_assignment", "cp_decode_tiled_workspace_bytes",
            "cp_decode_tiled", "cp_box_iou", "cp_box_eval", "cp_conv_transpose2d_workspace_bytes",
            "cp_conv_transpose2d_nhwc", "cp_dcnv2_backward_workspace_bytes", "cp_dcnv2_backward",
            "cp_pose_loss_workspace_bytes", "cp_pose_loss_forward", "cp_pose_loss_backward",
            "cp_pose_targets_workspace_bytes", "cp_pose_targets", "cp_model_lean_supported",
            "cp_model_detect_lean_workspace_bytes", "cp_model_detect_lean", "cp_model_dense_heads",
            "cp_model_heads_at_workspace_bytes", "cp_model_heads_at", "cp_decode_peaks_workspace_bytes", "cp_decode_peaks",
            "cp_decode_gathered", "cp_pose_heads_chunk_images", "cp_pose_heads_forward_workspace_bytes",
            "cp_pose_heads_forward", "cp_pose_heads_backward_workspace_bytes", "cp_pose_heads_backward",
            "cp_model_features", "cp_conv2d_backward_workspace_bytes", "cp_conv2d_backward_nhwc", "cp_conv2d_backward_path",
            "cp_batchnorm_workspace_bytes", "cp_batchnorm_forward_nhwc", "cp_batchnorm_backward_nhwc",
            "cp_conv_transpose2d_dw_nhwc", "cp_conv_transpose2d_backward_workspace_bytes",
            "cp_conv_transpose2d_backward_nhwc", "cp_maxpool2d_forward_nhwc", "cp_maxpool2d_backward_nhwc",
            "cp_conv2d_stem_backward_workspace_bytes", "cp_conv2d_stem_backward", "cp_groupnorm_workspace_bytes",
            "cp_groupnorm_forward_nhwc", "cp_groupnorm_backward_nhwc", "cp_gru_gate_forward", "cp_gru_gate_backward",
            "cp_pose_targets_track_workspace_bytes", "cp_pose_targets_track", "cp_train_inputs_workspace_bytes",
            "cp_train_inputs", "cp_pose_targets_track_det_workspace_bytes", "cp_pose_targets_track_det",
            "cp_dcnv2_backward_det_workspace_bytes", "cp_dcnv2_backward_det"]


def _check(rc, what):
    if rc != 0:
        msg = lib().cp_last_error().decode() if _lib is not None else ""
        raise RuntimeError("centerpose_hip: %s failed with code %d (%s)" % (what, rc, msg))


class KernelSel(enum.IntFlag):
    """The CP_SEL_* kernel-selection switches of include/centerpose_hip_testing.h (name = the header's without CP_SEL_)."""
    HEADS_SLABS = 0x00000001
    HEADS_WG_PER_HEAD = 0x00000002
    PW16_FRAG_A = 0x00000004
    SPLITK_ELEMENTWISE = 0x00000008
    TILE128_SMALL = 0x00000010
    NO_HEAD_FUSION = 0x00000020
    NO_LOWC = 0x00000040
    GN_HEAD_F32 = 0x00000080
    GRU_UNFUSED = 0x00000100
    NO_PRESCALE = 0x00000200
    DCN16S_GRID8 = 0x00000400
    HALO_NEVER = 0x00001000
    HALO_ALWAYS = 0x00002000
    HALO_LDS_WEIGHTS = 0x00004000
    DCN16P_NEVER = 0x00008000
    DCN16P_ALWAYS = 0x00010000
    GN_HEAD_MFMA = 0x00020000
    LEVEL1_ROWS_NEVER = 0x00040000
    DCN16P_NOT_WIDE = 0x00080000
    DCN16S_NEVER = 0x00100000
    DCN16S_ALWAYS = 0x00200000
    PW16_NEVER = 0x00400000
    DCN_GENERIC = 0x00800000
    HEADS_PER_HEAD_LAUNCH = 0x01000000
    DCN16T_ALWAYS = 0x02000000
    DCN16T_NEVER = 0x04000000
    STEM_LEVEL0_UNFUSED = 0x08000000
    STRM16_NEVER = 0x10000000
    STRM16_ALWAYS = 0x20000000
    LEVEL1_ROWS_ALWAYS = 0x40000000


@contextlib.contextmanager
def select_kernels(flags):
    """Run the block under the kernel-selection switches ``flags`` (KernelSel; cp_set_debug, a test hook) and return to the
    engine's own choice (0) on the way out, whatever happens inside."""
    _check(lib().cp_set_debug(int(flags)), "cp_set_debug")
    try:
        yield
    finally:
        lib().cp_set_debug(0)


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _dev(t):
    if not t.is_cuda:
        raise RuntimeError("centerpose_hip: tensors must live on the HIP device (no CPU path)")
    return t.contiguous().float()


def dcn_v2_forward(input, weight, bias, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group):
    """Same 14-argument signature as the reference's ``_ext.dcn_v2_forward`` (DCNv2/src/vision.cpp:5)."""
    L = lib()
    input, weight, bias, offset, mask = map(_dev, (input, weight, bias, offset, mask))
    B, C, H, W = input.shape
    Co = weight.shape[0]
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1  # dcn_v2_cuda.cu:75-76
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    if Ho < 1 or Wo < 1:
        raise RuntimeError("dcn_v2_forward: empty output")
    for name, t, shape in (("weight", weight, (Co, C, kh, kw)), ("bias", bias, (Co,)),
                           ("offset", offset, (B, deformable_group * 2 * kh * kw, Ho, Wo)),
                           ("mask", mask, (B, deformable_group * kh * kw, Ho, Wo))):
        if tuple(t.shape) != shape:  # the reference's AT_ASSERTM shape checks (dcn_v2_cuda.cu:60-66)
            raise RuntimeError("dcn_v2_forward: %s has shape %s, expected %s" % (name, tuple(t.shape), shape))
    out = torch.empty(B, Co, Ho, Wo, device=input.device, dtype=torch.float32)
    nbytes = L.cp_dcnv2_workspace_bytes(B, C, H, W, Co)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=input.device)
    rc = L.cp_dcnv2_forward(_stream(), _ptr(input), _ptr(weight), _ptr(bias), _ptr(offset), _ptr(mask), _ptr(out),
                            B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, _ptr(ws), nbytes)
    _check(rc, "cp_dcnv2_forward")
    return out


_deterministic = False
_warned_nondeterministic = False


def set_deterministic(flag):
    """Process-wide default of ``dcn_v2_backward``'s ``deterministic`` argument (False at import): with it every gradient
    of a training step is bitwise reproducible from run to run.  Returns the previous value."""
    global _deterministic
    prev, _deterministic = _deterministic, bool(flag)
    return prev


def deterministic():
    return _deterministic


def dcn_backward_is_fast(C, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group):
    """The geometry cp_dcnv2_backward_det covers (dcn_bwd.hip: cp_dcn_backward_fast)."""
    return (kh, kw, sh, sw, ph, pw, dh, dw, deformable_group) == (3, 3, 1, 1, 1, 1, 1, 1, 1) and C % 16 == 0


def resolve_deterministic(requested, fast, own_flag, torch_flag, torch_warn_only, what=""):
    """Which DCNv2 backward runs (pure: no device, no globals).  ``requested``: the call's ``deterministic`` argument (None:
    ``own_flag or torch_flag``); ``fast``: the geometry is one the deterministic kernels cover.  Returns (use the
    deterministic path, warn that the atomic path runs instead).  A deterministic request for any other geometry raises
    RuntimeError, as torch does for an operator without a deterministic implementation -- unless it came from torch's flag
    alone and torch's warn_only is set."""
    want = (own_flag or torch_flag) if requested is None else bool(requested)
    if not want:
        return False, False
    if fast:
        return True, False
    if requested is None and not own_flag and torch_warn_only:
        return False, True
    raise RuntimeError("dcn_v2_backward does not have a deterministic implementation for %s: the deterministic path covers "
                       "3x3 / stride 1 / pad 1 / dilation 1 / deformable_group 1 / C %% 16 == 0.  Pass deterministic=False, or "
                       "turn off hip.set_deterministic / torch.use_deterministic_algorithms." % (what or "this geometry"))


def dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group,
                    workspace=None, deterministic=None):
    """Same 15-argument signature as the reference's ``_ext.dcn_v2_backward`` (DCNv2/src/vision.cpp:6, dcn_v2.h:48-80):
    returns [grad_input, grad_offset, grad_mask, grad_weight, grad_bias], float32 on the input's device.  ``workspace`` (a
    uint8 device tensor of at least the queried size) may be passed to skip the allocation; a smaller one is an error.
    ``deterministic``: True runs cp_dcnv2_backward_det (grad_input summed in a fixed order, no float atomics: all five
    gradients bitwise reproducible; a larger workspace), False cp_dcnv2_backward, None (default) resolves at call time to
    ``hip.deterministic() or torch.are_deterministic_algorithms_enabled()`` -- see resolve_deterministic."""
    global _warned_nondeterministic
    L = lib()
    input, weight, bias, offset, mask, grad_output = map(_dev, (input, weight, bias, offset, mask, grad_output))
    B, C, H, W = input.shape
    Co = weight.shape[0]
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1  # dcn_v2_cuda.cu:242-243
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    if Ho < 1 or Wo < 1:
        raise RuntimeError("dcn_v2_backward: empty output")
    for name, t, shape in (("weight", weight, (Co, C, kh, kw)), ("bias", bias, (Co,)),
                           ("offset", offset, (B, deformable_group * 2 * kh * kw, Ho, Wo)),
                           ("mask", mask, (B, deformable_group * kh * kw, Ho, Wo)),
                           ("grad_output", grad_output, (B, Co, Ho, Wo))):
        if tuple(t.shape) != shape:
            raise RuntimeError("dcn_v2_backward: %s has shape %s, expected %s" % (name, tuple(t.shape), shape))
    geo = (kh, kw, sh, sw, ph, pw, dh, dw, deformable_group)
    det, warn = resolve_deterministic(
        deterministic, dcn_backward_is_fast(C, *geo), _deterministic, torch.are_deterministic_algorithms_enabled(),
        torch.is_deterministic_algorithms_warn_only_enabled(),
        "kernel %dx%d, stride (%d, %d), padding (%d, %d), dilation (%d, %d), deformable_group %d, C = %d" % (*geo, C))
    if warn and not _warned_nondeterministic:
        import warnings

        _warned_nondeterministic = True
        warnings.warn("dcn_v2_backward has no deterministic implementation for this geometry; running the float-atomic path "
                      "(torch.use_deterministic_algorithms(True, warn_only=True))")
    query, call = ((L.cp_dcnv2_backward_det_workspace_bytes, L.cp_dcnv2_backward_det) if det else
                   (L.cp_dcnv2_backward_workspace_bytes, L.cp_dcnv2_backward))
    grads = [torch.empty_like(t) for t in (input, offset, mask, weight, bias)]
    nbytes = query(B, C, H, W, Co, *geo)
    if nbytes == 0:
        raise RuntimeError("dcn_v2_backward: shape refused by the library")
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=input.device)
    rc = call(_stream(), _ptr(input), _ptr(weight), _ptr(offset), _ptr(mask), _ptr(grad_output),
              *[_ptr(g) for g in grads], B, C, H, W, Co, *geo, _ptr(workspace), workspace.numel() * workspace.element_size())
    _check(rc, "cp_dcnv2_backward_det" if det else "cp_dcnv2_backward")
    return grads


def _nhwc_view(feat):
    """[B,C,H,W] tensor -> the same values as NHWC memory ([B,C,H,W] tensor in channels_last format; no copy when it already is)."""
    if not feat.is_cuda:
        raise RuntimeError("centerpose_hip: tensors must live on the HIP device (no CPU path)")
    if feat.dim() != 4:
        raise RuntimeError("pose_heads: feat must be [B, Cin, H, W]")
    return feat.float().contiguous(memory_format=torch.channels_last)


def _heads_args(feat, params):
    """Shape checks and the pointer tables of a pose_heads call.  ``params``: per head (w0 [hid,Cin,3,3], b0 [hid],
    w1 [classes,hid,1,1], b1 [classes])."""
    B, Cin, H, W = feat.shape
    if len(params) < 1:
        raise RuntimeError("pose_heads: at least one head is needed")
    hid = params[0][0].shape[0]
    flat, classes = [], []
    for i, (w0, b0, w1, b1) in enumerate(params):
        w0, b0, w1, b1 = map(_dev, (w0, b0, w1, b1))
        c = w1.shape[0]
        for name, t, shape in (("w0", w0, (hid, Cin, 3, 3)), ("b0", b0, (hid,)), ("w1", w1, (c, hid, 1, 1)), ("b1", b1, (c,))):
            if tuple(t.shape) != shape:
                raise RuntimeError("pose_heads: head %d %s has shape %s, expected %s" % (i, name, tuple(t.shape), shape))
        flat.append((w0, b0, w1, b1))
        classes.append(int(c))
    n = len(flat)
    tables = [(c_void_p * n)(*[p[k].data_ptr() for p in flat]) for k in range(4)]
    return flat, tables, (c_int * n)(*classes), classes, (B, H, W, Cin, hid)


def pose_heads_chunk_images(B, H, W, hid):
    """Images whose hidden layer pose_heads_backward materialises at a time (cp_pose_heads_chunk_images)."""
    return int(lib().cp_pose_heads_chunk_images(int(B), int(H), int(W), int(hid)))


def pose_heads_forward(feat, params):
    """The prediction-head block conv3x3 -> ReLU -> conv1x1 of every head on one feature map (cp_pose_heads_forward).
    ``feat`` [B,Cin,H,W] (NCHW-contiguous or channels_last; the kernels read NHWC), ``params`` a list of (w0, b0, w1, b1)
    per head -> list of [B,classes_i,H,W] raw logits."""
    L = lib()
    feat = _nhwc_view(feat)
    flat, tables, cls_arr, classes, (B, H, W, Cin, hid) = _heads_args(feat, params)
    outs = [torch.empty(B, c, H, W, device=feat.device, dtype=torch.float32) for c in classes]
    optr = (c_void_p * len(outs))(*[t.data_ptr() for t in outs])
    nbytes = L.cp_pose_heads_forward_workspace_bytes(B, H, W, Cin, hid, len(outs), cls_arr)
    if nbytes == 0:
        raise RuntimeError("pose_heads_forward: shape refused by the library (%s)" % L.cp_last_error().decode())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=feat.device)
    rc = L.cp_pose_heads_forward(_stream(), _ptr(feat), len(outs), *tables, cls_arr, optr, B, H, W, Cin, hid, _ptr(ws), nbytes)
    _check(rc, "cp_pose_heads_forward")
    return outs


def pose_heads_backward(feat, params, grad_outs, need_feat_grad=True, grad_feat=None):
    """Gradients of pose_heads_forward (cp_pose_heads_backward).  ``grad_outs``: per head a [B,classes_i,H,W] tensor or None (a
    head the loss does not use: zero parameter gradients, nothing added to grad_feat).  Returns (grad_feat, grads) with
    grads[i] = (grad_w0, grad_b0, grad_w1, grad_b1); grad_feat is a [B,Cin,H,W] channels_last tensor, or None when
    ``need_feat_grad`` is false (the data-gradient contraction is then not launched).  ``grad_feat``: an optional
    channels_last buffer to write into."""
    L = lib()
    feat = _nhwc_view(feat)
    flat, tables, cls_arr, classes, (B, H, W, Cin, hid) = _heads_args(feat, params)
    n = len(flat)
    if len(grad_outs) != n:
        raise RuntimeError("pose_heads_backward: %d gradients for %d heads" % (len(grad_outs), n))
    gos = []
    for i, g in enumerate(grad_outs):
        if g is not None:
            g = _dev(g)
            if tuple(g.shape) != (B, classes[i], H, W):
                raise RuntimeError("pose_heads_backward: grad_out %d has shape %s, expected %s"
                                   % (i, tuple(g.shape), (B, classes[i], H, W)))
        gos.append(g)
    grads = [tuple(torch.empty_like(t) for t in p) for p in flat]
    gtab = [(c_void_p * n)(*[g[k].data_ptr() for g in grads]) for k in range(4)]
    goptr = (c_void_p * n)(*[g.data_ptr() if g is not None else None for g in gos])
    if need_feat_grad and grad_feat is None:
        grad_feat = torch.empty_like(feat, memory_format=torch.channels_last)
    if need_feat_grad and not (grad_feat.is_cuda and grad_feat.dtype == torch.float32 and grad_feat.shape == feat.shape and
                               grad_feat.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("pose_heads_backward: grad_feat must be a float32 channels_last tensor of feat's shape")
    nbytes = L.cp_pose_heads_backward_workspace_bytes(B, H, W, Cin, hid, n, cls_arr)
    if nbytes == 0:
        raise RuntimeError("pose_heads_backward: shape refused by the library (%s)" % L.cp_last_error().decode())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=feat.device)
    rc = L.cp_pose_heads_backward(_stream(), _ptr(feat), n, *tables, cls_arr, goptr, *gtab,
                                  _ptr(grad_feat) if need_feat_grad else c_void_p(0), B, H, W, Cin, hid, _ptr(ws), nbytes)
    _check(rc, "cp_pose_heads_backward")
    return (grad_feat if need_feat_grad else None), grads


def conv2d_nhwc(x, w, scale=None, shift=None, residual=None, stride=1, pad=0, act=0):
    """x [B,H,W,Cin] NHWC, w [Cout,Cin,KH,KW] -> [B,Ho,Wo,Cout] NHWC (unit-test entry of the igemm kernel)."""
    L = lib()
    x, w = _dev(x), _dev(w)
    B, H, W, Cin = x.shape
    Cout, _, KH, KW = w.shape
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    out = torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=torch.float32)
    nbytes = L.cp_conv2d_workspace_bytes(Cin, Cout, KH, KW)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    scale = _dev(scale) if scale is not None else None
    shift = _dev(shift) if shift is not None else None
    residual = _dev(residual) if residual is not None else None
    rc = L.cp_conv2d_nhwc(_stream(), _ptr(x), _ptr(w), _ptr(scale), _ptr(shift), _ptr(residual), _ptr(out),
                          B, H, W, Cin, Cout, KH, KW, stride, pad, act, _ptr(ws), nbytes)
    _check(rc, "cp_conv2d_nhwc")
    return out


def conv2d_backward(x, w, grad_out, stride=1, pad=0, y=None, need_x_grad=True, need_bias_grad=True):
    """Gradients of ``conv2d_nhwc(x, w, shift=bias)`` (cp_conv2d_backward_nhwc): x [B,H,W,Cin] NHWC, w [Cout,Cin,KH,KW],
    grad_out [B,Ho,Wo,Cout] NHWC -> (grad_x [B,H,W,Cin] | None, grad_w [Cout,Cin,KH,KW], grad_bias [Cout] | None).  ``y``: the
    activated forward output when the layer ended in a ReLU (grad_out is gated by y > 0).  Float32 and bitwise reproducible."""
    L = lib()
    x, w, grad_out = _dev(x), _dev(w), _dev(grad_out)
    y = _dev(y) if y is not None else None
    if x.dim() != 4 or w.dim() != 4 or w.shape[1] != x.shape[3]:
        raise RuntimeError("conv2d_backward: x must be [B,H,W,Cin] and w [Cout,Cin,KH,KW], got %s and %s"
                           % (tuple(x.shape), tuple(w.shape)))
    B, H, W, Cin = x.shape
    Cout, _, KH, KW = w.shape
    stride, pad = int(stride), int(pad)
    nbytes = L.cp_conv2d_backward_workspace_bytes(B, H, W, Cin, Cout, KH, KW, stride, pad, int(bool(need_x_grad)))
    if nbytes == 0:
        raise RuntimeError("conv2d_backward: shape refused by the library (%s)" % L.cp_last_error().decode())
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    for name, t in (("grad_out", grad_out), ("y", y)):
        if t is not None and tuple(t.shape) != (B, Ho, Wo, Cout):
            raise RuntimeError("conv2d_backward: %s has shape %s, expected %s" % (name, tuple(t.shape), (B, Ho, Wo, Cout)))
    grad_x = torch.empty_like(x) if need_x_grad else None
    grad_w = torch.empty_like(w)
    grad_b = torch.empty(Cout, device=x.device, dtype=torch.float32) if need_bias_grad else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    rc = L.cp_conv2d_backward_nhwc(_stream(), _ptr(x), _ptr(w), _ptr(y), _ptr(grad_out), _ptr(grad_x), _ptr(grad_w),
                                   _ptr(grad_b), B, H, W, Cin, Cout, KH, KW, stride, pad, _ptr(ws), nbytes)
    _check(rc, "cp_conv2d_backward_nhwc")
    return grad_x, grad_w, grad_b


CONV_BWD_GENERIC, CONV_BWD_MFMA, CONV_BWD_LOWC = 0, 1, 2   # include/centerpose_hip.h: CP_CONV_BWD_*


def conv2d_backward_path(B, H, W, Cin, Cout, KH, KW, stride=1, pad=0):
    """The kernels ``conv2d_backward`` takes for a geometry (cp_conv2d_backward_path; host arithmetic, no device involved):
    CONV_BWD_MFMA (KH == KW in {1, 3}, stride 1 | 2, pad == KH // 2, Cin % 32 == 0), CONV_BWD_LOWC (3x3, pad 1, stride 1 | 2,
    16 -> 16 | 32 channels and at least 4096 output pixels: dla_34's level0 / level1) or CONV_BWD_GENERIC (everything else the
    operator accepts: correct, not fast).  Raises RuntimeError for a geometry the operator refuses."""
    L = lib()
    rc = L.cp_conv2d_backward_path(int(B), int(H), int(W), int(Cin), int(Cout), int(KH), int(KW), int(stride), int(pad))
    if rc < 0:
        raise RuntimeError("conv2d_backward_path: shape refused by the library (%s)" % L.cp_last_error().decode())
    return rc


def _bn_vec(t, C, name):
    if t is None:
        return None
    t = _dev(t)
    if tuple(t.shape) != (C,):
        raise RuntimeError("batch_norm: %s has shape %s, expected %s" % (name, tuple(t.shape), (C,)))
    return t


def _bn_ws(L, x):
    if not x.is_cuda:
        raise RuntimeError("centerpose_hip: tensors must live on the HIP device (no CPU path)")
    if x.dim() != 4:
        raise RuntimeError("batch_norm: x must be [B,H,W,C], got %s" % (tuple(x.shape),))
    B, H, W, C = x.shape
    nbytes = L.cp_batchnorm_workspace_bytes(B, H, W, C)
    if nbytes == 0:
        raise RuntimeError("batch_norm: shape refused by the library (%s)" % L.cp_last_error().decode())
    return (B, H, W, C), nbytes, torch.empty(nbytes, dtype=torch.uint8, device=x.device)


def batch_norm_forward(x, gamma=None, beta=None, residual=None, running_mean=None, running_var=None, training=True,
                       momentum=0.1, eps=1e-5, act=0):
    """``act(batch_norm(x) [+ residual])`` (cp_batchnorm_forward_nhwc): x, residual [B,H,W,C] NHWC, gamma / beta [C] or None
    (1 / 0) -> (y [B,H,W,C], save_mean [C], save_invstd [C]).  ``training``: the batch's statistics, and running_mean /
    running_var (float32 device tensors, when given) are updated IN PLACE with ``momentum``; otherwise they are the
    statistics.  act 0 none, 1 relu.  Float32 and bitwise reproducible."""
    L = lib()
    geo, nbytes, ws = _bn_ws(L, x)
    x = _dev(x)
    C = geo[3]
    gamma, beta = _bn_vec(gamma, C, "gamma"), _bn_vec(beta, C, "beta")
    if residual is not None:
        residual = _dev(residual)
        if residual.shape != x.shape:
            raise RuntimeError("batch_norm: residual has shape %s, expected %s" % (tuple(residual.shape), tuple(x.shape)))
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (C,)):
            raise RuntimeError("batch_norm: %s must be a contiguous float32 [%d] tensor on the HIP device" % (name, C))
    y = torch.empty_like(x)
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    invstd = torch.empty_like(mean)
    rc = L.cp_batchnorm_forward_nhwc(_stream(), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(residual), _ptr(running_mean),
                                     _ptr(running_var), _ptr(y), _ptr(mean), _ptr(invstd), *geo, int(bool(training)),
                                     float(momentum), float(eps), int(act), _ptr(ws), nbytes)
    _check(rc, "cp_batchnorm_forward_nhwc")
    return y, mean, invstd


def batch_norm_backward(x, grad_out, save_mean, save_invstd, gamma=None, y=None, training=True, need_x_grad=True,
                        need_residual_grad=False, need_gamma_grad=True, need_beta_grad=True):
    """Gradients of batch_norm_forward (cp_batchnorm_backward_nhwc) -> (grad_x, grad_residual, grad_gamma, grad_beta), None
    where not asked for.  ``y``: the activated forward output when act was 1 (grad_out is gated by y > 0); without it
    grad_residual is ``grad_out`` itself, not a copy.  Float32 and bitwise reproducible."""
    L = lib()
    geo, nbytes, ws = _bn_ws(L, x)
    x, grad_out = _dev(x), _dev(grad_out)
    y = _dev(y) if y is not None else None
    C = geo[3]
    for name, t in (("grad_out", grad_out), ("y", y)):
        if t is not None and t.shape != x.shape:
            raise RuntimeError("batch_norm_backward: %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(x.shape)))
    gamma, save_mean, save_invstd = _bn_vec(gamma, C, "gamma"), _bn_vec(save_mean, C, "save_mean"), _bn_vec(save_invstd, C, "save_invstd")
    grad_x = torch.empty_like(x) if need_x_grad else None
    grad_res = torch.empty_like(x) if need_residual_grad and y is not None else None
    grad_g = torch.empty(C, device=x.device, dtype=torch.float32) if need_gamma_grad else None
    grad_b = torch.empty(C, device=x.device, dtype=torch.float32) if need_beta_grad else None
    if need_x_grad or grad_res is not None or need_gamma_grad or need_beta_grad:
        rc = L.cp_batchnorm_backward_nhwc(_stream(), _ptr(x), _ptr(y), _ptr(grad_out), _ptr(gamma), _ptr(save_mean),
                                          _ptr(save_invstd), _ptr(grad_x), _ptr(grad_res), _ptr(grad_g), _ptr(grad_b), *geo,
                                          int(bool(training)), _ptr(ws), nbytes)
        _check(rc, "cp_batchnorm_backward_nhwc")
    if need_residual_grad and y is None:
        grad_res = grad_out
    return grad_x, grad_res, grad_g, grad_b


def _gn_ws(L, x, G):
    if not x.is_cuda:
        raise RuntimeError("centerpose_hip: tensors must live on the HIP device (no CPU path)")
    if x.dim() != 4:
        raise RuntimeError("group_norm: x must be [B,H,W,C], got %s" % (tuple(x.shape),))
    B, H, W, C = x.shape
    nbytes = L.cp_groupnorm_workspace_bytes(B, H, W, C, int(G))
    if nbytes == 0:
        raise RuntimeError("group_norm: shape refused by the library (%s)" % L.cp_last_error().decode())
    return (B, H, W, C, int(G)), nbytes, torch.empty(nbytes, dtype=torch.uint8, device=x.device)


def group_norm_forward(x, num_groups, gamma=None, beta=None, eps=1e-5, act=0):
    """``act(group_norm(x))`` (cp_groupnorm_forward_nhwc): x [B,H,W,C] NHWC, gamma / beta [C] or None (1 / 0) -> (y [B,H,W,C],
    save_mean [B,G], save_invstd [B,G]).  act 0 none, 1 relu.  ``C % 4 == 0`` and ``C / G`` 1, 2 or a multiple of 4.  Float32
    and bitwise reproducible."""
    L = lib()
    geo, nbytes, ws = _gn_ws(L, x, num_groups)
    x = _dev(x)
    B, C, G = geo[0], geo[3], geo[4]
    gamma, beta = _bn_vec(gamma, C, "gamma"), _bn_vec(beta, C, "beta")
    y = torch.empty_like(x)
    mean = torch.empty(B, G, device=x.device, dtype=torch.float32)
    invstd = torch.empty_like(mean)
    rc = L.cp_groupnorm_forward_nhwc(_stream(), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(invstd), *geo,
                                     float(eps), int(act), _ptr(ws), nbytes)
    _check(rc, "cp_groupnorm_forward_nhwc")
    return y, mean, invstd


def group_norm_backward(x, grad_out, num_groups, save_mean, save_invstd, gamma=None, y=None, need_x_grad=True,
                        need_gamma_grad=True, need_beta_grad=True):
    """Gradients of group_norm_forward (cp_groupnorm_backward_nhwc) -> (grad_x, grad_gamma, grad_beta), None where not asked
    for.  ``y``: the activated forward output when act was 1 (grad_out is gated by y > 0).  Float32 and bitwise reproducible."""
    L = lib()
    geo, nbytes, ws = _gn_ws(L, x, num_groups)
    x, grad_out = _dev(x), _dev(grad_out)
    y = _dev(y) if y is not None else None
    B, C, G = geo[0], geo[3], geo[4]
    for name, t in (("grad_out", grad_out), ("y", y)):
        if t is not None and t.shape != x.shape:
            raise RuntimeError("group_norm_backward: %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(x.shape)))
    gamma = _bn_vec(gamma, C, "gamma")
    save_mean, save_invstd = _dev(save_mean), _dev(save_invstd)
    for name, t in (("save_mean", save_mean), ("save_invstd", save_invstd)):
        if tuple(t.shape) != (B, G):
            raise RuntimeError("group_norm_backward: %s has shape %s, expected %s" % (name, tuple(t.shape), (B, G)))
    grad_x = torch.empty_like(x) if need_x_grad else None
    grad_g = torch.empty(C, device=x.device, dtype=torch.float32) if need_gamma_grad else None
    grad_b = torch.empty(C, device=x.device, dtype=torch.float32) if need_beta_grad else None
    if need_x_grad or need_gamma_grad or need_beta_grad:
        rc = L.cp_groupnorm_backward_nhwc(_stream(), _ptr(x), _ptr(y), _ptr(grad_out), _ptr(gamma), _ptr(save_mean),
                                          _ptr(save_invstd), _ptr(grad_x), _ptr(grad_g), _ptr(grad_b), *geo, _ptr(ws), nbytes)
        _check(rc, "cp_groupnorm_backward_nhwc")
    return grad_x, grad_g, grad_b


def _gru_args(x3, h3, hprev):
    if not x3.is_cuda:
        raise RuntimeError("centerpose_hip: tensors must live on the HIP device (no CPU path)")
    if x3.dim() < 2 or x3.shape[-1] % 3:
        raise RuntimeError("gru_gate: x3 must be [..., 3 * Ch], got %s" % (tuple(x3.shape),))
    if (h3 is None) != (hprev is None):
        raise RuntimeError("gru_gate: h3 and hprev are given together, or neither (step 0)")
    x3 = _dev(x3)
    Ch = x3.shape[-1] // 3
    lead = tuple(x3.shape[:-1])
    if h3 is not None:
        h3, hprev = _dev(h3), _dev(hprev)
        if h3.shape != x3.shape or tuple(hprev.shape) != lead + (Ch,):
            raise RuntimeError("gru_gate: h3 %s / hprev %s do not match x3 %s" % (tuple(h3.shape), tuple(hprev.shape), tuple(x3.shape)))
    return x3, h3, hprev, lead, x3.numel() // (3 * Ch), Ch


def gru_gate_forward(x3, h3=None, hprev=None):
    """The ConvGRU cell's gate arithmetic (cp_gru_gate_forward): x3 = [Wir x | Wiz x | Win x] (+ biases) and h3 = [Whr h | Whz h |
    Whn h] as [..., 3 Ch], hprev [..., Ch] -> hout [..., Ch] = (1 - z) n + z hprev.  ``h3 = hprev = None``: step 0, h = 0."""
    x3, h3, hprev, lead, M, Ch = _gru_args(x3, h3, hprev)
    hout = torch.empty(lead + (Ch,), device=x3.device, dtype=torch.float32)
    _check(lib().cp_gru_gate_forward(_stream(), _ptr(x3), _ptr(h3), _ptr(hprev), _ptr(hout), M, Ch), "cp_gru_gate_forward")
    return hout


def gru_gate_backward(x3, h3, hprev, grad_hout, need_h3_grad=True, need_hprev_grad=True):
    """Gradients of gru_gate_forward (cp_gru_gate_backward) -> (grad_x3, grad_h3, grad_hprev); the gates are recomputed from
    the inputs.  At step 0 (``h3 = hprev = None``) the two hidden-side gradients are None."""
    x3, h3, hprev, lead, M, Ch = _gru_args(x3, h3, hprev)
    grad_hout = _dev(grad_hout)
    if tuple(grad_hout.shape) != lead + (Ch,):
        raise RuntimeError("gru_gate_backward: grad_hout has shape %s, expected %s" % (tuple(grad_hout.shape), lead + (Ch,)))
    grad_x3 = torch.empty_like(x3)
    grad_h3 = torch.empty_like(x3) if h3 is not None and need_h3_grad else None
    grad_hp = torch.empty_like(grad_hout) if h3 is not None and need_hprev_grad else None
    _check(lib().cp_gru_gate_backward(_stream(), _ptr(x3), _ptr(h3), _ptr(hprev), _ptr(grad_hout), _ptr(grad_x3), _ptr(grad_h3),
                                      _ptr(grad_hp), M, Ch), "cp_gru_gate_backward")
    return grad_x3, grad_h3, grad_hp


def conv_transpose2d(x, w, scale=None, shift=None, act=0):
    """x [B,H,W,Cin] NHWC, w [Cin,Cout,4,4] (ConvTranspose2d(k=4, stride=2, padding=1) layout) -> [B,2H,2W,Cout] NHWC,
    y = act(deconv(x) * scale + shift); act 0 none, 1 relu.  Precision: set_default_precision."""
    L = lib()
    x, w = _dev(x), _dev(w)
    B, H, W, Cin = x.shape
    if tuple(w.shape[2:]) != (4, 4) or w.shape[0] != Cin:
        raise RuntimeError("conv_transpose2d: weight must be [Cin, Cout, 4, 4], got %s" % (tuple(w.shape),))
    Cout = w.shape[1]
    out = torch.empty(B, 2 * H, 2 * W, Cout, device=x.device, dtype=torch.float32)
    nbytes = L.cp_conv_transpose2d_workspace_bytes(Cin, Cout)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    scale = _dev(scale) if scale is not None else None
    shift = _dev(shift) if shift is not None else None
    rc = L.cp_conv_transpose2d_nhwc(_stream(), _ptr(x), _ptr(w), _ptr(scale), _ptr(shift), _ptr(out),
                                    B, H, W, Cin, Cout, act, _ptr(ws), nbytes)
    _check(rc, "cp_conv_transpose2d_nhwc")
    return out


def conv_transpose2d_dw(x, w, f, add=None):
    """IDAUp's depth-wise up-sampling (cp_conv_transpose2d_dw_nhwc): x [B,H,W,C] NHWC, w [C,1,2f,2f] (ConvTranspose2d(C, C, 2f,
    stride=f, padding=f//2, groups=C) layout), add [B,fH,fW,C] or None -> add + up(x), [B,fH,fW,C] NHWC.  Float32."""
    L = lib()
    x, w = _dev(x), _dev(w)
    f = int(f)
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape) != (x.shape[3], 1, 2 * f, 2 * f):
        raise RuntimeError("conv_transpose2d_dw: x must be [B,H,W,C] and w [C,1,2f,2f], got %s and %s (f = %d)"
                           % (tuple(x.shape), tuple(w.shape), f))
    B, H, W, C = x.shape
    if add is not None:
        add = _dev(add)
        if tuple(add.shape) != (B, f * H, f * W, C):
            raise RuntimeError("conv_transpose2d_dw: add has shape %s, expected %s" % (tuple(add.shape), (B, f * H, f * W, C)))
    out = torch.empty(B, f * H, f * W, C, device=x.device, dtype=torch.float32)
    rc = L.cp_conv_transpose2d_dw_nhwc(_stream(), _ptr(x), _ptr(w), _ptr(add), _ptr(out), B, H, W, C, f)
    _check(rc, "cp_conv_transpose2d_dw_nhwc")
    return out


def conv_transpose2d_backward(x, w, grad_out, stride, pad, groups=1, need_x_grad=True):
    """Gradients of a bias-free ``ConvTranspose2d`` (cp_conv_transpose2d_backward_nhwc): x [B,H,W,Cin] NHWC, w [Cin,Cout/groups,K,K],
    grad_out [B,stride H,stride W,Cout] NHWC -> (grad_x [B,H,W,Cin] | None, grad_w like w).  Depth-wise (groups == Cin == Cout,
    stride 2 or 4, K = 2 stride, pad = stride / 2) or dense (groups 1, K 4, stride 2, pad 1).  Float32 and bitwise reproducible."""
    L = lib()
    x, w, grad_out = _dev(x), _dev(w), _dev(grad_out)
    stride, pad, groups = int(stride), int(pad), int(groups)
    if x.dim() != 4 or w.dim() != 4 or w.shape[0] != x.shape[3] or w.shape[2] != w.shape[3] or groups < 1:
        raise RuntimeError("conv_transpose2d_backward: x must be [B,H,W,Cin] and w [Cin,Cout/groups,K,K], got %s and %s"
                           % (tuple(x.shape), tuple(w.shape)))
    B, H, W, Cin = x.shape
    Cout, K = w.shape[1] * groups, w.shape[2]
    nbytes = L.cp_conv_transpose2d_backward_workspace_bytes(B, H, W, Cin, Cout, K, stride, pad, groups, int(bool(need_x_grad)))
    if nbytes == 0:
        raise RuntimeError("conv_transpose2d_backward: shape refused by the library (%s)" % L.cp_last_error().decode())
    if tuple(grad_out.shape) != (B, stride * H, stride * W, Cout):
        raise RuntimeError("conv_transpose2d_backward: grad_out has shape %s, expected %s"
                           % (tuple(grad_out.shape), (B, stride * H, stride * W, Cout)))
    grad_x = torch.empty_like(x) if need_x_grad else None
    grad_w = torch.empty_like(w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    rc = L.cp_conv_transpose2d_backward_nhwc(_stream(), _ptr(x), _ptr(w), _ptr(grad_out), _ptr(grad_x), _ptr(grad_w), B, H, W, Cin,
                                             Cout, K, stride, pad, groups, _ptr(ws), nbytes)
    _check(rc, "cp_conv_transpose2d_backward_nhwc")
    return grad_x, grad_w


def _pool_out(H, W, kernel, stride, pad):
    return (H + 2 * pad - kernel) // stride + 1, (W + 2 * pad - kernel) // stride + 1


def max_pool2d_forward(x, kernel, stride, pad):
    """``F.max_pool2d`` on an NHWC tensor (cp_maxpool2d_forward_nhwc): x [B,H,W,C] -> [B,Ho,Wo,C].  (kernel, stride, pad) is
    (2, 2, 0), which floors, or (3, 2, 1), padding as -inf; C % 4 == 0.  Bitwise torch's values."""
    x = _dev(x)
    if x.dim() != 4:
        raise RuntimeError("max_pool2d: x must be [B,H,W,C], got %s" % (tuple(x.shape),))
    B, H, W, C = x.shape
    kernel, stride, pad = int(kernel), int(stride), int(pad)
    Ho, Wo = _pool_out(H, W, kernel, stride, pad)
    out = torch.empty(B, max(Ho, 0), max(Wo, 0), C, device=x.device, dtype=torch.float32)
    _check(lib().cp_maxpool2d_forward_nhwc(_stream(), _ptr(x), _ptr(out), B, H, W, C, kernel, stride, pad),
           "cp_maxpool2d_forward_nhwc")
    return out


def max_pool2d_backward(x, grad_out, kernel, stride, pad):
    """Gradient of max_pool2d_forward (cp_maxpool2d_backward_nhwc): x [B,H,W,C], grad_out [B,Ho,Wo,C] -> grad_x [B,H,W,C].  The
    winner of every window is recomputed from x (torch's: the first maximum in row-major order); bitwise reproducible."""
    x, grad_out = _dev(x), _dev(grad_out)
    if x.dim() != 4:
        raise RuntimeError("max_pool2d_backward: x must be [B,H,W,C], got %s" % (tuple(x.shape),))
    B, H, W, C = x.shape
    kernel, stride, pad = int(kernel), int(stride), int(pad)
    Ho, Wo = _pool_out(H, W, kernel, stride, pad)
    if tuple(grad_out.shape) != (B, Ho, Wo, C):
        raise RuntimeError("max_pool2d_backward: grad_out has shape %s, expected %s" % (tuple(grad_out.shape), (B, Ho, Wo, C)))
    grad_x = torch.empty_like(x)
    _check(lib().cp_maxpool2d_backward_nhwc(_stream(), _ptr(x), _ptr(grad_out), _ptr(grad_x), B, H, W, C, kernel, stride, pad),
           "cp_maxpool2d_backward_nhwc")
    return grad_x


def conv2d_stem_backward(x, grad_out, stride=1, y=None, need_bias_grad=True):
    """Weight and bias gradient of a 7x7, padding-3 stem (cp_conv2d_stem_backward): x [B,Cin,H,W] NCHW planes with Cin in 1..3,
    grad_out [B,Ho,Wo,Cout] NHWC -> (grad_w [Cout,Cin,7,7], grad_bias [Cout] | None).  ``y``: the activated forward output when
    the layer ended in a ReLU (grad_out is gated by y > 0).  Float32 and bitwise reproducible; there is no input gradient."""
    L = lib()
    x, grad_out = _dev(x), _dev(grad_out)
    y = _dev(y) if y is not None else None
    if x.dim() != 4 or grad_out.dim() != 4:
        raise RuntimeError("conv2d_stem_backward: x must be [B,Cin,H,W] and grad_out [B,Ho,Wo,Cout], got %s and %s"
                           % (tuple(x.shape), tuple(grad_out.shape)))
    B, Cin, H, W = x.shape
    Cout, stride = grad_out.shape[3], int(stride)
    nbytes = L.cp_conv2d_stem_backward_workspace_bytes(B, H, W, Cin, Cout, stride)
    if nbytes == 0:
        raise RuntimeError("conv2d_stem_backward: shape refused by the library (%s)" % L.cp_last_error().decode())
    want = (B, (H - 1) // stride + 1, (W - 1) // stride + 1, Cout)
    for name, t in (("grad_out", grad_out), ("y", y)):
        if t is not None and tuple(t.shape) != want:
            raise RuntimeError("conv2d_stem_backward: %s has shape %s, expected %s" % (name, tuple(t.shape), want))
    grad_w = torch.empty(Cout, Cin, 7, 7, device=x.device, dtype=torch.float32)
    grad_b = torch.empty(Cout, device=x.device, dtype=torch.float32) if need_bias_grad else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    rc = L.cp_conv2d_stem_backward(_stream(), _ptr(x), _ptr(grad_out), _ptr(y), _ptr(grad_w), _ptr(grad_b), _ptr(ws), nbytes,
                                   B, H, W, Cin, Cout, stride)
    _check(rc, "cp_conv2d_stem_backward")
    return grad_w, grad_b


PRECISIONS = {"f32": 0, "f16x3": 1}


def set_default_precision(name):
    """'f32' (exact float32 MFMA) or 'f16x3' (split-binary16 MFMA, float32-class accuracy)."""
    _check(lib().cp_set_default_precision(PRECISIONS[name]), "cp_set_default_precision")


DET_FIELDS = OrderedDict([  # field -> (offset, width) inside a 118-float detection record (decode.py:347-361)
    ("bboxes", (0, 4)), ("scores", (4, 1)), ("kps", (5, 16)), ("clses", (21, 1)), ("obj_scale", (22, 3)),
    ("obj_scale_uncertainty", (25, 3)), ("tracking", (28, 2)), ("tracking_hp", (30, 16)),
    ("kps_displacement_mean", (46, 16)), ("kps_displacement_std", (62, 16)), ("kps_heatmap_mean", (78, 16)),
    ("kps_heatmap_std", (94, 16)), ("kps_heatmap_height", (110, 8))])
DET_STRIDE = 118


def decode_raw(hm, hps, wh, hm_hp, hps_uncertainty=None, scale=None, scale_uncertainty=None, reg=None,
               hp_offset=None, tracking=None, tracking_hp=None, K=100, rep_mode=1, fit_gaussian=False,
               balance=2.0, legacy_bool_mask=False, apply_sigmoid=False):
    """Device decode -> det [B,K,118] (device tensor).  hm / hm_hp are modified in place when
    apply_sigmoid is set.  Tensors must be contiguous float32 NCHW on the HIP device."""
    L = lib()
    for t in (hm, hps, wh, hm_hp):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise RuntimeError("decode: required heads must be contiguous float32 device tensors")
    opt = [None if t is None else _dev(t) for t in (hps_uncertainty, scale, scale_uncertainty, reg, hp_offset,
                                                    tracking, tracking_hp)]
    B, _, H, W = hm.shape
    det = torch.empty(B, K, DET_STRIDE, device=hm.device, dtype=torch.float32)
    n = L.cp_decode_workspace_bytes(B, K)
    ws = torch.empty(n, dtype=torch.uint8, device=hm.device)
    rc = L.cp_decode(_stream(), B, H, W, _ptr(hm), _ptr(hps), _ptr(wh), _ptr(opt[0]), _ptr(opt[1]), _ptr(opt[2]),
                     _ptr(opt[3]), _ptr(hm_hp), _ptr(opt[4]), _ptr(opt[5]), _ptr(opt[6]), int(K), int(rep_mode),
                     int(bool(fit_gaussian)), float(balance), int(bool(legacy_bool_mask)), int(bool(apply_sigmoid)),
                     _ptr(det), _ptr(ws), n)
    _check(rc, "cp_decode")
    return det


def decode_raw_tiled(hm, hps, wh, hm_hp, hps_uncertainty=None, scale=None, scale_uncertainty=None, reg=None,
                     hp_offset=None, tracking=None, tracking_hp=None, K=100, rep_mode=1, fit_gaussian=False,
                     balance=2.0, legacy_bool_mask=False, apply_sigmoid=False):
    """``decode_raw`` through cp_decode_tiled: the same records, bit for bit, for output grids of any size up to 1048576
    pixels (W % 4 == 0, W <= 4096, K <= 128).  The workspace grows with H*W and is sized here."""
    L = lib()
    for t in (hm, hps, wh, hm_hp):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise RuntimeError("decode_tiled: required heads must be contiguous float32 device tensors")
    opt = [None if t is None else _dev(t) for t in (hps_uncertainty, scale, scale_uncertainty, reg, hp_offset,
                                                    tracking, tracking_hp)]
    B, _, H, W = hm.shape
    n = L.cp_decode_tiled_workspace_bytes(B, H, W, int(K))
    if n == 0:
        raise RuntimeError("decode_tiled: unsupported shape B=%d H=%d W=%d K=%d (need 1 <= K <= 128, K <= H*W <= 1048576, "
                           "W %% 4 == 0, W <= 4096)" % (B, H, W, K))
    det = torch.empty(B, K, DET_STRIDE, device=hm.device, dtype=torch.float32)
    ws = torch.empty(n, dtype=torch.uint8, device=hm.device)
    rc = L.cp_decode_tiled(_stream(), B, H, W, _ptr(hm), _ptr(hps), _ptr(wh), _ptr(opt[0]), _ptr(opt[1]), _ptr(opt[2]),
                           _ptr(opt[3]), _ptr(hm_hp), _ptr(opt[4]), _ptr(opt[5]), _ptr(opt[6]), int(K), int(rep_mode),
                           int(bool(fit_gaussian)), float(balance), int(bool(legacy_bool_mask)), int(bool(apply_sigmoid)),
                           _ptr(det), _ptr(ws), n)
    _check(rc, "cp_decode_tiled")
    return det


def split_detections(det):
    """[B,K,118] -> dict of the 13 reference keys (views)."""
    return OrderedDict((k, det[..., o:o + w]) for k, (o, w) in DET_FIELDS.items())


def preprocess(image_u8_hwc, trans_input, mean, std, out_h, out_w):
    """Device warp + normalise of one BGR uint8 frame [H,W,3] -> float32 [1,3,out_h,out_w]
    (BaseDetector.pre_process, base_detector.py:127-134).  ``trans_input`` is the 2x3 source->input affine."""
    import numpy as np

    L = lib()
    if not (image_u8_hwc.is_cuda and image_u8_hwc.dtype == torch.uint8 and image_u8_hwc.is_contiguous()):
        raise RuntimeError("preprocess: image must be a contiguous uint8 device tensor [H,W,3]")
    H, W = int(image_u8_hwc.shape[0]), int(image_u8_hwc.shape[1])
    fwd = np.asarray(trans_input, np.float64).reshape(-1)
    f3 = ctypes.c_float * 3
    out = torch.empty(1, 3, out_h, out_w, device=image_u8_hwc.device, dtype=torch.float32)
    rc = L.cp_preprocess(_stream(), _ptr(image_u8_hwc), H, W, (ctypes.c_double * 6)(*fwd.tolist()),
                         f3(*[float(v) for v in np.asarray(mean).reshape(-1)]),
                         f3(*[float(v) for v in np.asarray(std).reshape(-1)]), _ptr(out), out_h, out_w)
    _check(rc, "cp_preprocess")
    return out


def preprocess_batch(images_u8_bhwc, trans_input, mean, std, out_h, out_w, out=None):
    """`preprocess` for B frames of one size sharing the transform: uint8 [B,H,W,3] -> float32 [B,3,out_h,out_w], one launch."""
    import numpy as np

    L = lib()
    t = images_u8_bhwc
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 4 and t.shape[3] == 3):
        raise RuntimeError("preprocess_batch: images must be a contiguous uint8 device tensor [B,H,W,3]")
    B, H, W = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    fwd = np.asarray(trans_input, np.float64).reshape(-1)
    f3 = ctypes.c_float * 3
    if out is None:
        out = torch.empty(B, 3, out_h, out_w, device=t.device, dtype=torch.float32)
    rc = L.cp_preprocess_batch(_stream(), _ptr(t), B, H, W, (ctypes.c_double * 6)(*fwd.tolist()),
                               f3(*[float(v) for v in np.asarray(mean).reshape(-1)]),
                               f3(*[float(v) for v in np.asarray(std).reshape(-1)]), _ptr(out), out_h, out_w)
    _check(rc, "cp_preprocess_batch")
    return out


def resize_u8(image_u8_hwc, out_h, out_w):
    """cv2.resize(img, (out_w, out_h)) (INTER_LINEAR, OpenCV's fixed-point form) of a uint8 [H,W,C] device frame."""
    L = lib()
    if not (image_u8_hwc.is_cuda and image_u8_hwc.dtype == torch.uint8 and image_u8_hwc.is_contiguous()
            and image_u8_hwc.dim() == 3):
        raise RuntimeError("resize_u8: image must be a contiguous uint8 device tensor [H,W,C]")
    H, W, C = (int(v) for v in image_u8_hwc.shape)
    out = torch.empty(out_h, out_w, C, device=image_u8_hwc.device, dtype=torch.uint8)
    _check(L.cp_resize_u8(_stream(), _ptr(image_u8_hwc), H, W, C, _ptr(out), out_h, out_w), "cp_resize_u8")
    return out


def render_gaussians(records, C, H, W, device, out=None):
    """Draw (channel, x, y, radius, k) Gaussians into a float32 [C,H,W] device map with max() merging
    (draw_umich_gaussian, utils/image.py:135-150): the pre_hm / pre_hm_hp render of CenterPoseTrack."""
    L = lib()
    rec = torch.as_tensor(records, dtype=torch.float64).reshape(-1, 5).contiguous().to(device)
    if out is None:
        out = torch.empty(C, H, W, dtype=torch.float32, device=device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (C, H, W)):
        raise RuntimeError("render_gaussians: out must be a contiguous float32 device tensor [C,H,W]")
    _check(L.cp_render_gaussians(_stream(), _ptr(rec) if rec.numel() else None, int(rec.shape[0]), _ptr(out), C, H, W,
                                 1), "cp_render_gaussians")
    return out


POST_STRIDE = 120
POST_FIELDS = OrderedDict([  # field -> (offset, width) inside a post-processed record (post_process.py:21-58)
    ("score", (0, 1)), ("cls", (1, 1)), ("obj_scale", (2, 3)), ("obj_scale_uncertainty", (5, 3)),
    ("kps_displacement_std", (8, 16)), ("bbox", (24, 4)), ("ct", (28, 2)), ("kps", (30, 16)), ("tracking", (46, 2)),
    ("tracking_hp", (48, 16)), ("kps_displacement_mean", (64, 16)), ("kps_heatmap_mean", (80, 16)),
    ("kps_heatmap_std", (96, 16)), ("kps_heatmap_height", (112, 8))])


def postprocess(det, meta, vis_thresh, nms=True, div_scale=1.0, out=None, cnt=None, ws=None):
    """Device post-process + Gaussian soft-NMS of a whole batch (object_pose.py:167-197).
    det [B,K,118] float32 device; meta [B,8] float64 (inverse affine 6, ratio, pad) -> (records [B,K,120] float64
    device, counts [B] int32 device); image b keeps records[b, :counts[b]] in the reference's final order.
    ``out`` / ``cnt`` / ``ws``: caller-owned result and workspace tensors (PoseStage rotates its own)."""
    L = lib()
    if not (det.is_cuda and det.dtype == torch.float32 and det.is_contiguous() and det.dim() == 3
            and det.shape[2] == DET_STRIDE):
        raise RuntimeError("postprocess: det must be a contiguous float32 device tensor [B,K,118]")
    B, K = int(det.shape[0]), int(det.shape[1])
    meta = torch.as_tensor(meta, dtype=torch.float64).reshape(B, 8).contiguous().to(det.device)
    if out is None:
        out = torch.empty(B, K, POST_STRIDE, dtype=torch.float64, device=det.device)
    if cnt is None:
        cnt = torch.empty(B, dtype=torch.int32, device=det.device)
    n = L.cp_postprocess_workspace_bytes(B, K)
    if ws is None:
        ws = torch.empty(n, dtype=torch.uint8, device=det.device)
    if tuple(out.shape) != (B, K, POST_STRIDE) or out.dtype != torch.float64 or cnt.numel() != B or ws.numel() < n:
        raise RuntimeError("postprocess: out / cnt / ws do not fit this batch")
    rc = L.cp_postprocess(_stream(), _ptr(det), B, K, _ptr(meta), float(vis_thresh), int(bool(nms)), float(div_scale),
                          _ptr(out), _ptr(cnt), _ptr(ws), n)
    _check(rc, "cp_postprocess")
    return out, cnt


PNP_STRIDE = 40


def pnp_solve(pts, scale, cam):
    """Batched cuboid PnP.  pts [N,npts,2] float32 (npts 8 or 16), scale [N,3] float32, cam [N,4] float64
    (fx, fy, cx, cy); all on the HIP device.  Returns out [N,40] float64 (layout: centerpose_hip.h)."""
    L = lib()
    if not (pts.is_cuda and scale.is_cuda and cam.is_cuda):
        raise RuntimeError("pnp_solve: tensors must live on the HIP device (no CPU path)")
    pts = pts.contiguous().float()
    scale = scale.contiguous().float()
    cam = cam.contiguous().double()
    N, npts = pts.shape[0], pts.shape[1]
    out = torch.zeros(N, PNP_STRIDE, device=pts.device, dtype=torch.float64)
    if N == 0:
        return out
    n = L.cp_pnp_workspace_bytes(N)
    ws = torch.empty(n, dtype=torch.uint8, device=pts.device)
    _check(L.cp_pnp_solve(_stream(), _ptr(pts), _ptr(scale), _ptr(cam), N, npts, _ptr(out), _ptr(ws), n),
           "cp_pnp_solve")
    return out


_pnp_ws_cache = {}


def pnp_from_post(post, count, cam, rep_mode=1, out=None, ws=None):
    """PnP of every post-processed slot on the device (cp_pnp_from_post): post [B,K,120] float64 + count [B] int32 from
    ``postprocess``, cam [B,4] float64 (fx, fy, cx, cy).  Returns [B,K,40] float64; rows k >= count[b] carry status -1.
    No host synchronisation.  ``out`` / ``ws``: caller-owned result and workspace (default: a fresh result and one
    cached workspace per (shape, device, stream) -- launches on the same stream are ordered, so they may share it)."""
    L = lib()
    B, K = int(post.shape[0]), int(post.shape[1])
    if not (post.is_cuda and post.dtype == torch.float64 and post.is_contiguous() and count.is_cuda and cam.is_cuda):
        raise RuntimeError("pnp_from_post: contiguous device tensors expected (no CPU path)")
    cam = cam.contiguous().double().reshape(B, 4)
    if out is None:
        out = torch.empty(B, K, PNP_STRIDE, dtype=torch.float64, device=post.device)
    n = L.cp_pnp_from_post_workspace_bytes(B, K)
    if ws is None:
        key = (B, K, post.device, torch.cuda.current_stream(post.device).cuda_stream)
        ws = _pnp_ws_cache.get(key)
        if ws is None:
            if len(_pnp_ws_cache) >= 16:
                _pnp_ws_cache.clear()
            ws = _pnp_ws_cache[key] = torch.empty(n, dtype=torch.uint8, device=post.device)
    if tuple(out.shape) != (B, K, PNP_STRIDE) or out.dtype != torch.float64 or ws.numel() < n:
        raise RuntimeError("pnp_from_post: out / ws do not fit this batch")
    _check(L.cp_pnp_from_post(_stream(), _ptr(post), _ptr(count), B, K, int(rep_mode), _ptr(cam), _ptr(out), _ptr(ws), n),
           "cp_pnp_from_post")
    return out


_masked_streams = {}   # (device index, n_cus) -> (handle, torch stream): ONE stream per mask for the life of the process (every
                       # hipExtStreamCreateWithCUMask is a hardware queue of its own; a process that kept creating them would
                       # push its other streams onto shared queues)


BOX_EVAL_STRIDE = 9  # CP_BOX_EVAL_STRIDE
BOX_EVAL_FIELDS = ("iou", "add", "adds", "azimuth", "polar", "pixel", "best3d", "best2d", "flags")
BOX_FLAG_SINGULAR_RAY, BOX_FLAG_SINGULAR_MO2C, BOX_FLAG_CLIP_OVERFLOW = 1, 2, 4


def _box_upload(arrays, device):
    """(array, shape, dtype) host arrays (numpy or CPU tensors) -> typed views of ONE device byte buffer, filled by one
    host-to-device copy: each array's bytes go in at a 16-byte aligned offset and come back out as a tensor of its own
    dtype (``Tensor.view(dtype)`` reinterprets, it does not convert).  Device tensors are used in place."""
    import numpy as np

    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out, host, total = [None] * len(arrays), [], 0
    for i, (a, shape, dt) in enumerate(arrays):
        if isinstance(a, torch.Tensor) and a.is_cuda:
            t = a.to(getattr(torch, np.dtype(dt).name)).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError("box metrics: expected shape %s, got %s" % (shape, tuple(t.shape)))
            out[i] = t
            continue
        h = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dt)
        if h.shape != shape:
            raise ValueError("box metrics: expected shape %s, got %s" % (shape, h.shape))
        host.append((i, h, total))
        total += (h.nbytes + 15) // 16 * 16
    if host:
        buf = np.zeros(total, np.uint8)
        for _, h, o in host:
            buf[o:o + h.nbytes] = h.reshape(-1).view(np.uint8)
        dbuf = torch.from_numpy(buf).to(dev)
        for i, h, o in host:
            out[i] = dbuf[o:o + h.nbytes].view(getattr(torch, h.dtype.name)).view(h.shape)
    return out, dev


def box_iou(a, b, device=None):
    """cp_box_iou: IoU3D.IoU(Box(a[i]), Box(b[i])).iou() of the reference evaluator for every pair; a, b [N,9,3] float64
    (numpy or tensors) -> numpy float64 [N]."""
    import numpy as np

    n = int(np.shape(a)[0])
    if n == 0:
        return np.zeros(0)
    f8 = np.float64
    (da, db), dev = _box_upload([(a, (n, 9, 3), f8), (b, (n, 9, 3), f8)], device)
    iou = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _check(lib().cp_box_iou(_stream(), _ptr(da), _ptr(db), n, _ptr(iou)), "cp_box_iou")
        return iou.cpu().numpy()


def box_eval(pred3d, gt3d, pred2d, mo2c, proj, single_rotation=None, num_symmetry=1, device=None):
    """cp_box_eval: evaluate_3d + evaluate_2d of the reference evaluator for N matched pairs in one launch.
    pred3d, gt3d [N,9,3], pred2d [N,9,2], mo2c, proj [N,4,4] float64; single_rotation [N] (nonzero: index 0 only, the mug
    break).  Returns numpy float64 [N, BOX_EVAL_STRIDE], columns BOX_EVAL_FIELDS."""
    import numpy as np

    n = int(np.shape(pred3d)[0])
    if n == 0:
        return np.zeros((0, BOX_EVAL_STRIDE))
    if num_symmetry < 1:
        raise ValueError("box_eval: num_symmetry must be >= 1")
    single = np.zeros(n, np.int32) if single_rotation is None else np.asarray(single_rotation).astype(np.int32)
    if single.shape != (n,):
        raise ValueError("box_eval: single_rotation must have shape (%d,)" % n)
    f8 = np.float64
    bufs, dev = _box_upload([(pred3d, (n, 9, 3), f8), (gt3d, (n, 9, 3), f8), (pred2d, (n, 9, 2), f8),
                             (mo2c, (n, 4, 4), f8), (proj, (n, 4, 4), f8), (single, (n,), np.int32)], device)
    out = torch.empty((n, BOX_EVAL_STRIDE), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _check(lib().cp_box_eval(_stream(), *[_ptr(t) for t in bufs], n, int(num_symmetry), _ptr(out)), "cp_box_eval")
        return out.cpu().numpy()


def masked_stream(device, n_cus):
    """A HIP stream whose kernels may only run on the first ``n_cus`` compute units (hipExtStreamCreateWithCUMask; bits are spread
    over the XCDs by the runtime), wrapped as a torch stream.  For latency-bound side work that must not take registers away from
    the kernels of the main stream everywhere on the chip: the batched PnP solve holds 286 - 330 vector registers per wavefront
    -- one such wave takes more than half of a SIMD's register file for the ~0.5 ms of its Levenberg-Marquardt walk, and a few
    hundred of them spread over all 1024 SIMDs cost the network kernels they overlap ~0.3 ms per step (profiles/NOTES.md round 6)."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(n_cus))
    if key in _masked_streams:
        return _masked_streams[key][1]
    rt = ctypes.CDLL("libamdhip64.so")
    words = (int(n_cus) + 31) // 32
    mask = (ctypes.c_uint32 * words)()
    for i in range(int(n_cus)):
        mask[i // 32] |= 1 << (i % 32)
    h = ctypes.c_void_p()
    with torch.cuda.device(dev):
        rc = rt.hipExtStreamCreateWithCUMask(ctypes.byref(h), ctypes.c_uint32(words), mask)
    if rc != 0 or not h.value:
        raise RuntimeError("hipExtStreamCreateWithCUMask failed with code %d" % rc)
    st = torch.cuda.ExternalStream(h.value, device=dev)
    _masked_streams[key] = (h, st)
    return st


class PoseStage(object):
    """Post-process + soft-NMS + batched PnP of decoded batches (base_detector.py:547-654 for a whole batch), with the
    PnP -- and, from 8 images per batch, the post-process -- on a side stream.  The solve is at most B*K independent float64 problems of ~1e5 operations each: a few dozen
    wavefronts whose run time is the slowest lane's Levenberg-Marquardt walk (0.5 - 2.5 ms), during which the rest of
    the chip would idle.  ``submit`` therefore queues the solve (and the post-process of a batch of 8 or more, behind a copy of the
    decoded records) on the stage's own stream, so that the solve of batch i runs under the network of batch i+1; ``depth`` sets of result buffers
    rotate, and the caller's stream waits for the solve that last used a set before post-process overwrites it.

    submit() -> (post [B,K,120], count [B], poses [B,K,40], done): the tensors are valid once ``done`` (a
    torch.cuda.Event) has completed -- ``done.synchronize()`` on the host or ``stream.wait_event(done)``.
    Caller-owned inputs (``det``, ``meta``, ``cam``) are read on the side stream as well: the stage tells the caching
    allocator (``record_stream``), so the caller may drop them right after ``submit``."""

    # batches of at least this many images post-process on the side stream too (below: on the caller's, one hop less per frame);
    # $CP_POST_SIDE_FROM overrides (A/B runs)
    SIDE_POST_FROM = int(os.environ.get("CP_POST_SIDE_FROM", "8"))

    def __init__(self, B, K, device, depth=2, cus=None):
        """``cus``: run the solve on a stream restricted to that many compute units (``masked_stream``); None = $CP_PNP_CUS or,
        unset, 32 (B = 64, 1650 mostly ill-posed detections per batch, profiles/r06_pnp_cu_mask_ab.txt: the first layers of the
        next batch, which the solve overlaps, 1.60 -> 1.45 ms, step 18.74 -> 18.63 ms with the longer solve's tail included; 8 / 16
        CUs stretch the solve to 5.4 / 3.4 ms and lose); 0 = an ordinary stream (the solve's waves land on every CU)."""
        L = lib()
        self.B, self.K, self.depth, self.i = int(B), int(K), int(depth), 0
        if cus is None:
            cus = int(os.environ.get("CP_PNP_CUS", "32"))
        self.cus = int(cus)
        self.side = None
        if self.cus > 0:
            try:
                self.side = masked_stream(device, self.cus)
            except (RuntimeError, OSError, AttributeError):   # runtime without the extension: an ordinary stream does the same work
                self.cus = 0
        if self.side is None:
            self.side = torch.cuda.Stream(device=device)
        n_post, n_pnp = L.cp_postprocess_workspace_bytes(B, K), L.cp_pnp_from_post_workspace_bytes(B, K)
        self.sets = []
        for _ in range(self.depth):
            self.sets.append(dict(
                post=torch.empty(B, K, POST_STRIDE, dtype=torch.float64, device=device),
                cnt=torch.empty(B, dtype=torch.int32, device=device),
                poses=torch.empty(B, K, PNP_STRIDE, dtype=torch.float64, device=device),
                det=torch.empty(B, K, DET_STRIDE, dtype=torch.float32, device=device),
                meta=torch.empty(B, 8, dtype=torch.float64, device=device),
                ws_post=torch.empty(n_post, dtype=torch.uint8, device=device),
                ws_pnp=torch.empty(n_pnp, dtype=torch.uint8, device=device),
                ready=torch.cuda.Event(), done=torch.cuda.Event(enable_timing=True),
                begin=torch.cuda.Event(enable_timing=True)))
        self._timed = []

    def submit(self, det, meta, cam, vis_thresh, nms=True, rep_mode=1):
        s = self.sets[self.i % self.depth]
        first_use = self.i < self.depth
        self.i += 1
        main = torch.cuda.current_stream()
        if not first_use:
            main.wait_event(s["done"])  # the post-process / solve that read this set `depth` batches ago
        B = int(det.shape[0])
        side_post = B >= self.SIDE_POST_FROM
        if side_post:
            # the post-process (one latency-bound launch of ~0.15 ms at B = 64: a serial soft-NMS walk per image) joins the solve on the
            # side stream; the caller's stream only copies the decoded records (3 MB) and the per-image affine into the set, so the
            # caller may overwrite `det` / `meta` with the next batch at once
            s["det"][:B].copy_(det, non_blocking=True)
            s["meta"][:B].copy_(torch.as_tensor(meta, dtype=torch.float64).reshape(B, 8).to(det.device), non_blocking=True)
        else:
            postprocess(det, meta, vis_thresh, nms=nms, out=s["post"], cnt=s["cnt"], ws=s["ws_post"])
        s["ready"].record(main)
        if torch.is_tensor(cam) and cam.is_cuda:
            cam.record_stream(self.side)  # read by the solve after this call returns
        with torch.cuda.stream(self.side):
            self.side.wait_event(s["ready"])
            s["begin"].record(self.side)
            if side_post:
                postprocess(s["det"][:B], s["meta"][:B], vis_thresh, nms=nms, out=s["post"], cnt=s["cnt"], ws=s["ws_post"])
            pnp_from_post(s["post"], s["cnt"], cam, rep_mode=rep_mode, out=s["poses"], ws=s["ws_pnp"])
            s["done"].record(self.side)
        self._timed = [(s["begin"], s["done"])]
        return s["post"], s["cnt"], s["poses"], s["done"]

    def take_solve_ms(self):
        """Milliseconds the most recent assembly + solve took on the side stream (synchronises on it); None before the
        first submit."""
        if not self._timed:
            return None
        b, d = self._timed[-1]
        d.synchronize()
        return b.elapsed_time(d)


TRACK_STRIDE = 520
TRACK_CAP = 128
TRACK_FIELDS = OrderedDict([  # field -> (offset, width) inside a device track record (include/centerpose_hip.h)
    ("tracking_id", (0, 1)), ("age", (1, 1)), ("active", (2, 1)), ("flags", (3, 1)), ("post", (4, 120)),
    ("kps_fusion_mean", (124, 16)), ("kps_fusion_std", (140, 16)), ("location", (156, 3)), ("quaternion_xyzw", (159, 4)),
    ("projected_cuboid", (163, 16)), ("kps_pnp", (179, 18)), ("kps_3d_cam", (197, 27)), ("kps_ori", (224, 18)),
    ("kf_x", (242, 32)), ("kf_P", (274, 128)), ("kps_mean_kf", (409, 16)), ("kps_std_kf", (425, 16)),
    ("obj_scale_kf", (441, 3)), ("obj_scale_uncertainty_kf", (444, 3)), ("conf", (447, 8)), ("kps_pnp_kf", (455, 18)),
    ("kps_3d_cam_kf", (473, 27)), ("kps_ori_kf", (500, 18))])


SEED_STRIDE = 234
SEED_PRESENT = 233  # presence bits of a seed record: 1 ct, 2 kps_gt, 4 kps_pnp / kps_3d_cam, 8 kps_ori
SEED_FIELDS = OrderedDict(  # field -> (offset, width) inside a seed record (include/centerpose_hip.h: cp_track_seed)
    list(POST_FIELDS.items()) + [("kps_fusion_mean", (120, 16)), ("kps_fusion_std", (136, 16)), ("kps_pnp", (152, 18)),
                                 ("kps_3d_cam", (170, 27)), ("kps_ori", (197, 18)), ("kps_gt", (215, 18))])


def seed_required_keys(params, gt=False):
    """The keys of a seed dict that the configured mode reads: the host tracker would raise a KeyError on a seed without one
    (`init_track` / `init_kf`, the association and read-out of its first frame, the branch of `_get_additional_inputs`
    that draws it)."""
    keys = ["score", "bbox", "cls", "kps"]
    if params.kalman:
        keys += ["kps_fusion_mean", "kps_fusion_std", "tracking_hp"]
    if params.scale_pool:
        keys += ["obj_scale", "obj_scale_uncertainty"]
    if params.pre_hm_hp:
        if gt:
            keys.append("kps_gt")
        elif params.use_pnp and params.render_hmhp_mode in (0, 1):
            keys.append("kps_ori")
    return keys


def pack_seeds(pre_dets_per_video, params, gt_render=None, S=None):
    """The reference's seed dicts (``meta['pre_dets']``, tools/objectron_eval/eval_video_official.py:430-449; 'ct' optional)
    -> (seeds float64 [B, S, SEED_STRIDE], counts int32 [B]) for ``DeviceTracker.seed``, one numpy conversion per field.
    ``pre_dets_per_video[b]`` is the list of video b, or None for a video that is not seeded now (count -1: left untouched);
    an empty list resets the video.
    ``gt_render[b]`` says whether video b's previous-frame maps are the ground-truth ones (it decides which keys are needed).
    The dicts are only read -- the host tracker's ``init_track`` writes into them, and the evaluator hands the same dicts
    to the next frame.  A seed that lacks a key the configured mode needs raises KeyError naming it, before anything is
    copied."""
    import numpy as np

    B = len(pre_dets_per_video)
    gt = [False] * B if gt_render is None else [bool(g) for g in gt_render]
    for b, dets in enumerate(pre_dets_per_video):
        for i, d in enumerate(dets or ()):
            for k in seed_required_keys(params, gt[b]):
                if k not in d:
                    raise KeyError("pack_seeds: seed %d of video %d has no '%s'" % (i, b, k))
    n_max = max([len(d) for d in pre_dets_per_video if d is not None] + [1])
    S = n_max if S is None else int(S)
    if not 1 <= S <= TRACK_CAP or n_max > S:
        raise ValueError("pack_seeds: %d seeds in one video, S = %d (at most %d)" % (n_max, S, TRACK_CAP))
    seeds = np.zeros((B, S, SEED_STRIDE))
    counts = np.array([-1 if d is None else len(d) for d in pre_dets_per_video], np.int32)
    flat = [d for dets in pre_dets_per_video for d in (dets or ())]
    if flat:
        vb = np.repeat(np.arange(B), np.maximum(counts, 0))
        vi = np.concatenate([np.arange(max(n, 0)) for n in counts])
        for k, (off, w) in SEED_FIELDS.items():   # one stacked conversion per field
            have = [k in d for d in flat]
            if all(have):
                try:
                    seeds[vb, vi, off:off + w] = np.asarray([d[k] for d in flat], np.float64).reshape(len(flat), w)
                    continue
                except ValueError:   # the seeds give this field in different shapes: one by one
                    pass
            if any(have):
                for j, d in enumerate(flat):
                    if have[j]:
                        seeds[vb[j], vi[j], off:off + w] = np.asarray(d[k], np.float64).reshape(-1)
        seeds[vb, vi, SEED_PRESENT] = [1 * ("ct" in d) + 2 * ("kps_gt" in d) + 4 * ("kps_pnp" in d and "kps_3d_cam" in d)
                                       + 8 * ("kps_ori" in d) for d in flat]
    return seeds, counts


def track_params_from_opt(opt, K=100, cap=TRACK_CAP):
    """cp_track_params for a reference ``opt`` (opts.py:242-300); raises for what only the host tracker does.  The ground-truth /
    empty previous-frame maps (--gt_pre_hm_hmhp, --gt_pre_hm_hmhp_first, --empty_pre_hm) are no fields of the struct: they
    decide per frame and video what ``BatchedTracking`` seeds and renders (``DeviceTracker.seed``)."""
    baseline = bool(getattr(opt, "refined_Kalman", False))  # Tracker_baseline wins when both flags are set (base_detector.py:53-57)
    if not (getattr(opt, "tracking_task", False) or baseline) or not (opt.kalman or opt.scale_pool):
        raise RuntimeError("device tracker: tracking_task or refined_Kalman, with kalman and / or scale_pool (demo.py:117-129)")
    cat = {"camera": 0, "bottle": 0, "cup": 0, "book": 1, "chair": 1, "cereal_box": 1, "bike": 2, "laptop": 2, "shoe": 2}
    lo, hi = opt.conf_border[opt.c][0], opt.conf_border[opt.c][1]
    return TrackParams(new_thresh=opt.new_thresh, pre_thresh=opt.pre_thresh, R=opt.R, conf_lo=lo, conf_hi=hi,
                       max_age=int(opt.max_age), kalman=int(bool(opt.kalman)), scale_pool=int(bool(opt.scale_pool)),
                       use_pnp=int(bool(opt.use_pnp)), hps_uncertainty=int(bool(opt.hps_uncertainty)),
                       show_axes=int(bool(opt.show_axes)), cat_rule=cat[opt.c], render_hm_mode=int(opt.render_hm_mode),
                       render_hmhp_mode=int(opt.render_hmhp_mode), pre_hm=int(bool(opt.pre_hm)),
                       pre_hm_hp=int(bool(opt.pre_hm_hp)), K=int(K), cap=int(cap),
                       hungarian=(2 if getattr(opt, "hungarian_solver", "munkres") == "scipy" else 1) if getattr(opt, "hungarian", False) else 0,
                       baseline=int(baseline))


def track_vmeta(metas):
    """[B,16] float64 rows of cp_track_step from the ``meta`` dicts of ``pre_process`` (+ 'camera_matrix')."""
    import numpy as np

    v = np.zeros((len(metas), 16))
    for b, m in enumerate(metas):
        v[b, 0:6] = np.asarray(m["trans_input"], np.float64).reshape(-1)
        v[b, 6:10] = [m["width"], m["height"], m["inp_width"], m["inp_height"]]
        if "camera_matrix" in m:
            K = np.asarray(m["camera_matrix"], np.float64)
            v[b, 10:14] = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    return v


class DeviceTracker(object):
    """CenterPoseTrack's per-video track tables on the device (cp_track_*): ``step`` consumes the outputs of
    ``postprocess`` / ``pnp_from_post`` of a frame of B videos, ``render`` draws the next frame's pre_hm / pre_hm_hp from
    the tracks, ``read`` copies the current lists to the host, ``seed`` replaces the lists of chosen videos by tracks made from
    annotations (and can leave their ground-truth Gaussians for the next ``render``).  ``read`` synchronises; so does ``step`` once every
    ``STATUS_EVERY`` frames, when it looks at the overflow counters (``check``) and raises if a frame needed more than ``cap``
    tracks -- AFTER the device state has advanced by that frame.  Set ``STATUS_EVERY = 0`` (class or instance attribute) for a
    loop that must never synchronise or that is being captured into a hipGraph, and poll ``dropped()`` / ``check()`` yourself."""

    STATUS_EVERY = 64  # frames between two looks at the overflow counters in step() (each look synchronises the stream); 0 = never

    def __init__(self, B, params, vmeta, device, inp_h, inp_w):
        L = lib()
        self.frames = 0
        self.B, self.P, self.device = int(B), params, device
        self.K, self.cap = int(params.K), int(params.cap)
        self.inp_h, self.inp_w = int(inp_h), int(inp_w)
        self.vmeta = torch.as_tensor(vmeta, dtype=torch.float64).reshape(self.B, 16).contiguous().to(device)
        n_state, n_ws = L.cp_track_state_bytes(self.B, self.cap), L.cp_track_workspace_bytes(self.B, self.K, self.cap)
        if n_state == 0 or n_ws == 0:
            raise RuntimeError("DeviceTracker: unsupported B / K / cap")
        self.state = torch.empty(n_state, dtype=torch.uint8, device=device)
        self.ws = torch.empty(n_ws, dtype=torch.uint8, device=device)
        self.recs = torch.empty(self.B, self.cap, 9, 5, dtype=torch.float64, device=device)
        self.planes = torch.empty(9 * self.B, self.inp_h, self.inp_w, dtype=torch.float32, device=device)
        self.hdr_bytes = ((4 + 4 * self.B) * 4 + 255) // 256 * 256
        self._seed_ring, self._seed_calls, self._seed_dev = [], 0, None   # staging of seed()
        self.reset()

    def reset(self):
        _check(lib().cp_track_reset(_stream(), _ptr(self.state), self.B, self.cap), "cp_track_reset")
        self.recs[..., 0] = -1.0  # nothing to draw before the first frame
        self.recs[..., 1:] = 0.0

    def step(self, post, count, det_pnp=None, check=True):
        """One frame of every video.  Raises BEFORE the device state has moved if the arguments or the launch are refused;
        with ``check`` (default) the periodic look at the overflow counters follows and may raise AFTER it has moved -- a caller
        that keeps per-frame state of its own passes ``check=False``, updates that state, then calls ``check_due()``."""
        if not (post.is_cuda and post.dtype == torch.float64 and post.is_contiguous() and tuple(post.shape) ==
                (self.B, self.K, POST_STRIDE) and count.is_cuda and count.dtype == torch.int32):
            raise RuntimeError("DeviceTracker.step: post [B,K,120] float64 / count [B] int32 device tensors expected")
        if det_pnp is not None and not (det_pnp.is_cuda and det_pnp.dtype == torch.float64 and det_pnp.is_contiguous() and
                                        tuple(det_pnp.shape) == (self.B, self.K, PNP_STRIDE)):
            raise RuntimeError("DeviceTracker.step: det_pnp must be the [B,K,40] float64 output of pnp_from_post")
        _check(lib().cp_track_step(_stream(), ctypes.byref(self.P), _ptr(self.vmeta), _ptr(post), _ptr(count), _ptr(det_pnp),
                                   self.B, _ptr(self.state), _ptr(self.recs), _ptr(self.ws), self.ws.numel()), "cp_track_step")
        self.frames += 1
        if check:
            self.check_due()

    SEED_RING = 2  # pinned staging buffers of seed(): the host may run this many seed() calls ahead of the device

    def seed(self, seeds, counts, gt_render=None):
        """``Tracker.init_track`` with ``meta['pre_dets']`` for chosen videos, between two frames (cp_track_seed): ``seeds``
        float64 [B, S, SEED_STRIDE] and ``counts`` int32 [B] as ``pack_seeds`` builds them (count < 0: that video is left
        untouched; 0: reset to an empty list), ``gt_render`` [B] true where ``recs`` must hold the video's ground-truth
        Gaussians (--gt_pre_hm_hmhp / --gt_pre_hm_hmhp_first) instead of the ones drawn from the tracks.  One pinned
        host-to-device copy for all videos and one launch; no synchronisation (a staging buffer is re-used only once the
        copy made from it ``SEED_RING`` calls ago has left the host).  Raises BEFORE the device state has moved."""
        import numpy as np

        seeds = np.ascontiguousarray(seeds, np.float64)
        counts = np.ascontiguousarray(counts, np.int32)
        if seeds.ndim != 3 or seeds.shape[0] != self.B or seeds.shape[2] != SEED_STRIDE or not 1 <= seeds.shape[1] <= TRACK_CAP:
            raise RuntimeError("DeviceTracker.seed: seeds must be [B, S, %d] float64 with 1 <= S <= %d" % (SEED_STRIDE, TRACK_CAP))
        if counts.shape != (self.B,) or int(counts.max()) > seeds.shape[1]:
            raise RuntimeError("DeviceTracker.seed: counts must be [B] int32, none above S")
        gt = np.zeros(self.B, np.int32) if gt_render is None else np.ascontiguousarray(np.asarray(gt_render) != 0, np.int32)
        if gt.shape != (self.B,):
            raise RuntimeError("DeviceTracker.seed: gt_render must hold one flag per video")
        S = int(seeds.shape[1])
        n_seed = seeds.size * 8
        n_bytes = n_seed + 8 * self.B                     # seeds | counts int32 [B] | gt_render int32 [B]
        ring = self._seed_ring
        slot = self._seed_calls % self.SEED_RING
        if len(ring) <= slot:
            ring.append([None, None])
        if ring[slot][0] is None or ring[slot][0].numel() < n_bytes:
            ring[slot] = [torch.empty(max(n_bytes, 1 << 16), dtype=torch.uint8).pin_memory(), None]
        host, ev = ring[slot]
        if ev is not None:
            ev.synchronize()   # the copy out of this buffer, SEED_RING calls ago
        hv = host.numpy()
        hv[:n_seed].view(np.float64)[:] = seeds.reshape(-1)
        hv[n_seed:n_seed + 4 * self.B].view(np.int32)[:] = counts
        hv[n_seed + 4 * self.B:n_bytes].view(np.int32)[:] = gt
        dev = self._seed_dev
        if dev is None or dev.numel() < n_bytes:
            dev = self._seed_dev = torch.empty(max(n_bytes, 1 << 16), dtype=torch.uint8, device=self.device)
        dev[:n_bytes].copy_(host[:n_bytes], non_blocking=True)
        ring[slot][1] = torch.cuda.Event()
        ring[slot][1].record()
        self._seed_calls += 1
        p = dev.data_ptr()
        _check(lib().cp_track_seed(_stream(), ctypes.byref(self.P), _ptr(self.vmeta), p, p + n_seed, p + n_seed + 4 * self.B,
                                   self.B, S, _ptr(self.state), _ptr(self.recs)), "cp_track_seed")

    def check_due(self):
        """The periodic overflow check of ``step`` (every STATUS_EVERY frames; synchronises when it runs)."""
        if self.STATUS_EVERY and self.frames % self.STATUS_EVERY == 0:  # the device-resident loop never calls read(): surface overflows here
            self.check()

    def dropped(self):
        """Per video: list entries dropped so far because a frame needed more than `cap` tracks (cp_track_status; the
        tracker then keeps the first `cap` entries in the reference's order -- matched, new by score, coasting)."""
        out = (ctypes.c_int * self.B)()
        _check(lib().cp_track_status(_stream(), _ptr(self.state), self.B, out), "cp_track_status")
        return list(out)

    def check(self):
        d = self.dropped()
        if any(d):
            raise RuntimeError("DeviceTracker: more than cap = %d tracks in a frame of video(s) %s (entries dropped: %s); "
                               "raise cap or the thresholds" % (self.cap, [b for b, v in enumerate(d) if v], [v for v in d if v]))

    def render(self):
        """-> (pre_hm [B,1,H,W], pre_hm_hp [B,8,H,W]) drawn from the current tracks (views of one plane buffer)."""
        B, H, W = self.B, self.inp_h, self.inp_w
        _check(lib().cp_render_gaussians(_stream(), _ptr(self.recs), B * self.cap * 9, _ptr(self.planes), 9 * B, H, W, 1),
               "cp_render_gaussians")
        return self.planes[:B].view(B, 1, H, W), self.planes[B:].view(B, 8, H, W)

    def read(self):
        """Host copy of the current lists: a list of B float64 arrays [n_b, 520] (layout: TRACK_FIELDS)."""
        import numpy as np

        raw = self.state.cpu().numpy()
        hdr = raw[: (4 + 4 * self.B) * 4].view(np.int32)
        tr = raw[self.hdr_bytes:].view(np.float64).reshape(2, self.B, self.cap, TRACK_STRIDE)
        out = []
        for b in range(self.B):
            n, overflow = int(hdr[4 + 4 * b]), int(hdr[4 + 4 * b + 2])
            if overflow:
                raise RuntimeError("DeviceTracker: video %d needed more than %d tracks (%d list entries dropped)" % (b, self.cap, overflow))
            out.append(tr[int(hdr[0]), b, :n].copy())
        return out


def track_record_to_dict(r, opt=None):
    """One device track record -> the reference's per-track dict (the keys `Tracker.step` leaves on a track)."""
    import numpy as np

    d = {}
    post = r[4:124]
    for k, (off, w) in POST_FIELDS.items():
        v = post[off:off + w]
        d[k] = float(v[0]) if k == "score" else int(v[0]) if k == "cls" else [v[0], v[1]] if k == "ct" else v.copy()
    flags = int(r[3])
    d.update(tracking_id=int(r[0]), age=int(r[1]), active=int(r[2]))
    f = lambda k: r[TRACK_FIELDS[k][0]:TRACK_FIELDS[k][0] + TRACK_FIELDS[k][1]].copy()
    d["kps_fusion_mean"], d["kps_fusion_std"] = f("kps_fusion_mean"), f("kps_fusion_std")
    d["kps_mean_kf"], d["kps_std_kf"] = f("kps_mean_kf").reshape(8, 2), list(f("kps_std_kf"))
    d["obj_scale_kf"], d["obj_scale_uncertainty_kf"] = f("obj_scale_kf"), f("obj_scale_uncertainty_kf")
    if flags & 1:
        d["location"], d["quaternion_xyzw"] = list(f("location")), f("quaternion_xyzw")
        d["projected_cuboid"] = f("projected_cuboid").reshape(8, 2)
        d["kps_pnp"], d["kps_3d_cam"] = f("kps_pnp").reshape(9, 2), f("kps_3d_cam").reshape(9, 3)
    if flags & 8:
        d["kps_ori"] = f("kps_ori").reshape(9, 2)
    if flags & 2:
        d["kps_pnp_kf"], d["kps_3d_cam_kf"] = f("kps_pnp_kf").reshape(9, 2), f("kps_3d_cam_kf").reshape(9, 3)
        d["kps_ori_kf"] = f("kps_ori_kf").reshape(9, 2)
    d["in_boxes"] = bool(flags & 4)
    return d


# heads the decode reads at the peaks only (every head but the two heat-maps); hp_offset at the joint peaks, the rest at the centres
_MAP_HEADS = ("hm", "hm_hp")


def decode_peaks(hm, hm_hp, K=100, apply_sigmoid=False):
    """The first half of the decode (cp_decode_peaks): NMS + top-K of hm [B,1,H,W] and hm_hp [B,8,H,W] ->
    (pk_score float32 [B,9,K], pk_ind int32 [B,9,K]); index = y * W + x, map 0 = hm, 1..8 = hm_hp.  Any grid decode_raw or
    decode_raw_tiled accepts."""
    L = lib()
    hm, hm_hp = _dev(hm), _dev(hm_hp)
    B, _, H, W = hm.shape
    n = L.cp_decode_peaks_workspace_bytes(B, H, W, int(K))
    if n == 0:
        raise RuntimeError("cp_decode_peaks: unsupported shape")
    ws = torch.empty(n, dtype=torch.uint8, device=hm.device)
    pk_score = torch.empty(B, 9, K, device=hm.device, dtype=torch.float32)
    pk_ind = torch.empty(B, 9, K, device=hm.device, dtype=torch.int32)
    _check(L.cp_decode_peaks(_stream(), B, H, W, _ptr(hm), _ptr(hm_hp), int(K), int(bool(apply_sigmoid)), _ptr(pk_score),
                             _ptr(pk_ind), _ptr(ws), ws.numel()), "cp_decode_peaks")
    return pk_score, pk_ind


def decode_gathered(hm_hp, pk_score, pk_ind, hps, wh, hps_uncertainty=None, scale=None, scale_uncertainty=None, reg=None,
                    hp_offset=None, tracking=None, tracking_hp=None, rep_mode=1, fit_gaussian=False, balance=2.0,
                    legacy_bool_mask=False):
    """The second half of the decode on COMPACT tables (cp_decode_gathered): each regression head holds its values at the
    peaks only -- [B,C,K] at the centre peaks pk_ind[:, 0], hp_offset [B,8,2,K] at the joint peaks pk_ind[:, 1:] -- and
    hm_hp is the dense (sigmoided) map.  -> det [B,K,118], bit-identical to decode_raw on maps holding the same values."""
    L = lib()
    hm_hp = _dev(hm_hp)
    B, _, H, W = hm_hp.shape
    K = pk_ind.shape[2]
    opt = [None if t is None else _dev(t) for t in (hps, wh, hps_uncertainty, scale, scale_uncertainty, reg, hp_offset,
                                                     tracking, tracking_hp)]
    want = (16, 2, 16, 3, 3, 2, None, 2, 16)
    for t, c in zip(opt, want):
        if t is not None and tuple(t.shape) != ((B, 8, 2, K) if c is None else (B, c, K)):
            raise ValueError("decode_gathered: a table has shape %s" % (tuple(t.shape),))
    det = torch.empty(B, K, DET_STRIDE, device=hm_hp.device, dtype=torch.float32)
    pk_score, pk_ind = pk_score.contiguous(), pk_ind.contiguous()
    if pk_score.dtype != torch.float32 or pk_ind.dtype != torch.int32:
        raise ValueError("decode_gathered: pk_score float32 and pk_ind int32 expected")
    _check(L.cp_decode_gathered(_stream(), B, H, W, _ptr(hm_hp), *[_ptr(t) for t in opt], _ptr(pk_score), _ptr(pk_ind),
                                int(K), int(rep_mode), int(bool(fit_gaussian)), float(balance), int(bool(legacy_bool_mask)),
                                _ptr(det)), "cp_decode_gathered")
    return det


class LazyHeads(Mapping):
    """What ``HipModel.detect(heads="lazy")`` returns for the heads on a model that takes the lean path: a read-only mapping
    with the model's head names in order.  ``hm`` / ``hm_hp`` are there at once.  Any other key -- also through ``items()`` /
    ``values()`` -- is the dense map the decode never needed: it is computed on first access from the feature map the detect
    call left behind (cp_model_dense_heads, on the current stream, all remaining heads in one launch) and cached.  After the
    next ``detect`` on the model that feature map is gone and such an access raises.
    ``gathered``: head -> compact table of the lean path ([B,C,K] at the centre peaks, hp_offset [B,8,2,K] at the joint
    peaks); ``pk_score`` / ``pk_ind``: the peaks [B,9,K]."""

    def __init__(self, model, gen, shapes, ready, gathered, pk_score, pk_ind):
        self._model, self._gen, self._shapes = model, gen, shapes
        self._ready = dict(ready)
        self.gathered, self.pk_score, self.pk_ind = gathered, pk_score, pk_ind

    def __iter__(self):
        return iter(self._shapes)

    def __len__(self):
        return len(self._shapes)

    def __contains__(self, k):   # (Mapping's own asks __getitem__, which would compute the maps)
        return k in self._shapes

    def __getitem__(self, k):
        if k not in self._shapes:
            raise KeyError(k)
        if k not in self._ready:
            self._materialise()
        return self._ready[k]

    def materialised(self):
        return len(self._ready) == len(self._shapes)

    def _materialise(self):
        m = self._model
        if m._det_gen != self._gen:
            raise RuntimeError("detect: the dense '%s' maps of this call were not read before the next detect() on the model, and "
                               "the feature map they are computed from is gone; read them earlier or call detect(heads=\"dense\")"
                               % "', '".join(k for k in self._shapes if k not in self._ready))
        dev = self.pk_ind.device
        new = OrderedDict((k, torch.empty(*shp, device=dev, dtype=torch.float32)) for k, shp in self._shapes.items()
                          if k not in self._ready)
        ptrs = (c_void_p * len(self._shapes))(*[new[k].data_ptr() if k in new else 0 for k in self._shapes])
        _check(lib().cp_model_dense_heads(m._h, _stream(), ptrs), "cp_model_dense_heads")
        self._ready.update(new)


class HipModel(object):
    """Device-resident DLA-34 / DLA-34+ConvGRU / hourglass / resdcn_N network built from a reference-format state dict."""

    def __init__(self, arch, heads, state_dict, tracking_task=False, head_conv=256, precision=None):
        L = lib()
        self.arch = arch
        self.heads = OrderedDict(heads)
        self.tracking_task = bool(tracking_task)
        names = (c_char_p * len(self.heads))(*[k.encode() for k in self.heads])
        classes = (c_int * len(self.heads))(*[int(v) for v in self.heads.values()])
        h = c_void_p()
        _check(L.cp_model_create(arch.encode(), int(self.tracking_task), len(self.heads), names, classes,
                                 int(head_conv), ctypes.byref(h)), "cp_model_create")
        self._h = h
        for k, v in state_dict.items():
            if k.startswith("module.") and not k.startswith("module_list"):
                k = k[7:]  # lib/models/model.py:43-48
            if not torch.is_floating_point(v):
                continue  # num_batches_tracked
            t = v.detach().cpu().contiguous().float()
            _check(L.cp_model_set_param(h, k.encode(), c_void_p(t.data_ptr()), t.numel()), "cp_model_set_param")
        _check(L.cp_model_finalize(h), "cp_model_finalize")
        if precision is not None:
            self.set_precision(precision)
        self._ws = None
        self._ws_key = None

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and _lib is not None:
                _lib.cp_model_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_precision(self, name):
        _check(lib().cp_model_set_precision(self._h, PRECISIONS[name]), "cp_model_set_precision")
        self.precision = name

    def profile(self, enable=True):
        """Arm / disarm per-launch HIP-event timing of the implicit-GEMM kernels."""
        _check(lib().cp_model_profile(self._h, int(bool(enable))), "cp_model_profile")

    def profile_read(self):
        """-> {kernel name: dict(launches, ms, flops, bytes)} accumulated since the last read."""
        nv = lib().cp_num_kernel_variants()  # sized by the library, not by a copy of CP_NUM_KERNEL_VARIANTS
        buf = (ctypes.c_double * (nv * 4))()
        _check(lib().cp_model_profile_read(self._h, buf, nv), "cp_model_profile_read")
        out = OrderedDict()
        for v in range(nv):
            if buf[v * 4] > 0:
                out[lib().cp_kernel_variant_name(v).decode()] = dict(
                    launches=int(buf[v * 4]), ms=buf[v * 4 + 1], flops=buf[v * 4 + 2], bytes=buf[v * 4 + 3])
        return out

    def profile_roles(self):
        """-> {role: dict(launches, ms, flops, bytes)} of the launches drained by the last profile_read()."""
        nr = lib().cp_num_roles()
        buf = (ctypes.c_double * (nr * 4))()
        _check(lib().cp_model_profile_roles(self._h, buf, nr), "cp_model_profile_roles")
        out = OrderedDict()
        for r in range(nr):
            if buf[r * 4] > 0:
                out[lib().cp_role_name(r).decode()] = dict(
                    launches=int(buf[r * 4]), ms=buf[r * 4 + 1], flops=buf[r * 4 + 2], bytes=buf[r * 4 + 3])
        return out

    def workspace_bytes(self, B, H, W):
        n = lib().cp_model_workspace_bytes(self._h, B, H, W)
        if n == 0:
            raise RuntimeError("cp_model_workspace_bytes failed: " + lib().cp_last_error().decode())
        return n

    def workspace_used(self):
        """Bytes of the work space the last pass reached (cp_model_workspace_used): at most workspace_bytes() of its shape."""
        return int(lib().cp_model_workspace_used(self._h))

    def maxpool_launches(self):
        """Stand-alone 2x2 max-pool launches of the last pass (cp_model_maxpool_launches): the stride-2 level entries whose pooled
        input was not written by its producer."""
        return int(lib().cp_model_maxpool_launches(self._h))

    def _workspace(self, B, H, W, device):
        key = (B, H, W, str(device))
        if self._ws_key != key:
            self._ws = None
            n = self.workspace_bytes(B, H, W)
            self._ws = torch.empty(n, dtype=torch.uint8, device=device)
            self._ws_key = key
        return self._ws

    def forward(self, images, pre_img=None, pre_hm=None, pre_hm_hp=None, sigmoid_hm=False, tap=None):
        """images [B,3,H,W] on the HIP device -> OrderedDict head -> [B,classes,H/4,W/4].
        With ``tap`` also returns the named intermediate activation as NCHW.  A tap changes the launch sequence: the fused heads
        are off, and a tap whose name contains ``.node_`` (an IDAUp node or its offset / mask map) runs every IDAUp with its
        stand-alone up-sample + add launches, so a profile taken with such a tap is that of the unfused sequence (the one site
        between two IDAUps, dla_up's last node storing ida_up's first sum, is unfused only by a tap on that node).  Likewise a tap on
        any level entry's ``<entry>.project`` runs every entry's projection as a launch of its own (it is otherwise computed inside the
        block's conv2 and never stored)."""
        L = lib()
        images = _dev(images)
        B, _, H, W = images.shape
        pre_img = _dev(pre_img) if pre_img is not None else None
        pre_hm = _dev(pre_hm) if pre_hm is not None else None
        pre_hm_hp = _dev(pre_hm_hp) if pre_hm_hp is not None else None
        outs = OrderedDict()
        for k, c in self.heads.items():
            outs[k] = torch.empty(B, c, H // 4, W // 4, device=images.device, dtype=torch.float32)
        ptrs = (c_void_p * len(outs))(*[t.data_ptr() for t in outs.values()])
        ws = self._workspace(B, H, W, images.device)
        if tap is None:
            rc = L.cp_model_forward(self._h, _stream(), B, H, W, _ptr(images), _ptr(pre_img), _ptr(pre_hm),
                                    _ptr(pre_hm_hp), ptrs, int(bool(sigmoid_hm)), _ptr(ws), ws.numel())
            _check(rc, "cp_model_forward")
            return outs
        tap_buf = torch.zeros(B * 512 * (H // 4) * (W // 4) if False else B * 16 * H * W, device=images.device,
                              dtype=torch.float32)
        dims = (c_int * 3)(0, 0, 0)
        rc = L.cp_model_forward_tap(self._h, _stream(), B, H, W, _ptr(images), _ptr(pre_img), _ptr(pre_hm),
                                    _ptr(pre_hm_hp), ptrs, int(bool(sigmoid_hm)), _ptr(ws), ws.numel(),
                                    tap.encode(), _ptr(tap_buf), dims)
        _check(rc, "cp_model_forward_tap")
        C, h, w = dims[0], dims[1], dims[2]
        if C == 0:
            raise RuntimeError("unknown tap %r" % tap)
        return outs, tap_buf[: B * C * h * w].view(B, C, h, w)

    def features(self, images, pre_img=None, pre_hm=None, pre_hm_hp=None):
        """The tensor the heads read (cp_model_features): images [B,3,H,W] -> [B,Cin,H/4,W/4] in channels_last memory format (the
        engine's NHWC buffer, no copy); no head is launched.  dla_34 and resdcn_* only."""
        L = lib()
        if self.arch.startswith("dlav1") or self.arch == "hourglass":
            raise NotImplementedError("features(): %s has no single feature map that plain conv3x3 -> ReLU -> conv1x1 heads read"
                                      % self.arch)
        images = _dev(images)
        B, _, H, W = images.shape
        pre_img = _dev(pre_img) if pre_img is not None else None
        pre_hm = _dev(pre_hm) if pre_hm is not None else None
        pre_hm_hp = _dev(pre_hm_hp) if pre_hm_hp is not None else None
        feat = torch.empty(B, H // 4, W // 4, 64, device=images.device, dtype=torch.float32)
        ws = self._workspace(B, H, W, images.device)
        rc = L.cp_model_features(self._h, _stream(), B, H, W, _ptr(images), _ptr(pre_img), _ptr(pre_hm), _ptr(pre_hm_hp),
                                 _ptr(feat), _ptr(ws), ws.numel())
        _check(rc, "cp_model_features")
        return feat.permute(0, 3, 1, 2)

    def lean_supported(self, B, H, W):
        """Does detect(heads="lazy") take the lean path for this shape (cp_model_lean_supported)?"""
        return bool(lib().cp_model_lean_supported(self._h, int(B), int(H), int(W)))

    def heads_at(self, index):
        """The regression heads (every head but hm / hm_hp) at the pixels ``index`` [B,n] (int32, y * (W/4) + x) of the feature
        map the last lean detect() left behind -> OrderedDict head -> [B,classes,n] (cp_model_heads_at)."""
        L = lib()
        index = index.to(torch.int32).contiguous()
        B, n = index.shape
        out = OrderedDict((k, torch.empty(B, c, n, device=index.device, dtype=torch.float32)) for k, c in self.heads.items()
                          if k not in _MAP_HEADS)
        ptrs = (c_void_p * len(self.heads))(*[out[k].data_ptr() if k in out else 0 for k in self.heads])
        nb = L.cp_model_heads_at_workspace_bytes(self._h, B, n)
        ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=index.device)
        _check(L.cp_model_heads_at(self._h, _stream(), _ptr(index), n, ptrs, _ptr(ws), ws.numel()), "cp_model_heads_at")
        return out

    def _detect_lean(self, images, pre_img, pre_hm, pre_hm_hp, K, rep_mode, fit_gaussian, balance, legacy_bool_mask, graph):
        L = lib()
        B, _, H, W = images.shape
        dev = images.device
        key = ("lean", B, H, W, str(dev), K)
        st = getattr(self, "_lean_state", None)
        if st is None or st[0] != key:
            f32 = dict(device=dev, dtype=torch.float32)
            maps = OrderedDict((k, torch.empty(B, self.heads[k], H // 4, W // 4, **f32)) for k in _MAP_HEADS)
            tables = OrderedDict((k, torch.empty(*((B, 8, 2, K) if k == "hp_offset" else (B, c, K)), **f32))
                                 for k, c in self.heads.items() if k not in _MAP_HEADS)
            pk_score = torch.empty(B, 9, K, **f32)
            pk_ind = torch.empty(B, 9, K, device=dev, dtype=torch.int32)
            det = torch.empty(B, K, DET_STRIDE, **f32)
            n = L.cp_model_detect_lean_workspace_bytes(self._h, B, H, W, K)
            if n == 0:
                raise RuntimeError("cp_model_detect_lean_workspace_bytes failed: " + L.cp_last_error().decode())
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            hp = (c_void_p * len(self.heads))(*[maps[k].data_ptr() if k in maps else 0 for k in self.heads])
            tp = (c_void_p * len(self.heads))(*[tables[k].data_ptr() if k in tables else 0 for k in self.heads])
            shapes = OrderedDict((k, (B, c, H // 4, W // 4)) for k, c in self.heads.items())
            st = (key, maps, tables, pk_score, pk_ind, det, ws, hp, tp, shapes)
            self._lean_state = st
        _, maps, tables, pk_score, pk_ind, det, ws, hp, tp, shapes = st
        rc = L.cp_model_detect_lean(self._h, _stream(), B, H, W, _ptr(images), _ptr(pre_img), _ptr(pre_hm), _ptr(pre_hm_hp),
                                    hp, tp, _ptr(pk_score), _ptr(pk_ind), int(K), int(rep_mode), int(bool(fit_gaussian)),
                                    float(balance), int(bool(legacy_bool_mask)), _ptr(det), _ptr(ws), ws.numel(),
                                    int(bool(graph)))
        _check(rc, "cp_model_detect_lean")
        return LazyHeads(self, self._det_gen, shapes, maps, tables, pk_score, pk_ind), det

    def detect(self, images, pre_img=None, pre_hm=None, pre_hm_hp=None, K=100, rep_mode=1, fit_gaussian=False,
               balance=2.0, legacy_bool_mask=False, graph=True, heads="lazy"):
        """backbone + heads + sigmoid + decode in one library call -> (heads mapping, det [B,K,118]).
        Output tensors are owned by the model and REUSED by the next call with the same batch shape (that is what lets
        the launch sequence be replayed from a hipGraph).  With ``graph`` the caller must run on a non-default stream
        and pass the same input tensors (copy new frames into them).

        The decode reads hm and hm_hp on every pixel, but the regression heads only at the decoded peaks: their dense maps
        are a by-product it never needed.  ``heads="lazy"`` (default), on a model that supports it (f16x3, grouped fused
        heads: dla_34, hourglass -- ``lean_supported``), runs cp_model_detect_lean, which evaluates those heads at the peaks
        only; the first return value is then a ``LazyHeads`` mapping (same keys, same order) whose regression maps are
        computed on first access, at their old cost, and only until the next ``detect`` on the model (afterwards such an
        access raises).  On any other model ``"lazy"`` is today's call and returns the plain OrderedDict.
        ``heads="dense"``: cp_model_detect, every map computed up front."""
        if heads not in ("lazy", "dense"):
            raise ValueError("detect: heads must be 'lazy' or 'dense'")
        L = lib()
        B, _, H, W = images.shape
        for t in (images, pre_img, pre_hm, pre_hm_hp):
            if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
                raise RuntimeError("detect: inputs must be contiguous float32 device tensors")
        self._det_gen = getattr(self, "_det_gen", 0) + 1   # (what a LazyHeads of an earlier call checks)
        if heads == "lazy" and L.cp_model_lean_supported(self._h, B, H, W):
            return self._detect_lean(images, pre_img, pre_hm, pre_hm_hp, K, rep_mode, fit_gaussian, balance, legacy_bool_mask,
                                     graph)
        key = ("det", B, H, W, str(images.device), K)
        st = getattr(self, "_det_state", None)
        if st is None or st[0] != key:
            outs = OrderedDict((k, torch.empty(B, c, H // 4, W // 4, device=images.device, dtype=torch.float32))
                               for k, c in self.heads.items())
            det = torch.empty(B, K, DET_STRIDE, device=images.device, dtype=torch.float32)
            n = L.cp_model_detect_workspace_bytes(self._h, B, H, W, K)
            if n == 0:
                raise RuntimeError("cp_model_detect_workspace_bytes failed: " + L.cp_last_error().decode())
            ws = torch.empty(n, dtype=torch.uint8, device=images.device)
            ptrs = (c_void_p * len(outs))(*[t.data_ptr() for t in outs.values()])
            st = (key, outs, det, ws, ptrs)
            self._det_state = st
        _, outs, det, ws, ptrs = st
        for t in (images, pre_img, pre_hm, pre_hm_hp):
            if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
                raise RuntimeError("detect: inputs must be contiguous float32 device tensors")
        rc = L.cp_model_detect(self._h, _stream(), B, H, W, _ptr(images), _ptr(pre_img), _ptr(pre_hm), _ptr(pre_hm_hp),
                               ptrs, int(K), int(rep_mode), int(bool(fit_gaussian)), float(balance),
                               int(bool(legacy_bool_mask)), _ptr(det), _ptr(ws), ws.numel(), int(bool(graph)))
        _check(rc, "cp_model_detect")
        return outs, det

    __call__ = forward


# batch key -> (descriptor field, kind): kind "f" float32 values, "m" a mask (any dtype -> float32), "i" indices
_PL_BATCH = (("hm", "gt_hm", "f"), ("hm_hp", "gt_hm_hp", "f"), ("ind", "ind", "i"), ("reg_mask", "reg_mask", "m"),
             ("hps", "gt_hps", "f"), ("hps_mask", "hps_mask", "m"), ("wh", "gt_wh", "f"), ("reg", "gt_reg", "f"),
             ("scale", "gt_scale", "f"), ("hp_ind", "hp_ind", "i"), ("hp_mask", "hp_mask", "m"),
             ("hp_offset", "gt_hp_offset", "f"), ("tracking", "gt_tracking", "f"), ("tracking_mask", "tracking_mask", "m"),
             ("tracking_hp", "gt_tracking_hp", "f"), ("tracking_hp_mask", "tracking_hp_mask", "m"))


def _pl_used(terms, flags):
    """Head names and batch keys the counted terms (bit i: POSE_LOSS_TERMS[i]) read."""
    on = {t for i, t in enumerate(POSE_LOSS_TERMS) if terms >> i & 1}
    train = not flags & PL_VAL
    heads, keys = ["hm", "hps"], ["hm", "ind", "hps", "hps_mask"]
    if flags & PL_HM_HP_MAPS or "hm_hp" in on:
        heads.append("hm_hp"), keys.append("hm_hp")
    if train and flags & PL_HPS_UNCERTAINTY:
        heads.append("hps_uncertainty")
    for t, h, k in (("wh", "wh", ("wh", "reg_mask")), ("off", "reg", ("reg", "reg_mask")),
                    ("obj_scale", "scale", ("scale", "reg_mask")), ("hp_offset", "hp_offset", ("hp_offset", "hp_ind", "hp_mask")),
                    ("tracking", "tracking", ("tracking", "tracking_mask")),
                    ("tracking_hp", "tracking_hp", ("tracking_hp", "tracking_hp_mask"))):
        if t in on:
            heads.append(h)
            keys.extend(x for x in k if x not in keys)
    if "obj_scale" in on and train and flags & PL_SCALE_UNCERTAINTY:
        heads.append("scale_uncertainty")
    return heads, keys


def pose_loss_forward(outputs, batch, terms, flags, weights, kl_kps=0.1, kl_scale=0.1, dimension_ref=(1.0, 1.0, 1.0),
                      with_terms=False):
    """cp_pose_loss_forward: ObjectPoseLoss's loss on the device.  ``outputs`` is a list (one per stack) of dicts of NCHW
    float32 head tensors; the hm (and hm_hp) tensors are overwritten in place with sigmoid(logit).  ``batch`` holds the
    dataset's collated ground truth on the same device ([B,S,...]; uint8 / int64 masks, int64 indices).  ``terms`` has
    bit i set when POSE_LOSS_TERMS[i] counts, ``flags`` is PL_* bits, ``weights`` the nine term weights.
    Returns (loss [], stats [10], choice int64 [B], terms [9,B,S] or None, clamped [(hm, hm_hp or None)] per stack, state);
    ``state`` is what pose_loss_backward needs.  An index outside [0, H*W) raises ValueError before any launch."""
    L = lib()
    heads_used, keys = _pl_used(terms, flags)
    ns = len(outputs)
    if not 1 <= ns <= POSE_LOSS_MAX_STACKS:
        raise ValueError("pose_loss: 1 to %d stacks" % POSE_LOSS_MAX_STACKS)
    hm = outputs[0]["hm"]
    B, C, H, W = hm.shape
    dev = hm.device
    for k in keys:
        if k not in batch:
            raise ValueError("pose_loss: batch['%s'] is missing" % k)
        if not batch[k].is_cuda or batch[k].device != dev:
            raise ValueError("pose_loss: batch['%s'] must live on %s" % (k, dev))
    S, K = batch["ind"].shape[1], batch["ind"].shape[2]
    J = batch["hps"].shape[-1] // 2
    HW = H * W
    shapes = {"hm": (B, S, C, H, W), "hm_hp": (B, S, J, H, W), "ind": (B, S, K), "reg_mask": (B, S, K),
              "hps": (B, S, K, 2 * J), "hps_mask": (B, S, K, 2 * J), "wh": (B, S, K, 2), "reg": (B, S, K, 2),
              "scale": (B, S, K, 3), "hp_ind": (B, S, K * J), "hp_mask": (B, S, K * J), "hp_offset": (B, S, K * J, 2),
              "tracking": (B, S, K, 2), "tracking_mask": (B, S, K), "tracking_hp": (B, S, K, 2 * J),
              "tracking_hp_mask": (B, S, K, 2 * J)}
    for k in keys:
        if tuple(batch[k].shape) != shapes[k]:
            raise ValueError("pose_loss: batch['%s'] has shape %s, expected %s" % (k, tuple(batch[k].shape), shapes[k]))
    hchan = {"hm": C, "hm_hp": J, "hps": 2 * J, "hps_uncertainty": 2 * J, "wh": 2, "reg": 2, "scale": 3,
             "scale_uncertainty": 3, "hp_offset": 2, "tracking": 2, "tracking_hp": 2 * J}
    for st, out in enumerate(outputs):
        for h in heads_used:
            t = out.get(h)
            if t is None:
                raise ValueError("pose_loss: outputs[%d]['%s'] is missing" % (st, h))
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.data_ptr() % 16:
                raise ValueError("pose_loss: outputs[%d]['%s'] must be a contiguous, 16-byte aligned float32 tensor on %s"
                                 % (st, h, dev))
            if tuple(t.shape) != (B, hchan[h], H, W):
                raise ValueError("pose_loss: outputs[%d]['%s'] has shape %s, expected %s"
                                 % (st, h, tuple(t.shape), (B, hchan[h], H, W)))
    # every index in [0, H*W): one reduction, one read-back (torch.gather refuses the same batches)
    idx_keys = [k for k in ("ind", "hp_ind") if k in keys]
    bad = torch.stack([((batch[k] < 0) | (batch[k] >= HW)).any() for k in idx_keys]).to(torch.int32)
    nbad = (bad * torch.tensor([1 << i for i in range(len(idx_keys))], dtype=torch.int32, device=dev)).sum().item()
    for i, k in enumerate(idx_keys):
        if nbad >> i & 1:
            raise ValueError("pose_loss: batch['%s'] holds an index outside [0, %d)" % (k, HW))
    keep = []
    d = PoseLossDesc()
    d.B, d.S, d.K, d.H, d.W, d.num_classes, d.num_joints, d.num_stacks = B, S, K, H, W, C, J, ns
    d.terms, d.flags = int(terms), int(flags)
    for i in range(9):
        d.weight[i] = float(weights[i])
    d.kl_kps, d.kl_scale = float(kl_kps), float(kl_scale)
    for i in range(3):
        d.dimension_ref[i] = float(dimension_ref[i])
    for key, field, kind in _PL_BATCH:
        if key not in keys:
            continue
        t = batch[key]
        t = t.to(torch.int32) if kind == "i" else t.float()
        t = t.contiguous()
        if t.data_ptr() % 16:  # the heat-map kernels read float4 lines: an offset view gets aligned storage
            t = t.clone()
        keep.append(t)
        setattr(d, field, t.data_ptr())
    clamped = []
    for st, out in enumerate(outputs):
        for i, h in enumerate(POSE_LOSS_HEADS):
            if h in heads_used:
                d.head[st][i] = out[h].data_ptr()
        pair = []
        for j, h in enumerate(("hm", "hm_hp")):
            if h in heads_used:
                c = torch.empty_like(out[h])
                d.clamped[st][j] = c.data_ptr()
                pair.append(c)
            else:
                pair.append(None)
        clamped.append(tuple(pair))
    nbytes = L.cp_pose_loss_workspace_bytes(ctypes.byref(d))
    if nbytes == 0:
        _check(L.cp_pose_loss_forward(_stream(), ctypes.byref(d), None, None, None, None, None, 0), "cp_pose_loss_forward")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    stats = torch.empty(10, dtype=torch.float32, device=dev)
    choice = torch.empty(B, dtype=torch.int64, device=dev)
    tm = torch.empty(9, B, S, dtype=torch.float32, device=dev) if with_terms else None
    _check(L.cp_pose_loss_forward(_stream(), ctypes.byref(d), _ptr(loss), _ptr(stats), _ptr(choice), _ptr(tm), _ptr(ws),
                                  nbytes), "cp_pose_loss_forward")
    state = {"desc": d, "ws": ws, "keep": keep, "heads": heads_used, "outputs": [dict(o) for o in outputs]}
    return loss, stats, choice, tm, clamped, state


def _aligned(t):
    t = t.float().contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def pose_loss_backward(state, dloss, dmaps=None):
    """cp_pose_loss_backward: dL/d(head) of every head the counted terms use, for the forward that made ``state``;
    ``dloss`` a one-element float32 device tensor.  ``dmaps`` (optional, one (hm, hm_hp) pair per stack, entries may be
    None) are gradients arriving on the in-place sigmoid tensors; they are chained through the sigmoid and added.
    Returns a list (one per stack) of {head name: gradient}."""
    d = state["desc"]
    dloss = dloss.reshape(1).float().contiguous()
    ws = state["ws"]
    grads = []
    ptrs = (c_void_p * (POSE_LOSS_MAX_STACKS * len(POSE_LOSS_HEADS)))()
    dm = (c_void_p * (2 * POSE_LOSS_MAX_STACKS))()
    hold = []
    counted = {"hm": True, "hm_hp": bool(d.terms >> POSE_LOSS_TERMS.index("hm_hp") & 1)}
    for st, out in enumerate(state["outputs"]):
        g = {}
        for j, h in enumerate(("hm", "hm_hp")):
            t = dmaps[st][j] if dmaps is not None else None
            if t is not None and h in state["heads"]:
                t = _aligned(t)
                hold.append(t)
                dm[2 * st + j] = t.data_ptr()
        for i, h in enumerate(POSE_LOSS_HEADS):
            if h not in state["heads"]:
                continue
            if h in counted and not counted[h] and not dm[2 * st + (h == "hm_hp")]:
                continue
            g[h] = torch.empty_like(out[h])
            ptrs[st * len(POSE_LOSS_HEADS) + i] = g[h].data_ptr()
        grads.append(g)
    _check(lib().cp_pose_loss_backward(_stream(), ctypes.byref(d), _ptr(dloss), dm, ptrs, _ptr(ws),
                                       ws.numel()), "cp_pose_loss_backward")
    return grads


def pose_targets_desc(images, objects, S, R, flags, out):
    """cp_pose_targets_desc for host float64 records ``images`` [B, PT_IMG_STRIDE] and ``objects`` [B, K, PT_OBJ_STRIDE]
    (numpy arrays, kept alive by the caller), ``flags`` {PT_FLAGS name: bool} and ``out`` {PT_OUTPUTS name: tensor or
    None}."""
    d = PoseTargetsDesc()
    d.B, d.S, d.R = images.shape[0], int(S), int(R)
    d.max_objs, d.num_joints = objects.shape[1], 8
    for n in PT_FLAGS:
        setattr(d, n, int(bool(flags.get(n, False))))
    d.images, d.objects = images.ctypes.data, objects.ctypes.data
    for n in PT_OUTPUTS:
        t = out.get(n)
        setattr(d, "out_" + n, t.data_ptr() if t is not None else None)
    return d


def pose_targets(images, objects, S, R, flags, out):
    """cp_pose_targets: the training targets of a batch, written into the device tensors of ``out`` on the current
    stream.  ``images`` / ``objects`` are the host records (converted to pageable float64 copies here, which the call
    stages before it returns); refused arguments raise ValueError before any launch."""
    import numpy as np

    images = np.array(images, dtype=np.float64, order="C", copy=True)
    objects = np.array(objects, dtype=np.float64, order="C", copy=True)
    if images.ndim != 2 or images.shape[1] != PT_IMG_STRIDE or objects.ndim != 3 or \
            objects.shape[0] != images.shape[0] or objects.shape[2] != PT_OBJ_STRIDE:
        raise ValueError("pose_targets: records must be [B, %d] and [B, K, %d]" % (PT_IMG_STRIDE, PT_OBJ_STRIDE))
    L = lib()
    d = pose_targets_desc(images, objects, S, R, flags, out)
    nbytes = L.cp_pose_targets_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=out["hm"].device) if nbytes else None
    rc = L.cp_pose_targets(_stream(), ctypes.byref(d), _ptr(ws), nbytes)
    if rc == CP_ERR_INVALID:
        raise ValueError("centerpose_hip: cp_pose_targets: %s" % L.cp_last_error().decode())
    _check(rc, "cp_pose_targets")


def pose_targets_track_desc(records, S, R, flags, track, out):
    """cp_pose_targets_track_desc.  ``records``: the five host float64 arrays {'pt_image', 'pt_objects', 'ptk_image',
    'ptk_pre_objects', 'ptk_cur_objects'} (kept alive by the caller); ``flags`` as pose_targets_desc's; ``track``
    {PTK_GEOMETRY / PTK_FLAGS / PTK_DISTURB name: value} (max_pre_objs comes from the records); ``out`` {PT_OUTPUTS or
    PTK_OUTPUTS name: tensor or None}."""
    d = PoseTargetsTrackDesc()
    d.cur = pose_targets_desc(records["pt_image"], records["pt_objects"], S, R, flags, out)
    for n in PTK_GEOMETRY + PTK_FLAGS:
        setattr(d, n, int(track.get(n, 0)))
    d.max_pre_objs = records["ptk_pre_objects"].shape[1]
    for n in PTK_DISTURB:
        setattr(d, n, float(track.get(n, 0.0)))
    d.track_images = records["ptk_image"].ctypes.data
    d.pre_objects = records["ptk_pre_objects"].ctypes.data
    d.cur_objects = records["ptk_cur_objects"].ctypes.data
    for n in PTK_OUTPUTS:
        t = out.get(n)
        setattr(d, "out_" + n, t.data_ptr() if t is not None else None)
    return d


def pose_targets_track(records, S, R, flags, track, out):
    """cp_pose_targets_track: the tracking task's training targets of a batch, written into the device tensors of ``out``
    on the current stream (arguments as pose_targets_track_desc's; the records are converted to pageable float64 copies
    here, which the call stages before it returns).  Refused arguments raise ValueError before any launch."""
    import numpy as np

    recs = {k: np.array(records[k], dtype=np.float64, order="C", copy=True)
            for k in ("pt_image", "pt_objects", "ptk_image", "ptk_pre_objects", "ptk_cur_objects")}
    B = recs["pt_image"].shape[0]
    want = {"pt_image": (PT_IMG_STRIDE,), "pt_objects": (None, PT_OBJ_STRIDE), "ptk_image": (PTK_IMG_STRIDE,),
            "ptk_pre_objects": (None, PTK_PRE_STRIDE), "ptk_cur_objects": (None, PTK_CUR_STRIDE)}
    for k, tail in want.items():
        a = recs[k]
        if a.ndim != 1 + len(tail) or a.shape[0] != B or a.shape[-1] != tail[-1]:
            raise ValueError("pose_targets_track: %s must be [B, %s]" % (k, ", ".join("K" if t is None else str(t) for t in tail)))
    if recs["ptk_cur_objects"].shape[1] != recs["pt_objects"].shape[1]:
        raise ValueError("pose_targets_track: ptk_cur_objects and pt_objects must have the same max_objs")
    L = lib()
    d = pose_targets_track_desc(recs, S, R, flags, track, out)
    nbytes = L.cp_pose_targets_track_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=out["hm"].device) if nbytes else None
    rc = L.cp_pose_targets_track(_stream(), ctypes.byref(d), _ptr(ws), nbytes)
    if rc == CP_ERR_INVALID:
        raise ValueError("centerpose_hip: cp_pose_targets_track: %s" % L.cp_last_error().decode())
    _check(rc, "cp_pose_targets_track")


def pose_targets_track_det(records, S, R, flags, track, det, out):
    """cp_pose_targets_track_det: cp_pose_targets_track with a detector's boxes for the images whose ``records['ptk_gen']``
    row asks for data generation mode 1.  ``det``: {'post': [B, K_det, 120] float64, 'count': [B] int32, 'pnp':
    [B, K_det, 40] float64 device tensors of ``postprocess`` / ``pnp_from_post`` on the previous frames' input images,
    'render_hm_mode', 'render_hmhp_mode', 'cat_rule'}.  Everything else as pose_targets_track; refused arguments raise
    ValueError before any launch.  No host synchronisation."""
    import numpy as np

    names = ("pt_image", "pt_objects", "ptk_image", "ptk_pre_objects", "ptk_cur_objects", "ptk_gen")
    recs = {k: np.array(records[k], dtype=np.float64, order="C", copy=True) for k in names}
    B = recs["pt_image"].shape[0]
    want = {"pt_image": (PT_IMG_STRIDE,), "pt_objects": (None, PT_OBJ_STRIDE), "ptk_image": (PTK_IMG_STRIDE,),
            "ptk_pre_objects": (None, PTK_PRE_STRIDE), "ptk_cur_objects": (None, PTK_CUR_STRIDE), "ptk_gen": (PTK_GEN_STRIDE,)}
    for k, tail in want.items():
        a = recs[k]
        if a.ndim != 1 + len(tail) or a.shape[0] != B or a.shape[-1] != tail[-1]:
            raise ValueError("pose_targets_track_det: %s must be [B, %s]" %
                             (k, ", ".join("K" if t is None else str(t) for t in tail)))
    if recs["ptk_cur_objects"].shape[1] != recs["pt_objects"].shape[1]:
        raise ValueError("pose_targets_track_det: ptk_cur_objects and pt_objects must have the same max_objs")
    post, count, pnp = det["post"], det["count"], det["pnp"]
    if not (post.is_cuda and post.dtype == torch.float64 and post.is_contiguous() and post.dim() == 3 and
            post.shape[0] == B and post.shape[2] == POST_STRIDE):
        raise ValueError("pose_targets_track_det: det['post'] must be a contiguous float64 device tensor [B, K_det, %d]"
                         % POST_STRIDE)
    K_det = int(post.shape[1])
    if not (pnp.is_cuda and pnp.dtype == torch.float64 and pnp.is_contiguous() and tuple(pnp.shape) == (B, K_det, PNP_STRIDE)):
        raise ValueError("pose_targets_track_det: det['pnp'] must be a contiguous float64 device tensor [B, K_det, %d]"
                         % PNP_STRIDE)
    if not (count.is_cuda and count.dtype == torch.int32 and count.is_contiguous() and count.numel() == B):
        raise ValueError("pose_targets_track_det: det['count'] must be a contiguous int32 device tensor [B]")
    L = lib()
    d = PoseTargetsTrackDetDesc()
    d.track = pose_targets_track_desc(recs, S, R, flags, track, out)
    d.det_post, d.det_count, d.det_pnp = post.data_ptr(), count.data_ptr(), pnp.data_ptr()
    d.K_det = K_det
    for n in PTK_DET_OPTS[1:]:
        setattr(d, n, int(det[n]))
    d.gen = recs["ptk_gen"].ctypes.data
    nbytes = L.cp_pose_targets_track_det_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=out["hm"].device) if nbytes else None
    rc = L.cp_pose_targets_track_det(_stream(), ctypes.byref(d), _ptr(ws), nbytes)
    if rc == CP_ERR_INVALID:
        raise ValueError("centerpose_hip: cp_pose_targets_track_det: %s" % L.cp_last_error().decode())
    _check(rc, "cp_pose_targets_track_det")


def train_inputs_means_offset(N):
    """CP_TI_WS_MEANS(N): where cp_train_inputs leaves the float32 gs_mean of every image in its workspace."""
    return (int(N) * TI_STRIDE * 8 + 255) // 256 * 256


def train_inputs(frames, records, mean, std, out, return_means=False):
    """cp_train_inputs: the training input images of N frames, written into the device tensor ``out`` [N,3,out_h,out_w]
    float32 on the current stream.  ``frames`` is one contiguous uint8 device tensor of any shape that holds every frame
    at its record's byte offset; ``records`` the host records [N, TI_STRIDE] (converted to a pageable float64 copy
    here, which the call stages before it returns).  Refused arguments raise ValueError before any launch.
    ``return_means``: also return the float32 [N] grey means the call used (a view of its workspace)."""
    import numpy as np

    records = np.array(records, dtype=np.float64, order="C", copy=True)
    if records.ndim != 2 or records.shape[1] != TI_STRIDE:
        raise ValueError("train_inputs: records must be [N, %d]" % TI_STRIDE)
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous()):
        raise ValueError("train_inputs: frames must be a contiguous uint8 device tensor")
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4 and
            out.shape[0] == records.shape[0] and out.shape[1] == 3):
        raise ValueError("train_inputs: out must be a contiguous float32 device tensor [N, 3, out_h, out_w]")
    L = lib()
    N, out_h, out_w = records.shape[0], int(out.shape[2]), int(out.shape[3])
    f3 = ctypes.c_float * 3
    nbytes = L.cp_train_inputs_workspace_bytes(N, out_h, out_w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=out.device) if nbytes else None
    rc = L.cp_train_inputs(_stream(), _ptr(frames), frames.numel(), records.ctypes.data, N,
                           f3(*[float(v) for v in np.asarray(mean).reshape(-1)]),
                           f3(*[float(v) for v in np.asarray(std).reshape(-1)]), _ptr(out), out_h, out_w, _ptr(ws), nbytes)
    if rc == CP_ERR_INVALID:
        raise ValueError("centerpose_hip: cp_train_inputs: %s" % L.cp_last_error().decode())
    _check(rc, "cp_train_inputs")
    if return_means:
        o = train_inputs_means_offset(N)
        return out, ws[o:o + 4 * N].view(torch.float32)
    return out
