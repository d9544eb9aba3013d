"""The structs of include/centerpose_hip.h as ctypes.Structures (field for field), with the name tuples and record layouts
of the same header sections.  They stand below ``_abi`` because its signature table points at them; ``track`` and ``train``
hold the code that fills them."""
import ctypes
from ctypes import c_int, c_void_p


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


# ---- the overlay (cp_draw_*): primitive kinds, the slots of a record and the params struct of include/centerpose_hip.h ----
DRAW_SEGMENT, DRAW_DISC, DRAW_RECT, DRAW_FILL, DRAW_GLYPH = 1, 2, 3, 4, 5
DRAW_COORD_MIN, DRAW_COORD_MAX, DRAW_MAX_DIM, DRAW_MAX_P = -8192, 8191, 8192, 65536
DRAW_SLOTS = 44
DRAW_SLOT = dict(box=0, label=1, discs=15, edges=23, cross=35, axes=41)
DRAW_LABEL_CHARS, DRAW_LABEL_SCALE = 13, 2
DRAW_CAT0 = {"black": 0xFFFFFF, "white": 0x8080FF}  # the reference's category-0 colour per theme, B | G << 8 | R << 16


class DrawParams(ctypes.Structure):
    """cp_draw_params of include/centerpose_hip.h (field for field)."""
    _fields_ = [("vis_thresh", ctypes.c_double)] + \
               [(n, c_int) for n in ("reg_bbox", "show_axes", "paper_display", "tracking_task", "theme", "labels", "width", "height")]
