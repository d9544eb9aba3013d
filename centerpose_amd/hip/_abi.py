"""The library and its C ABI: where libcenterpose_hip.so is, the one table of its entry points' signatures, ``lib()``, and
the few primitives every wrapper of the package is made of.  The other modules reach these as ``_abi.lib()``,
``_abi._stream()``, ...: through the module object, so that this is the one place to stub them."""
import contextlib
import ctypes
import enum
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

import torch

from ._structs import DrawParams, PoseLossDesc, PoseTargetsDesc, PoseTargetsTrackDesc, PoseTargetsTrackDetDesc, TrackParams

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # centerpose_amd/, where csrc/Makefile leaves the library
# $CENTERPOSE_HIP_LIB selects another build of the same ABI (tuning variants: make -C csrc EXP=n)
LIB_PATH = os.environ.get("CENTERPOSE_HIP_LIB") or os.path.join(_PKG, "libcenterpose_hip.so")

_lib = None
ABI_VERSION = 7  # CP_ABI_VERSION of include/centerpose_hip.h this binding was written against
CP_ERR_INVALID = -1

_vp, _i = [c_void_p], [c_int]
_pvp, _pi, _pf, _pd = [POINTER(c_void_p)], [POINTER(c_int)], [POINTER(c_float)], [POINTER(c_double)]
_ws = [c_void_p, c_size_t]  # the (workspace, workspace_bytes) pair most launches end with
_model = _vp * 2 + _i * 3 + _vp * 4  # model, stream, B, H, W, images, pre_img, pre_hm, pre_hm_hp

# entry point -> (return type, argument types): one entry per declaration of include/centerpose_hip.h and
# include/centerpose_hip_testing.h, checked against their text by tests/test_binding_table_cpu.py
SIGNATURES = {
    "cp_abi_version": (c_int, []),
    "cp_version": (c_char_p, []),
    "cp_last_error": (c_char_p, []),
    "cp_num_kernel_variants": (c_int, []),
    "cp_num_roles": (c_int, []),
    "cp_dcnv2_workspace_bytes": (c_size_t, _i * 5),
    "cp_dcnv2_forward": (c_int, _vp * 7 + _i * 14 + _ws),
    "cp_dcnv2_backward_workspace_bytes": (c_size_t, _i * 14),
    "cp_dcnv2_backward": (c_int, _vp * 11 + _i * 14 + _ws),
    "cp_dcnv2_backward_det_workspace_bytes": (c_size_t, _i * 14),
    "cp_dcnv2_backward_det": (c_int, _vp * 11 + _i * 14 + _ws),
    "cp_dcnv2_backward_prec_workspace_bytes": (c_size_t, _i * 16),
    "cp_dcnv2_backward_prec": (c_int, _vp * 11 + _i * 16 + _ws),
    "cp_dcnv2_backward_prec_mask": (c_int, _i * 16),
    "cp_pose_heads_chunk_images": (c_int, _i * 4),
    "cp_pose_heads_forward_workspace_bytes": (c_size_t, _i * 6 + _pi),
    "cp_pose_heads_backward_workspace_bytes": (c_size_t, _i * 6 + _pi),
    "cp_pose_heads_forward": (c_int, _vp * 2 + _i + _pvp * 4 + _pi + _pvp + _i * 5 + _ws),
    "cp_pose_heads_backward": (c_int, _vp * 2 + _i + _pvp * 4 + _pi + _pvp * 5 + _vp + _i * 5 + _ws),
    "cp_pose_heads_backward_prec_workspace_bytes": (c_size_t, _i * 6 + _pi + _i),
    "cp_pose_heads_backward_prec": (c_int, _vp * 2 + _i + _pvp * 4 + _pi + _pvp * 5 + _vp + _i * 6 + _ws),
    "cp_pose_heads_backward_prec_mask": (c_int, _i * 6),
    "cp_model_features": (c_int, _model + _vp + _ws),
    "cp_model_create": (c_int, [c_char_p, c_int, c_int, POINTER(c_char_p)] + _pi + _i + _pvp),
    "cp_model_set_param": (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    "cp_model_finalize": (c_int, _vp),
    "cp_model_destroy": (None, _vp),
    "cp_model_workspace_bytes": (c_size_t, _vp + _i * 3),
    "cp_model_workspace_used": (c_size_t, _vp),
    "cp_model_maxpool_launches": (c_int, _vp),
    "cp_model_forward": (c_int, _model + _pvp + _i + _ws),
    "cp_model_forward_tap": (c_int, _model + _pvp + _i + _ws + [c_char_p, c_void_p] + _pi),
    "cp_conv2d_workspace_bytes": (c_size_t, _i * 4),
    "cp_conv_transpose2d_workspace_bytes": (c_size_t, _i * 2),
    "cp_conv_transpose2d_nhwc": (c_int, _vp * 6 + _i * 6 + _ws),
    "cp_conv2d_nhwc": (c_int, _vp * 7 + _i * 10 + _ws),
    "cp_conv2d_backward_workspace_bytes": (c_size_t, _i * 10),
    "cp_conv2d_backward_nhwc": (c_int, _vp * 8 + _i * 9 + _ws),
    "cp_conv2d_backward_path": (c_int, _i * 9),
    "cp_conv2d_backward_prec_workspace_bytes": (c_size_t, _i * 11),
    "cp_conv2d_backward_prec_nhwc": (c_int, _vp * 8 + _i * 10 + _ws),
    "cp_conv2d_backward_prec_mask": (c_int, _i * 10),
    "cp_conv_transpose2d_dw_nhwc": (c_int, _vp * 5 + _i * 5),
    "cp_conv_transpose2d_backward_workspace_bytes": (c_size_t, _i * 10),
    "cp_conv_transpose2d_backward_nhwc": (c_int, _vp * 6 + _i * 9 + _ws),
    "cp_conv_transpose2d_backward_prec_workspace_bytes": (c_size_t, _i * 11),
    "cp_conv_transpose2d_backward_prec_nhwc": (c_int, _vp * 6 + _i * 10 + _ws),
    "cp_conv_transpose2d_backward_prec_mask": (c_int, _i * 10),
    "cp_batchnorm_workspace_bytes": (c_size_t, _i * 4),
    "cp_batchnorm_forward_nhwc": (c_int, _vp * 10 + _i * 5 + [c_float, c_float, c_int] + _ws),
    "cp_batchnorm_backward_nhwc": (c_int, _vp * 11 + _i * 5 + _ws),
    "cp_batchnorm_sync_record_floats": (c_int, _i),
    "cp_batchnorm_sync_stats_nhwc": (c_int, _vp * 3 + _i * 4 + _ws),
    "cp_batchnorm_sync_forward_nhwc": (c_int, _vp * 12 + _i * 5 + [c_float, c_float, c_int] + _ws),
    "cp_batchnorm_sync_backward_reduce_nhwc": (c_int, _vp * 9 + _i * 4 + _ws),
    "cp_batchnorm_sync_backward_apply_nhwc": (c_int, _vp * 8 + _i + _vp * 3 + _i * 4 + _ws),
    "cp_groupnorm_workspace_bytes": (c_size_t, _i * 5),
    "cp_groupnorm_forward_nhwc": (c_int, _vp * 7 + _i * 5 + [c_float, c_int] + _ws),
    "cp_groupnorm_backward_nhwc": (c_int, _vp * 10 + _i * 5 + _ws),
    "cp_gru_gate_forward": (c_int, _vp * 5 + _i * 2),
    "cp_gru_gate_backward": (c_int, _vp * 8 + _i * 2),
    "cp_maxpool2d_forward_nhwc": (c_int, _vp * 3 + _i * 7),
    "cp_maxpool2d_backward_nhwc": (c_int, _vp * 4 + _i * 7),
    "cp_conv2d_stem_backward_workspace_bytes": (c_size_t, _i * 6),
    "cp_conv2d_stem_backward": (c_int, _vp * 7 + [c_size_t] + _i * 6),
    "cp_conv2d_stem_wide_backward_workspace_bytes": (c_size_t, _i * 6),
    "cp_conv2d_stem_wide_backward": (c_int, _vp * 7 + [c_size_t] + _i * 6),
    "cp_upsample2_add_nhwc": (c_int, _vp * 4 + _i * 4),
    "cp_upsample2_add_backward_nhwc": (c_int, _vp * 3 + _i * 4),
    "cp_decode_workspace_bytes": (c_size_t, _i * 2),
    "cp_decode": (c_int, _vp + _i * 3 + _vp * 11 + _i * 3 + [c_float] + _i * 2 + _vp + _ws),
    "cp_decode_tiled_workspace_bytes": (c_size_t, _i * 4),
    "cp_decode_tiled": (c_int, _vp + _i * 3 + _vp * 11 + _i * 3 + [c_float] + _i * 2 + _vp + _ws),
    "cp_model_detect_workspace_bytes": (c_size_t, _vp + _i * 4),
    "cp_model_detect": (c_int, _model + _pvp + _i * 3 + [c_float] + _i + _vp + _ws + _i),
    "cp_model_lean_supported": (c_int, _vp + _i * 3),
    "cp_model_detect_lean_workspace_bytes": (c_size_t, _vp + _i * 4),
    "cp_model_detect_lean": (c_int, _model + _pvp * 2 + _vp * 2 + _i * 3 + [c_float] + _i + _vp + _ws + _i),
    "cp_model_dense_heads": (c_int, _vp * 2 + _pvp),
    "cp_model_heads_at_workspace_bytes": (c_size_t, _vp + _i * 2),
    "cp_model_heads_at": (c_int, _vp * 3 + _i + _pvp + _ws),
    "cp_decode_peaks_workspace_bytes": (c_size_t, _i * 4),
    "cp_decode_peaks": (c_int, _vp + _i * 3 + _vp * 2 + _i * 2 + _vp * 2 + _ws),
    "cp_decode_gathered": (c_int, _vp + _i * 3 + _vp * 12 + _i * 3 + [c_float] + _i + _vp),
    "cp_set_default_precision": (c_int, _i),
    "cp_set_debug": (c_int, _i),
    "cp_render_gaussians": (c_int, _vp * 2 + _i + _vp + _i * 4),
    "cp_postprocess_workspace_bytes": (c_size_t, _i * 2),
    "cp_postprocess": (c_int, _vp * 2 + _i * 2 + [c_void_p, c_double, c_int, c_float] + _vp * 2 + _ws),
    "cp_preprocess": (c_int, _vp * 2 + _i * 2 + _pd + _pf * 2 + _vp + _i * 2),
    "cp_preprocess_batch": (c_int, _vp * 2 + _i * 3 + _pd + _pf * 2 + _vp + _i * 2),
    "cp_resize_u8": (c_int, _vp * 2 + _i * 3 + _vp + _i * 2),
    "cp_model_set_precision": (c_int, _vp + _i),
    "cp_model_profile": (c_int, _vp + _i),
    "cp_model_profile_read": (c_int, _vp + _pd + _i),
    "cp_kernel_variant_name": (c_char_p, _i),
    "cp_model_profile_roles": (c_int, _vp + _pd + _i),
    "cp_role_name": (c_char_p, _i),
    "cp_pnp_workspace_bytes": (c_size_t, _i),
    "cp_pnp_from_post_workspace_bytes": (c_size_t, _i * 2),
    "cp_pnp_from_post": (c_int, _vp * 3 + _i * 3 + _vp * 2 + _ws),
    "cp_pnp_solve": (c_int, _vp * 4 + _i * 2 + _vp + _ws),
    "cp_track_state_bytes": (c_size_t, _i * 2),
    "cp_track_workspace_bytes": (c_size_t, _i * 3),
    "cp_track_reset": (c_int, _vp * 2 + _i * 2),
    "cp_track_status": (c_int, _vp * 2 + _i + _pi),
    "cp_track_step": (c_int, _vp + [POINTER(TrackParams)] + _vp * 4 + _i + _vp * 2 + _ws),
    "cp_track_seed": (c_int, _vp + [POINTER(TrackParams)] + _vp * 4 + _i * 2 + _vp * 2),
    "cp_linear_assignment": (c_int, _vp + _i * 3 + _pi),
    "cp_box_iou": (c_int, _vp * 3 + _i + _vp),
    "cp_box_eval": (c_int, _vp * 7 + _i * 2 + _vp),
    "cp_pose_loss_workspace_bytes": (c_size_t, [POINTER(PoseLossDesc)]),
    "cp_pose_loss_forward": (c_int, _vp + [POINTER(PoseLossDesc)] + _vp * 4 + _ws),
    "cp_pose_loss_backward": (c_int, _vp + [POINTER(PoseLossDesc)] + _vp + _pvp * 2 + _ws),
    "cp_pose_targets_workspace_bytes": (c_size_t, [POINTER(PoseTargetsDesc)]),
    "cp_pose_targets": (c_int, _vp + [POINTER(PoseTargetsDesc)] + _ws),
    "cp_pose_targets_track_workspace_bytes": (c_size_t, [POINTER(PoseTargetsTrackDesc)]),
    "cp_pose_targets_track": (c_int, _vp + [POINTER(PoseTargetsTrackDesc)] + _ws),
    "cp_pose_targets_track_det_workspace_bytes": (c_size_t, [POINTER(PoseTargetsTrackDetDesc)]),
    "cp_pose_targets_track_det": (c_int, _vp + [POINTER(PoseTargetsTrackDetDesc)] + _ws),
    "cp_train_inputs_workspace_bytes": (c_size_t, _i * 3),
    "cp_train_inputs": (c_int, _vp * 2 + [c_size_t] + _vp + _i + _pf * 2 + _vp + _i * 2 + _ws),
    "cp_adam_table_bytes": (c_size_t, _i + [POINTER(c_int64)] + _pi * 2),
    "cp_adam_table_build": (c_int, [c_void_p, c_size_t] + _i + _pvp * 4 + [POINTER(c_int64)] + _pi * 2),
    "cp_adam_state_bytes": (c_size_t, _i),
    "cp_adam_workspace_bytes": (c_size_t, _i),
    "cp_adam_step": (c_int, _vp * 2 + _i * 2 + [c_double] * 6 + _i + _vp + _ws),
    "cp_grad_flat_elems": (c_size_t, _i + [POINTER(c_int64)]),
    "cp_grad_flat_offsets": (c_int, _i + [POINTER(c_int64)] * 2),
    "cp_grad_pack_table_bytes": (c_size_t, _i + [POINTER(c_int64)] + _pi),
    "cp_grad_pack_table_build": (c_int, [c_void_p, c_size_t] + _i + _pvp + [POINTER(c_int64)] * 2 + _pi),
    "cp_grad_pack": (c_int, _vp * 2 + _i * 2 + _vp + [c_int64, c_float]),
    "cp_draw_workspace_bytes": (c_size_t, _i * 2),
    "cp_draw_primitives": (c_int, _vp * 2 + _i * 3 + [c_size_t] + _vp + _i + _ws),
    "cp_draw_detections": (c_int, _vp * 5 + _i * 2 + [POINTER(DrawParams)] + _vp),
    "cp_draw_tracks": (c_int, _vp * 2 + _i * 2 + _vp + [POINTER(DrawParams)] + _vp),
}


def _sig(fn, restype, argtypes):
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
    # fail with "rebuild", not with ctypes' "undefined symbol" (an unbound int f(void) is called as ctypes' default)
    if not hasattr(L, "cp_abi_version"):
        raise RuntimeError("centerpose_amd: %s predates the ABI guard (no cp_abi_version): rebuild the library" % LIB_PATH)
    if L.cp_abi_version() != ABI_VERSION:
        raise RuntimeError("centerpose_amd: %s has ABI version %d, this binding was written for %d (rebuild the library)"
                           % (LIB_PATH, L.cp_abi_version(), ABI_VERSION))
    for name, (restype, argtypes) in SIGNATURES.items():
        _sig(getattr(L, name), restype, argtypes)
    _lib = L
    return L


def exported_symbols():
    """Names every declaration in include/centerpose_hip.h (+ the test hook of centerpose_hip_testing.h) must resolve to (used by CPU tests)."""
    return list(SIGNATURES)


def _check(rc, what):
    if rc != 0:
        msg = lib().cp_last_error().decode() if _lib is not None else ""
        raise RuntimeError("centerpose_hip: %s failed with code %d (%s)" % (what, rc, msg))


def _check_args(rc, what):
    """``_check``, with CP_ERR_INVALID (arguments the library refused before any launch) as a ValueError."""
    if rc == CP_ERR_INVALID:
        raise ValueError("centerpose_hip: %s: %s" % (what, lib().cp_last_error().decode()))
    _check(rc, what)


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _ptrs(*ts):
    return [_ptr(t) for t in ts]


def _float3(v):
    """A per-channel mean / std (anything numpy reads) as the float[3] the preprocessing entry points take."""
    import numpy as np

    return (c_float * 3)(*[float(x) for x in np.asarray(v).reshape(-1)])


def _on_device(*ts, what="centerpose_hip"):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("%s: tensors must live on the HIP device (no CPU path)" % what)


def _dev(t):
    _on_device(t)
    return t.contiguous().float()


def _dev_opt(t):
    return _dev(t) if t is not None else None


def _nhwc_view(feat):
    """[B,C,H,W] tensor -> the same values as NHWC memory ([B,C,H,W] tensor in channels_last format; no copy when it already is)."""
    _on_device(feat)
    if feat.dim() != 4:
        raise RuntimeError("pose_heads: feat must be [B, Cin, H, W]")
    return feat.float().contiguous(memory_format=torch.channels_last)


def _check_shapes(what, items, exc=RuntimeError):
    """``items``: (name, tensor or None, expected shape); the first tensor of another shape raises ``exc``."""
    for name, t, shape in items:
        if t is not None and tuple(t.shape) != tuple(shape):
            raise exc("%s: %s has shape %s, expected %s" % (what, name, tuple(t.shape), tuple(shape)))


def _refuse(op, last_error=True):
    raise RuntimeError("%s: shape refused by the library%s" % (op, " (%s)" % lib().cp_last_error().decode() if last_error else ""))


def _workspace(nbytes, device, op=None, last_error=True, given=None):
    """The uint8 tensor of a queried workspace size (``given``: the caller's own, used as it is).  A size of 0 is the library
    refusing the shape: with ``op``, the operator's name, that raises here (``_refuse``); without, the launch itself reports
    it."""
    if nbytes == 0 and op is not None:
        _refuse(op, last_error)
    return given if given is not None else torch.empty(nbytes, dtype=torch.uint8, device=device)


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


PRECISIONS = {"f32": 0, "f16x3": 1}


def set_default_precision(name):
    """'f32' (exact float32 MFMA) or 'f16x3' (split-binary16 MFMA, float32-class accuracy)."""
    _check(lib().cp_set_default_precision(PRECISIONS[name]), "cp_set_default_precision")
