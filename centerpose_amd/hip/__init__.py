"""ctypes binding of libcenterpose_hip.so (C ABI: include/centerpose_hip.h).

PyTorch-ROCm is only the tensor container / allocator / stream provider here: every call hands raw
``data_ptr()`` device pointers and the current HIP stream to the library.  There is NO fallback:
if the shared library is missing or a call fails, a ``RuntimeError`` is raised.

One job per module -- ``_abi``: the library, the table of its signatures and the primitives the wrappers share;
``_structs``: the header's structs; ``ops``: the stand-alone operators; ``detect``: preprocess to poses; ``model``: the
network; ``track``: the device tracker; ``metrics``: the box metrics; ``train``: loss, targets and input images; ``optim``: the clip + Adam
step and the gradient pack of data-parallel training, reached as ``hip.optim.NAME``; ``sync_norm``: SyncBatchNorm's four
phases, reached as ``hip.sync_norm.NAME``; ``draw``: the overlay, reached as ``hip.draw.NAME`` (the names re-exported here are a recorded surface).  This file only re-exports: callers use ``hip.NAME``, and the modules that time or stub an operator replace ``hip.NAME``.
"""
from . import _abi
from . import draw
from . import optim
from . import sync_norm
from ._abi import (ABI_VERSION, CP_ERR_INVALID, LIB_PATH, PRECISIONS, KernelSel, _dev, _nhwc_view, exported_symbols, lib,
                   select_kernels, set_default_precision)
from ._structs import (PL_HM_HP_MAPS, PL_HPS_UNCERTAINTY, PL_RESIDUAL, PL_SCALE_UNCERTAINTY, PL_VAL, POSE_LOSS_HEADS,
                       POSE_LOSS_MAX_STACKS, POSE_LOSS_STATS, POSE_LOSS_TERMS, PT_FLAGS, PT_IMG, PT_IMG_STRIDE, PT_MAX_OBJS, PT_OBJ,
                       PT_OBJ_STRIDE, PT_OUTPUTS, PTK_CAT_RULE, PTK_CUR, PTK_CUR_STRIDE, PTK_DET_MAX_K, PTK_DET_OPTS, PTK_DISTURB,
                       PTK_DRAW, PTK_FLAGS, PTK_GEN, PTK_GEN_STRIDE, PTK_GEOMETRY, PTK_IMG, PTK_IMG_STRIDE, PTK_NUM_DRAWS,
                       PTK_OUTPUTS, PTK_PRE, PTK_PRE_STRIDE, TI_IMG, TI_ORDERS, TI_STRIDE, PoseLossDesc, PoseTargetsDesc,
                       PoseTargetsTrackDesc, PoseTargetsTrackDetDesc, TrackParams)
from .detect import (DET_FIELDS, DET_STRIDE, PNP_STRIDE, POST_FIELDS, POST_STRIDE, PoseStage, decode_gathered, decode_peaks,
                     decode_raw, decode_raw_tiled, masked_stream, pnp_from_post, pnp_solve, postprocess, preprocess,
                     preprocess_batch, render_gaussians, resize_u8, split_detections)
from .metrics import (BOX_EVAL_FIELDS, BOX_EVAL_STRIDE, BOX_FLAG_CLIP_OVERFLOW, BOX_FLAG_SINGULAR_MO2C, BOX_FLAG_SINGULAR_RAY,
                      box_eval, box_iou)
from .model import HipModel, LazyHeads
from .ops import (CONV_BWD_GENERIC, CONV_BWD_LOWC, CONV_BWD_MFMA, batch_norm_backward, batch_norm_forward, conv2d_backward,
                  conv2d_backward_path, conv2d_nhwc, conv2d_stem_backward, conv_transpose2d, conv_transpose2d_backward_f32 as conv_transpose2d_backward,
                  conv_transpose2d_dw, dcn_backward_is_fast, dcn_v2_backward_f32 as dcn_v2_backward, dcn_v2_forward, deterministic, group_norm_backward,
                  group_norm_forward, gru_gate_backward, gru_gate_forward, max_pool2d_backward, max_pool2d_forward,
                  pose_heads_backward, pose_heads_chunk_images, pose_heads_forward, resolve_deterministic, set_deterministic)
from .track import (SEED_FIELDS, SEED_PRESENT, SEED_STRIDE, TRACK_CAP, TRACK_FIELDS, TRACK_STRIDE, DeviceTracker,
                    linear_assignment, pack_seeds, seed_required_keys, track_params_from_opt, track_record_to_dict, track_vmeta)
from .train import (_pl_used, pose_loss_backward, pose_loss_forward, pose_targets, pose_targets_desc, pose_targets_track,
                    pose_targets_track_desc, pose_targets_track_det, train_inputs, train_inputs_means_offset)
