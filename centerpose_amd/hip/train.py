"""The training task on the device: ObjectPoseLoss (cp_pose_loss_*), the training targets (cp_pose_targets, with the
tracking task's and a detector's boxes) and the training input images (cp_train_inputs).  Their descriptors and record
layouts are ``_structs``'s."""
import ctypes
from ctypes import c_void_p

import torch

from . import _abi
from ._structs import (PL_HM_HP_MAPS, PL_HPS_UNCERTAINTY, PL_SCALE_UNCERTAINTY, PL_VAL, POSE_LOSS_HEADS, POSE_LOSS_MAX_STACKS,
                       POSE_LOSS_TERMS, PT_FLAGS, PT_IMG_STRIDE, PT_OBJ_STRIDE, PT_OUTPUTS, PTK_CUR_STRIDE, PTK_DET_OPTS,
                       PTK_DISTURB, PTK_FLAGS, PTK_GEN_STRIDE, PTK_GEOMETRY, PTK_IMG_STRIDE, PTK_OUTPUTS, PTK_PRE_STRIDE, TI_STRIDE,
                       PoseLossDesc, PoseTargetsDesc, PoseTargetsTrackDesc, PoseTargetsTrackDetDesc)
from .detect import PNP_STRIDE, POST_STRIDE

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
    L = _abi.lib()
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
    _abi._check_shapes("pose_loss", [("batch['%s']" % k, batch[k], shapes[k]) for k in keys], ValueError)
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
            _abi._check_shapes("pose_loss", [("outputs[%d]['%s']" % (st, h), t, (B, hchan[h], H, W))], ValueError)
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
        _abi._check(L.cp_pose_loss_forward(_abi._stream(), ctypes.byref(d), None, None, None, None, None, 0), "cp_pose_loss_forward")
    ws = _abi._workspace(nbytes, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    stats = torch.empty(10, dtype=torch.float32, device=dev)
    choice = torch.empty(B, dtype=torch.int64, device=dev)
    tm = torch.empty(9, B, S, dtype=torch.float32, device=dev) if with_terms else None
    _abi._check(L.cp_pose_loss_forward(_abi._stream(), ctypes.byref(d), *_abi._ptrs(loss, stats, choice, tm, ws), nbytes),
                "cp_pose_loss_forward")
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
    _abi._check(_abi.lib().cp_pose_loss_backward(_abi._stream(), ctypes.byref(d), _abi._ptr(dloss), dm, ptrs, _abi._ptr(ws),
                                                 ws.numel()), "cp_pose_loss_backward")
    return grads


def _set_outputs(d, names, out):
    for n in names:
        t = out.get(n)
        setattr(d, "out_" + n, t.data_ptr() if t is not None else None)


def _launch_targets(name, d, device):
    """Size the workspace of the filled descriptor ``d``, then the launch: cp_<name>_workspace_bytes and cp_<name>."""
    L = _abi.lib()
    nbytes = getattr(L, "cp_%s_workspace_bytes" % name)(ctypes.byref(d))
    ws = _abi._workspace(nbytes, device) if nbytes else None
    _abi._check_args(getattr(L, "cp_" + name)(_abi._stream(), ctypes.byref(d), _abi._ptr(ws), nbytes), "cp_" + name)


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
    _set_outputs(d, PT_OUTPUTS, out)
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
    _launch_targets("pose_targets", pose_targets_desc(images, objects, S, R, flags, out), out["hm"].device)


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
    _set_outputs(d, PTK_OUTPUTS, out)
    return d


# the tracking task's host records and the trailing dimensions of each ([B, ...]; None: that batch's K); the detector's adds the last
_PTK_RECORDS = (("pt_image", (PT_IMG_STRIDE,)), ("pt_objects", (None, PT_OBJ_STRIDE)), ("ptk_image", (PTK_IMG_STRIDE,)),
                ("ptk_pre_objects", (None, PTK_PRE_STRIDE)), ("ptk_cur_objects", (None, PTK_CUR_STRIDE)),
                ("ptk_gen", (PTK_GEN_STRIDE,)))


def _track_records(what, records, layout):
    """The host records ``layout`` names as pageable float64 copies, their shapes checked -> ({name: array}, B)."""
    import numpy as np

    recs = {k: np.array(records[k], dtype=np.float64, order="C", copy=True) for k, _ in layout}
    B = recs["pt_image"].shape[0]
    for k, tail in layout:
        a = recs[k]
        if a.ndim != 1 + len(tail) or a.shape[0] != B or a.shape[-1] != tail[-1]:
            raise ValueError("%s: %s must be [B, %s]" % (what, k, ", ".join("K" if t is None else str(t) for t in tail)))
    if recs["ptk_cur_objects"].shape[1] != recs["pt_objects"].shape[1]:
        raise ValueError("%s: ptk_cur_objects and pt_objects must have the same max_objs" % what)
    return recs, B


def pose_targets_track(records, S, R, flags, track, out):
    """cp_pose_targets_track: the tracking task's training targets of a batch, written into the device tensors of ``out``
    on the current stream (arguments as pose_targets_track_desc's; the records are converted to pageable float64 copies
    here, which the call stages before it returns).  Refused arguments raise ValueError before any launch."""
    recs, _ = _track_records("pose_targets_track", records, _PTK_RECORDS[:5])
    _launch_targets("pose_targets_track", pose_targets_track_desc(recs, S, R, flags, track, out), out["hm"].device)


def pose_targets_track_det(records, S, R, flags, track, det, out):
    """cp_pose_targets_track_det: cp_pose_targets_track with a detector's boxes for the images whose ``records['ptk_gen']``
    row asks for data generation mode 1.  ``det``: {'post': [B, K_det, 120] float64, 'count': [B] int32, 'pnp':
    [B, K_det, 40] float64 device tensors of ``postprocess`` / ``pnp_from_post`` on the previous frames' input images,
    'render_hm_mode', 'render_hmhp_mode', 'cat_rule'}.  Everything else as pose_targets_track; refused arguments raise
    ValueError before any launch.  No host synchronisation."""
    recs, B = _track_records("pose_targets_track_det", records, _PTK_RECORDS)
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
    d = PoseTargetsTrackDetDesc()
    d.track = pose_targets_track_desc(recs, S, R, flags, track, out)
    d.det_post, d.det_count, d.det_pnp = post.data_ptr(), count.data_ptr(), pnp.data_ptr()
    d.K_det = K_det
    for n in PTK_DET_OPTS[1:]:
        setattr(d, n, int(det[n]))
    d.gen = recs["ptk_gen"].ctypes.data
    _launch_targets("pose_targets_track_det", d, out["hm"].device)


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
    L = _abi.lib()
    N, out_h, out_w = records.shape[0], int(out.shape[2]), int(out.shape[3])
    nbytes = L.cp_train_inputs_workspace_bytes(N, out_h, out_w)
    ws = _abi._workspace(nbytes, out.device) if nbytes else None
    rc = L.cp_train_inputs(_abi._stream(), _abi._ptr(frames), frames.numel(), records.ctypes.data, N, _abi._float3(mean),
                           _abi._float3(std), _abi._ptr(out), out_h, out_w, _abi._ptr(ws), nbytes)
    _abi._check_args(rc, "cp_train_inputs")
    if return_means:
        o = train_inputs_means_offset(N)
        return out, ws[o:o + 4 * N].view(torch.float32)
    return out
