"""ObjectPose training targets on the device: the ground truth that ObjectPoseDataset.__getitem__ builds for the current
frame (datasets/dataset_combined.py:957-1130), for a whole batch and every symmetry variant, computed by cp_pose_targets.

The host keeps image decoding, the augmentation draws and the output affine (the input image itself, warp and colour
augmentation included, can be built on the device too: train_inputs.py).  A dataset returns, per image, the input or
the decoded frame plus the small fixed-size records of ``pack_annotations`` (the default collate stacks them); the
training step expands them on the device:

    records = pack_annotations(anns, trans_output_rot, width, height, flipped, rot, opt)   # per image, in the dataset
    batch.update(PoseTargets(opt)(collated_records))                                       # per batch, on the device

The returned dict has the keys, dtypes and [B, S, ...] shapes of the reference's collated ``ret`` (float32 maps and
regression targets, uint8 reg_mask / hps_mask, int64 ind / hp_ind / hp_mask), gated by the same ``opt`` flags, so
ObjectPoseLoss reads it as it reads the reference's.
"""
import numpy as np
import torch

from . import hip

NUM_JOINTS = 8
MAX_OBJS = 10  # ObjectPoseDataset.max_objs (dataset_combined.py:128)

_REFUSED = (("tracking_task", "opt.tracking_task: the previous-frame targets depend on frame sampling and random draws on "
                              "the host; pose_targets_track.TrackPoseTargets builds them from packed draws"),
            ("pre_hm", "opt.pre_hm: a previous-frame render"),
            ("pre_hm_hp", "opt.pre_hm_hp: a previous-frame render"),
            ("tracking", "opt.tracking: needs the previous frame's matched centres"),
            ("tracking_hp", "opt.tracking_hp: needs the previous frame's matched keypoints"),
            ("dense_hp", "opt.dense_hp: the dense keypoint maps (ObjectPoseLoss refuses it as well)"),
            ("mse_loss", "opt.mse_loss: the fixed hm_gauss radius (ObjectPoseLoss refuses it as well)"))


def num_symmetry(opt):
    """S, the category's variant count (dataset_combined.py:357-366)."""
    if opt.c == "chair":
        return 4
    if (opt.c == "cup" and not opt.mug) or opt.c == "bottle":
        return int(opt.num_symmetry)
    return 1


def pack_annotations(anns, trans_output_rot, width, height, flipped, rot, opt, max_objs=MAX_OBJS, _nsym0=None):
    """The per-image records of cp_pose_targets (layouts in include/centerpose_hip.h), on the host in numpy:
    {'pt_image': float64 [32], 'pt_objects': float64 [max_objs, 64]}.  ``anns`` is the image's annotation JSON,
    ``trans_output_rot`` the 2x3 output affine, ``width`` / ``height`` the decoded image's size, ``flipped`` / ``rot`` the
    augmentation's draws.  Each object's variant count is resolved here as the reference's loop does (:962-966): 4 or 1
    from its 'symmetric' key, else the value left by the previous object (the category's S for the first); a count
    above S raises ValueError."""
    S = num_symmetry(opt)
    objs = anns["objects"]
    n = min(len(objs), max_objs)
    img = np.zeros(hip.PT_IMG_STRIDE, np.float64)
    I, O = hip.PT_IMG, hip.PT_OBJ
    img[I["trans"]:I["trans"] + 6] = np.asarray(trans_output_rot, np.float64).reshape(6)
    img[I["width"]], img[I["height"]] = width, height
    img[I["flipped"]], img[I["rot"]], img[I["num_objs"]] = float(bool(flipped)), float(rot), n
    img[I["proj"]:I["proj"] + 16] = np.asarray(anns["camera_data"]["camera_projection_matrix"], np.float64).reshape(16)
    obj = np.zeros((max_objs, hip.PT_OBJ_STRIDE), np.float64)
    nsym = S if _nsym0 is None else _nsym0  # pack_track_annotations: the count the previous frame's loop left
    for k in range(n):
        ann = objs[k]
        if "symmetric" in ann:
            nsym = 4 if ann["symmetric"] == "True" else 1
        if nsym > S:
            raise ValueError("pack_annotations: object %d has %d symmetry variants, the category (%s) has S = %d"
                             % (k, nsym, opt.c, S))
        o = obj[k]
        o[O["nsym"]] = nsym
        o[O["cuboid"]:O["cuboid"] + 18] = np.asarray(ann["projected_cuboid"], np.float64).reshape(18)
        if nsym != 1:  # read only by the variant projection
            o[O["quat"]:O["quat"] + 4] = np.asarray(ann["quaternion_xyzw"], np.float64)
            o[O["loc"]:O["loc"] + 3] = np.asarray(ann["location"], np.float64)
            o[O["kps3d"]:O["kps3d"] + 27] = np.asarray(ann["keypoints_3d"], np.float64).reshape(27)
        if opt.obj_scale:
            o[O["scale"]:O["scale"] + 3] = np.asarray(ann["scale"], np.float64)
    return {"pt_image": img, "pt_objects": obj}


def target_keys(opt):
    """The keys of the reference's ``ret`` (:1133-1172) that the targets fill, in its order."""
    keys = ["hm", "reg_mask", "ind", "hps", "hps_mask"]
    if opt.hps_uncertainty:
        keys.append("hps_uncertainty")
    if opt.obj_scale:
        keys.append("scale")
        if opt.obj_scale_uncertainty:
            keys.append("scale_uncertainty")
    if opt.reg_bbox:
        keys.append("wh")
    if opt.reg_offset:
        keys.append("reg")
    if opt.hm_hp:
        keys.append("hm_hp")
    if opt.reg_hp_offset:
        keys += ["hp_offset", "hp_ind", "hp_mask"]
    return keys


class PoseTargets:
    """Expands collated ``pack_annotations`` records into the batch's training targets on the device.  Refuses, at
    construction, what the device path does not build: the tracking task and its targets, dense_hp, mse_loss, and the
    meta / gt_det record of a split other than 'train' (or opt.debug > 0)."""

    def __init__(self, opt, split="train", max_objs=MAX_OBJS):
        for name, why in _REFUSED:
            if getattr(opt, name, False):
                raise NotImplementedError("PoseTargets on the device: %s" % why)
        if split != "train" or getattr(opt, "debug", 0) > 0:
            raise NotImplementedError("PoseTargets on the device: split %r / opt.debug > 0 add the meta record (gt_det), "
                                      "which is not built" % split)
        if not 1 <= max_objs <= hip.PT_MAX_OBJS:
            raise ValueError("PoseTargets: max_objs must be in [1, %d]" % hip.PT_MAX_OBJS)
        self.opt, self.S, self.R, self.K = opt, num_symmetry(opt), int(opt.output_res), int(max_objs)
        self.keys = target_keys(opt)

    def __call__(self, records, device=None):
        """``records``: {'pt_image': [B, 32], 'pt_objects': [B, K, 64]} (tensors or arrays on the host).  Returns
        {key: device tensor} on ``device`` (default: the current HIP device), written on the current stream."""
        img = records["pt_image"]
        obj = records["pt_objects"]
        img = img.cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
        obj = obj.cpu().numpy() if torch.is_tensor(obj) else np.asarray(obj)
        if obj.ndim != 3 or obj.shape[1] != self.K:
            raise ValueError("PoseTargets: pt_objects must be [B, %d, %d]" % (self.K, hip.PT_OBJ_STRIDE))
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        B, S, K, R, J = img.shape[0], self.S, self.K, self.R, NUM_JOINTS
        f32, u8, i64 = torch.float32, torch.uint8, torch.int64
        spec = {"hm": ((B, S, 1, R, R), f32), "hm_hp": ((B, S, J, R, R), f32), "reg_mask": ((B, S, K), u8),
                "ind": ((B, S, K), i64), "hps": ((B, S, K, 2 * J), f32), "hps_mask": ((B, S, K, 2 * J), u8),
                "hps_uncertainty": ((B, S, K, 2 * J), f32), "wh": ((B, S, K, 2), f32), "reg": ((B, S, K, 2), f32),
                "scale": ((B, S, K, 3), f32), "scale_uncertainty": ((B, S, K, 3), f32),
                "hp_offset": ((B, S, K * J, 2), f32), "hp_ind": ((B, S, K * J), i64), "hp_mask": ((B, S, K * J), i64)}
        out = {k: torch.empty(spec[k][0], dtype=spec[k][1], device=dev) for k in self.keys}
        opt = self.opt
        flags = {"center_3D": opt.center_3D, "use_absolute_scale": opt.use_absolute_scale, "obj_scale": opt.obj_scale,
                 "hps_uncertainty": opt.hps_uncertainty, "reg_hp_offset": opt.reg_hp_offset, "hm_hp": opt.hm_hp}
        hip.pose_targets(img, obj, S, R, flags, out)
        return out
