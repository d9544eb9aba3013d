"""The tracking task's training targets on the device (CenterPoseTrack, opt.tracking_task): what Step 1 of
ObjectPoseDataset.__getitem__ builds from the previous frame in its noise-simulation mode
(datasets/dataset_combined.py:401-954 with data_generation_mode == 0) and what Step 2 reads of it, computed by
cp_pose_targets_track together with the current frame's targets of pose_targets.PoseTargets.

The host keeps the choice of the previous frame, both frames' images and JSON, ``img_pre``, the augmentation draws and the
two affines, and draws the noise: a fixed set of random numbers per previous object.  A dataset returns, per sample,

    draws = draw_track_noise(None, len(anns_pre["objects"]))
    records = pack_track_annotations(anns, anns_pre, trans_output_rot, trans_input_pre, width, height, flipped, rot, opt,
                                     draws)                                                # per image, in the dataset
    batch.update(TrackPoseTargets(opt)(collated_records))                                  # per batch, on the device

and the returned dict has the reference's collated keys: PoseTargets' plus pre_hm, pre_hm_hp [B, C, input_h, input_w],
tracking [B, S, K, 2], tracking_mask [B, S, K], tracking_hp and tracking_hp_mask [B, S, K, 16], gated by the same ``opt``
flags, so PoseNetGRU and ObjectPoseLoss read them directly.
"""
import numpy as np
import torch

from . import hip
from .pose_targets import MAX_OBJS, NUM_JOINTS, num_symmetry, pack_annotations, target_keys

NUM_DRAWS = hip.PTK_NUM_DRAWS + 1  # the kernel's 64 slots and the variant choice's uniform

_REFUSED = (("dense_hp", "opt.dense_hp: the dense keypoint maps (ObjectPoseLoss refuses it as well)"),
            ("mse_loss", "opt.mse_loss: the fixed hm_gauss radius (ObjectPoseLoss refuses it as well)"))


def draw_track_noise(rng, n_pre_objects):
    """The random numbers of one sample's previous frame: float64 [n_pre_objects, 65], per object the 64 slots of
    hip.PTK_DRAW (filled whether or not the object ends up using them) and, last, a uniform u in [0, 1) from which the
    packer takes id_symmetry_pre = int(u * num_symmetry), the uniform choice of np.random.choice(num_symmetry) (:578).
    ``rng``: None (numpy's global state, as the reference), a numpy Generator or a RandomState.

    The distributions are the reference's: scipy.stats.truncnorm(-3, 3) for the centre's and the joints' noise (:715,
    :808), uniform [0, 1) for the lost, heat and false-positive tests (:730, :733, :814, :878, :929), standard normals for
    the false positives' offsets (:881-882, :932-933), uniform(0, 0.3) / uniform(0, 0.4) for their peaks (:888, :937).
    The stream ORDER is not: the reference draws only what an object's branches reach, in loop order, so the same seed
    gives other numbers here."""
    from scipy import stats

    n, D = int(n_pre_objects), hip.PTK_DRAW
    r = np.random if rng is None else rng
    randn = r.standard_normal
    tn = stats.truncnorm(-3, 3)
    out = np.zeros((n, NUM_DRAWS), np.float64)
    if n == 0:
        return out
    J, js = D["joints"], D["joint_stride"]
    out[:, D["ct_noise"]:D["ct_noise"] + 2] = tn.rvs((n, 2), random_state=rng)
    out[:, D["ct_lost"]], out[:, D["ct_heat"]], out[:, D["ct_fp"]] = r.random(n), r.random(n), r.random(n)
    out[:, D["ct_fp_noise"]:D["ct_fp_noise"] + 2] = randn((n, 2))
    out[:, D["ct_fp_peak"]] = r.uniform(0, 0.4, n)
    jt = out[:, J:J + js * NUM_JOINTS].reshape(n, NUM_JOINTS, js)
    jt[:, :, D["j_noise"]:D["j_noise"] + 2] = tn.rvs((n, NUM_JOINTS, 2), random_state=rng)
    jt[:, :, D["j_lost"]], jt[:, :, D["j_fp"]] = r.random((n, NUM_JOINTS)), r.random((n, NUM_JOINTS))
    jt[:, :, D["j_fp_noise"]:D["j_fp_noise"] + 2] = randn((n, NUM_JOINTS, 2))
    jt[:, :, D["j_fp_peak"]] = r.uniform(0, 0.3, (n, NUM_JOINTS))
    out[:, J:J + js * NUM_JOINTS] = jt.reshape(n, -1)
    out[:, hip.PTK_NUM_DRAWS] = r.random(n)
    return out


def _mug_skip(opt, ann):
    return bool((opt.mug == False and ann["mug"] == True) or (opt.mug == True and ann["mug"] == False))  # noqa: E712


def pack_track_annotations(anns, anns_pre, trans_output_rot, trans_input_pre, width, height, flipped, rot, opt, draws,
                           max_objs=MAX_OBJS, max_pre_objs=None):
    """The per-sample records of cp_pose_targets_track (layouts in include/centerpose_hip.h), on the host in numpy:
    pack_annotations' {'pt_image', 'pt_objects'} plus {'ptk_image': float64 [32], 'ptk_pre_objects': float64
    [max_pre_objs, 128], 'ptk_cur_objects': float64 [max_objs, 2]}.  ``anns_pre`` / ``trans_input_pre`` are the previous
    frame's annotation JSON and 2x3 input affine, ``draws`` the array of draw_track_noise for its objects.

    Resolved here, as the reference's two loops do: each object's variant count, carried ACROSS the frames (the
    reference's ``num_symmetry`` variable leaves the previous frame's loop with the last object's value and enters the
    current frame's, :561-565, :962-966); id_symmetry_pre; the cup / mug skip of a previous object (:567-571) and of the
    current frame, which reads the LAST previous object's 'mug' (:968-972); the track ids opt.c + name.split('_')[1] as
    small integers per sample.

    ValueError: more previous objects than ``max_pre_objs`` (default ``max_objs``; dropping some would change the result
    silently), a variant count above S, a current object with more than one variant at an index the previous frame does
    not have while opt.pre_hm_hp is on (the reference raises IndexError at :986), and the cup category with an empty
    previous frame (the reference raises NameError at :970)."""
    S = num_symmetry(opt)
    Kp = int(max_objs if max_pre_objs is None else max_pre_objs)
    pre = anns_pre["objects"]
    if len(pre) > Kp:
        raise ValueError("pack_track_annotations: the previous frame has %d objects, max_pre_objs is %d" % (len(pre), Kp))
    draws = np.asarray(draws, np.float64)
    if draws.shape != (len(pre), NUM_DRAWS):
        raise ValueError("pack_track_annotations: draws must be [%d, %d] (draw_track_noise)" % (len(pre), NUM_DRAWS))
    I, P, O, C = hip.PTK_IMG, hip.PTK_PRE, hip.PT_OBJ, hip.PTK_CUR
    img = np.zeros(hip.PTK_IMG_STRIDE, np.float64)
    img[I["trans"]:I["trans"] + 6] = np.asarray(trans_input_pre, np.float64).reshape(6)
    img[I["num_pre"]] = len(pre)
    img[I["proj"]:I["proj"] + 16] = np.asarray(anns_pre["camera_data"]["camera_projection_matrix"], np.float64).reshape(16)
    codes = {}

    def code(ann):
        return codes.setdefault(opt.c + ann["name"].split("_")[1], len(codes))

    pobj = np.zeros((Kp, hip.PTK_PRE_STRIDE), np.float64)
    nsym = S
    for k, ann in enumerate(pre):
        if "symmetric" in ann:
            nsym = 4 if ann["symmetric"] == "True" else 1
        if nsym > S:
            raise ValueError("pack_track_annotations: previous object %d has %d symmetry variants, the category (%s) has "
                             "S = %d" % (k, nsym, opt.c, S))
        o = pobj[k]
        o[O["nsym"]] = nsym
        o[P["skip"]] = float(opt.c == "cup" and _mug_skip(opt, ann))
        o[P["idsym"]] = min(int(draws[k, hip.PTK_NUM_DRAWS] * nsym), nsym - 1)
        o[P["id"]] = code(ann)
        o[O["cuboid"]:O["cuboid"] + 18] = np.asarray(ann["projected_cuboid"], np.float64).reshape(18)
        if nsym != 1:
            o[O["quat"]:O["quat"] + 4] = np.asarray(ann["quaternion_xyzw"], np.float64)
            o[O["loc"]:O["loc"] + 3] = np.asarray(ann["location"], np.float64)
            o[O["kps3d"]:O["kps3d"] + 27] = np.asarray(ann["keypoints_3d"], np.float64).reshape(27)
        o[P["draws"]:P["draws"] + hip.PTK_NUM_DRAWS] = draws[k, :hip.PTK_NUM_DRAWS]
    recs = pack_annotations(anns, trans_output_rot, width, height, flipped, rot, opt, max_objs, _nsym0=nsym)
    n = int(recs["pt_image"][hip.PT_IMG["num_objs"]])
    cobj = np.zeros((max_objs, hip.PTK_CUR_STRIDE), np.float64)
    skip = False
    if opt.c == "cup" and n:
        if not pre:
            raise ValueError("pack_track_annotations: the cup category needs a previous object ('mug' of the last one)")
        skip = _mug_skip(opt, pre[-1])
    need_name = bool(opt.tracking or opt.tracking_hp)
    for k in range(n):
        ann = anns["objects"][k]
        cobj[k, C["id"]] = code(ann) if need_name or "name" in ann else -1
        cobj[k, C["skip"]] = float(skip)
        if opt.pre_hm_hp and not skip and recs["pt_objects"][k, O["nsym"]] != 1 and k >= len(pre):
            raise ValueError("pack_track_annotations: current object %d has %d variants and the previous frame only %d "
                             "objects (id_symmetry_pre_list[%d])" % (k, recs["pt_objects"][k, O["nsym"]], len(pre), k))
    recs.update({"ptk_image": img, "ptk_pre_objects": pobj, "ptk_cur_objects": cobj})
    return recs


def track_target_keys(opt):
    """The keys of the reference's ``ret`` (:1162-1200) that the targets fill (pre_img stays with the host)."""
    keys = target_keys(opt)
    keys += [k for k in ("pre_hm", "pre_hm_hp") if getattr(opt, k)]
    if opt.tracking:
        keys += ["tracking", "tracking_mask"]
    if opt.tracking_hp:
        keys += ["tracking_hp", "tracking_hp_mask"]
    return keys


class TrackPoseTargets:
    """Expands collated ``pack_track_annotations`` records into the tracking task's training targets on the device.
    Refuses, at construction, what the device path does not build: the detector-in-the-loop generation mode
    (opt.data_generation_mode_ratio > 0), dense_hp, mse_loss, and the meta / gt_det record of a split other than 'train'
    (or opt.debug > 0).  Without opt.tracking_task the reference builds none of this: use pose_targets.PoseTargets."""

    def __init__(self, opt, split="train", max_objs=MAX_OBJS, max_pre_objs=None):
        if not getattr(opt, "tracking_task", False):
            raise ValueError("TrackPoseTargets: opt.tracking_task is off; PoseTargets builds the current frame's targets")
        if getattr(opt, "data_generation_mode_ratio", 0) > 0:
            raise NotImplementedError("TrackPoseTargets on the device: opt.data_generation_mode_ratio > 0 runs a detector "
                                      "on the previous frame (data_generation_mode 1), which is not built")
        for name, why in _REFUSED:
            if getattr(opt, name, False):
                raise NotImplementedError("TrackPoseTargets on the device: %s" % why)
        if split != "train" or getattr(opt, "debug", 0) > 0:
            raise NotImplementedError("TrackPoseTargets on the device: split %r / opt.debug > 0 add the meta record "
                                      "(gt_det), which is not built" % split)
        Kp = max_objs if max_pre_objs is None else max_pre_objs
        if not 1 <= max_objs <= hip.PT_MAX_OBJS or not 1 <= Kp <= hip.PT_MAX_OBJS:
            raise ValueError("TrackPoseTargets: max_objs and max_pre_objs must be in [1, %d]" % hip.PT_MAX_OBJS)
        self.opt, self.S, self.R, self.K, self.Kp = opt, num_symmetry(opt), int(opt.output_res), int(max_objs), int(Kp)
        self.keys = track_target_keys(opt)

    def __call__(self, records, device=None):
        """``records``: the collated dict of pack_track_annotations (tensors or arrays on the host).  Returns
        {key: device tensor} on ``device`` (default: the current HIP device), written on the current stream."""
        recs = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in records.items()
                if k in ("pt_image", "pt_objects", "ptk_image", "ptk_pre_objects", "ptk_cur_objects")}
        if recs["pt_objects"].ndim != 3 or recs["pt_objects"].shape[1] != self.K:
            raise ValueError("TrackPoseTargets: pt_objects must be [B, %d, %d]" % (self.K, hip.PT_OBJ_STRIDE))
        if recs["ptk_pre_objects"].ndim != 3 or recs["ptk_pre_objects"].shape[1] != self.Kp:
            raise ValueError("TrackPoseTargets: ptk_pre_objects must be [B, %d, %d]" % (self.Kp, hip.PTK_PRE_STRIDE))
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        opt = self.opt
        B, S, K, R, J = recs["pt_image"].shape[0], self.S, self.K, self.R, NUM_JOINTS
        H, W = int(opt.input_h), int(opt.input_w)
        f32, u8, i64 = torch.float32, torch.uint8, torch.int64
        spec = {"hm": ((B, S, 1, R, R), f32), "hm_hp": ((B, S, J, R, R), f32), "reg_mask": ((B, S, K), u8),
                "ind": ((B, S, K), i64), "hps": ((B, S, K, 2 * J), f32), "hps_mask": ((B, S, K, 2 * J), u8),
                "hps_uncertainty": ((B, S, K, 2 * J), f32), "wh": ((B, S, K, 2), f32), "reg": ((B, S, K, 2), f32),
                "scale": ((B, S, K, 3), f32), "scale_uncertainty": ((B, S, K, 3), f32),
                "hp_offset": ((B, S, K * J, 2), f32), "hp_ind": ((B, S, K * J), i64), "hp_mask": ((B, S, K * J), i64),
                "pre_hm": ((B, 1, H, W), f32), "pre_hm_hp": ((B, J, H, W), f32), "tracking": ((B, S, K, 2), f32),
                "tracking_mask": ((B, S, K), u8), "tracking_hp": ((B, S, K, 2 * J), f32),
                "tracking_hp_mask": ((B, S, K, 2 * J), u8)}
        out = {k: torch.empty(spec[k][0], dtype=spec[k][1], device=dev) for k in self.keys}
        flags = {"center_3D": opt.center_3D, "use_absolute_scale": opt.use_absolute_scale, "obj_scale": opt.obj_scale,
                 "hps_uncertainty": opt.hps_uncertainty, "reg_hp_offset": opt.reg_hp_offset, "hm_hp": opt.hm_hp}
        track = {n: getattr(opt, n) for n in hip.PTK_FLAGS + hip.PTK_DISTURB}
        track.update(input_w=W, input_h=H, down_ratio=int(opt.down_ratio))
        hip.pose_targets_track(recs, S, R, flags, track, out)
        return out
