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

With opt.data_generation_mode_ratio > 0 (main_CenterPoseTrack.py:185-188 sets 0.3 for six of the nine categories) a
share of the samples takes the previous frame's heat-maps and labels from a trained CenterPose detector instead of the
simulated noise (data_generation_mode 1, :464-550 and the branches of the per-object loop).  The dataset then draws the
mode and hands the packer what the detector's post-process needs; the detector runs once per batch, on the device:

    mode = draw_generation_mode(None, opt.data_generation_mode_ratio)
    same = opt.same_aug_pre and frame_dist != 0
    records = pack_track_annotations(..., draws, generation=dict(
        mode=mode, c=c if same else c_pre, s=s if same else s_pre, aug_s=aug_s if same else aug_s_pre,
        intrinsics=anns_pre["camera_data"]["intrinsics"]))
    targets = TrackPoseTargets(opt, detector=HipModel("dlav1_34", heads, state_dict))
    batch.update(targets(collated_records, pre_img=batch["pre_img"]))      # pre_img: TrainInputs' previous frames

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


def draw_generation_mode(rng, ratio):
    """The per-sample draw of :465: 1 (the detector's boxes) when a uniform in [0, 1) falls below ``ratio``, else 0 (the
    simulated noise).  ``rng`` as draw_track_noise's.  The uniform is drawn whatever the ratio, as the reference does."""
    r = np.random if rng is None else rng
    return 1 if r.random() < ratio else 0


def _mug_skip(opt, ann):
    return bool((opt.mug == False and ann["mug"] == True) or (opt.mug == True and ann["mug"] == False))  # noqa: E712


def pack_track_annotations(anns, anns_pre, trans_output_rot, trans_input_pre, width, height, flipped, rot, opt, draws,
                           max_objs=MAX_OBJS, max_pre_objs=None, generation=None):
    """The per-sample records of cp_pose_targets_track (layouts in include/centerpose_hip.h), on the host in numpy:
    pack_annotations' {'pt_image', 'pt_objects'} plus {'ptk_image': float64 [32], 'ptk_pre_objects': float64
    [max_pre_objs, 128], 'ptk_cur_objects': float64 [max_objs, 2]}.  ``anns_pre`` / ``trans_input_pre`` are the previous
    frame's annotation JSON and 2x3 input affine, ``draws`` the array of draw_track_noise for its objects.

    ``generation``: None for the noise-simulation mode, with exactly the records above; or, for a dataset that trains
    with opt.data_generation_mode_ratio > 0, a dict for EVERY sample (so that the batch collates) with 'mode' (0 / 1,
    draw_generation_mode; default 1), 'c' and 's' (the previous frame's augmentation centre and extent: c, s when
    same_aug_pre and frame_dist != 0, else c_pre, s_pre, :478-489), 'aug_s' (the radius scale of :681-690: aug_s or
    aug_s_pre by the same rule) and 'intrinsics' (anns_pre['camera_data']['intrinsics'], :469-473).  It adds 'ptk_gen':
    float64 [4] = (mode, aug_s, 0, 0) and 'ptk_det_meta': float64 [12] = cp_postprocess's meta of the detector run on
    img_pre, get_affine_transform(c, s, 0, (output_res, output_res), inv=1) (6), s / output_res, 0 -- the reference's
    post-process ignores the rotation here (utils/post_process.py transform_preds) and so does this -- then the camera
    fx, fy, cx, cy.

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
    if generation is not None:
        from .lib.utils.image import get_affine_transform
        from .lib.utils.post_process import length_ratio

        mode = int(generation.get("mode", 1))
        if mode not in (0, 1):
            raise ValueError("pack_track_annotations: generation['mode'] must be 0 or 1")
        R = int(opt.output_res)
        gen = np.zeros(hip.PTK_GEN_STRIDE, np.float64)
        gen[hip.PTK_GEN["mode"]], gen[hip.PTK_GEN["radius_scale"]] = mode, float(generation["aug_s"])
        meta = np.zeros(12, np.float64)
        meta[:6] = get_affine_transform(generation["c"], generation["s"], 0, (R, R), inv=1).reshape(-1)
        meta[6] = length_ratio(generation["s"], R, R)
        k = generation["intrinsics"]
        meta[8:12] = k["fx"], k["fy"], k["cx"], k["cy"]
        recs.update({"ptk_gen": gen, "ptk_det_meta": meta})
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

    ``detector``: a dlav1_34 ``hip.HipModel`` (or a module with ``_engine()``, such as lib.models' HipPoseNet) built
    without pre_img, as :144-154 build the reference's; for the cup category the caller passes the cup or the mug model,
    whichever opt.mug selects (:496-501).  With it, opt.data_generation_mode_ratio > 0 is accepted: the images whose
    record is in data generation mode 1 take the previous frame's heat-maps and labels from the detector's boxes
    (cp_pose_targets_track_det).  ``det_opt`` supplies the detector's vis_thresh, nms, K and rep_mode (defaults: those of
    opts().init, 0.3 / False / 100 / 1, the values :144-154 leave).

    Refuses, at construction, what the device path does not build: opt.data_generation_mode_ratio > 0 without a
    detector, a rep_mode 2 detector (its sampled PnP points stay on the host), dense_hp, mse_loss, and the meta / gt_det
    record of a split other than 'train' (or opt.debug > 0, which also covers the reference's debug pictures of the
    detector's boxes).  Without opt.tracking_task the reference builds none of this: use pose_targets.PoseTargets."""

    def __init__(self, opt, split="train", max_objs=MAX_OBJS, max_pre_objs=None, detector=None, det_opt=None):
        if not getattr(opt, "tracking_task", False):
            raise ValueError("TrackPoseTargets: opt.tracking_task is off; PoseTargets builds the current frame's targets")
        if getattr(opt, "data_generation_mode_ratio", 0) > 0 and detector is None:
            raise NotImplementedError("TrackPoseTargets on the device: opt.data_generation_mode_ratio > 0 runs a detector "
                                      "on the previous frame (data_generation_mode 1); pass detector=, a dlav1_34 "
                                      "HipModel built without pre_img")
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
        self.detector = None
        if detector is not None:
            g = (lambda n, dflt: getattr(det_opt, n, dflt)) if det_opt is not None else (lambda n, dflt: dflt)
            self.det = {"vis_thresh": float(g("vis_thresh", 0.3)), "nms": bool(g("nms", False)), "K": int(g("K", 100)),
                        "rep_mode": int(g("rep_mode", 1))}
            bc = g("balance_coefficient", 2.0)  # the decode's remaining options (models/decode.py), the reference's defaults
            self.decode = {"balance": float(bc[opt.c] if isinstance(bc, dict) else bc),
                           "legacy_bool_mask": bool(g("legacy_bool_mask", False))}
            if self.det["rep_mode"] == 2:
                raise NotImplementedError("TrackPoseTargets on the device: a rep_mode 2 detector (PnP on points sampled "
                                          "from a Gaussian mixture on the host) is not built")
            if self.det["rep_mode"] not in (0, 1, 3, 4):
                raise ValueError("TrackPoseTargets: det_opt.rep_mode must be 0, 1, 3 or 4")
            if not 1 <= self.det["K"] <= hip.PTK_DET_MAX_K:
                raise ValueError("TrackPoseTargets: det_opt.K must be in [1, %d]" % hip.PTK_DET_MAX_K)
            if opt.c not in hip.PTK_CAT_RULE:
                raise ValueError("TrackPoseTargets: no pnp_shell visibility rule for category %r" % (opt.c,))
            self.render = {"render_hm_mode": int(getattr(opt, "render_hm_mode", 1)),
                           "render_hmhp_mode": int(getattr(opt, "render_hmhp_mode", 2)),
                           "cat_rule": hip.PTK_CAT_RULE[opt.c]}
            if self.render["render_hm_mode"] not in (0, 1) or self.render["render_hmhp_mode"] not in (0, 1, 2, 3):
                raise ValueError("TrackPoseTargets: opt.render_hm_mode must be 0 / 1 and opt.render_hmhp_mode 0..3")
            self.detector = detector._engine() if hasattr(detector, "_engine") else detector
            if getattr(self.detector, "tracking_task", False) or not hasattr(self.detector, "detect"):
                raise ValueError("TrackPoseTargets: detector must be a HipModel built without the tracking inputs")

    def detect(self, pre_img, det_meta):
        """The detector on the previous frames' input images, all on the device: (post [B, K, 120] float64, count [B]
        int32, pnp [B, K, 40] float64).  ``det_meta``: the collated 'ptk_det_meta' [B, 12] on the host."""
        d = self.det
        # the model replays its launch sequence from a hipGraph on a side stream, which reads the input at a fixed
        # address: the frames are copied into a buffer that lives as long as this object
        graph = torch.cuda.current_stream(pre_img.device) != torch.cuda.default_stream(pre_img.device)
        if graph:
            buf = getattr(self, "_det_in", None)
            if buf is None or buf.shape != pre_img.shape or buf.device != pre_img.device:
                buf = self._det_in = torch.empty_like(pre_img)
            buf.copy_(pre_img, non_blocking=True)
            pre_img = buf
        _, det = self.detector.detect(pre_img, K=d["K"], rep_mode=d["rep_mode"], graph=graph, **self.decode)
        self._det_meta = torch.from_numpy(np.ascontiguousarray(det_meta, np.float64).reshape(-1, 12))  # (kept while in flight)
        meta = self._det_meta.to(pre_img.device, non_blocking=True)
        post, count = hip.postprocess(det, meta[:, :8].contiguous(), d["vis_thresh"], d["nms"])
        return post, count, hip.pnp_from_post(post, count, meta[:, 8:12].contiguous(), d["rep_mode"])

    def __call__(self, records, pre_img=None, device=None, detections=None):
        """``records``: the collated dict of pack_track_annotations (tensors or arrays on the host).  ``pre_img``:
        [B, 3, input_h, input_w] float32 on the device, the previous frames as TrainInputs built them; required when a
        record is in data generation mode 1, and then the detector runs once on the whole batch (a fixed shape, so its
        hipGraph replays; the images in mode 0 ignore its answer).  ``detections``: instead of ``pre_img``, the detector's
        answer where the caller has run it already: (post [B, K, 120] float64, count [B] int32, pnp [B, K, 40] float64)
        device tensors of hip.postprocess / hip.pnp_from_post.  Returns {key: device tensor} on ``device`` (default:
        the current HIP device), written on the current stream, without a host synchronisation."""
        names = ("pt_image", "pt_objects", "ptk_image", "ptk_pre_objects", "ptk_cur_objects", "ptk_gen", "ptk_det_meta")
        recs = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in records.items() if k in names}
        if recs["pt_objects"].ndim != 3 or recs["pt_objects"].shape[1] != self.K:
            raise ValueError("TrackPoseTargets: pt_objects must be [B, %d, %d]" % (self.K, hip.PT_OBJ_STRIDE))
        if recs["ptk_pre_objects"].ndim != 3 or recs["ptk_pre_objects"].shape[1] != self.Kp:
            raise ValueError("TrackPoseTargets: ptk_pre_objects must be [B, %d, %d]" % (self.Kp, hip.PTK_PRE_STRIDE))
        gen = recs.get("ptk_gen")
        use_det = gen is not None and bool(np.any(np.asarray(gen)[:, hip.PTK_GEN["mode"]] != 0))
        if use_det:
            if self.detector is None:
                raise ValueError("TrackPoseTargets: a record is in data generation mode 1 and no detector was given")
            if pre_img is None and detections is None:
                raise ValueError("TrackPoseTargets: a record is in data generation mode 1: pre_img, the previous frames' "
                                 "input images on the device, is required")
            if detections is None and "ptk_det_meta" not in recs:
                raise ValueError("TrackPoseTargets: a record is in data generation mode 1 without 'ptk_det_meta'")
        src = None if not use_det else (detections[0] if detections is not None else pre_img)
        dev = torch.device(device) if device is not None else (
            src.device if use_det else torch.device("cuda", torch.cuda.current_device()))
        opt = self.opt
        B, S, K, R, J = recs["pt_image"].shape[0], self.S, self.K, self.R, NUM_JOINTS
        H, W = int(opt.input_h), int(opt.input_w)
        if use_det and detections is None and not (torch.is_tensor(pre_img) and pre_img.is_cuda and
                                                   pre_img.dtype == torch.float32 and tuple(pre_img.shape) == (B, 3, H, W)):
            raise ValueError("TrackPoseTargets: pre_img must be a float32 device tensor [%d, 3, %d, %d]" % (B, H, W))
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
        if not use_det:
            hip.pose_targets_track(recs, S, R, flags, track, out)
            return out
        post, count, pnp = detections if detections is not None else self.detect(pre_img.contiguous(), recs["ptk_det_meta"])
        det = dict(self.render, post=post, count=count, pnp=pnp)
        hip.pose_targets_track_det(recs, S, R, flags, track, det, out)
        return out
