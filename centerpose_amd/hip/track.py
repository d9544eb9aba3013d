"""CenterPoseTrack's tracker on the device (cp_track_*): the track and seed record layouts, ``pack_seeds``,
``DeviceTracker``, and the host-side assignment solver."""
import ctypes
from collections import OrderedDict
from ctypes import c_int, c_void_p

import torch

from . import _abi
from ._structs import PTK_CAT_RULE, TrackParams
from .detect import PNP_STRIDE, POST_FIELDS, POST_STRIDE


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
    _abi._check(_abi.lib().cp_linear_assignment(cost.ctypes.data_as(c_void_p), n, m, int(solver), match), "cp_linear_assignment")
    return np.array([(i, match[i]) for i in range(n) if match[i] >= 0], dtype=np.int64).reshape(-1, 2)


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
    lo, hi = opt.conf_border[opt.c][0], opt.conf_border[opt.c][1]
    return TrackParams(new_thresh=opt.new_thresh, pre_thresh=opt.pre_thresh, R=opt.R, conf_lo=lo, conf_hi=hi,
                       max_age=int(opt.max_age), kalman=int(bool(opt.kalman)), scale_pool=int(bool(opt.scale_pool)),
                       use_pnp=int(bool(opt.use_pnp)), hps_uncertainty=int(bool(opt.hps_uncertainty)),
                       show_axes=int(bool(opt.show_axes)), cat_rule=PTK_CAT_RULE[opt.c], render_hm_mode=int(opt.render_hm_mode),
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
        L = _abi.lib()
        self.frames = 0
        self.B, self.P, self.device = int(B), params, device
        self.K, self.cap = int(params.K), int(params.cap)
        self.inp_h, self.inp_w = int(inp_h), int(inp_w)
        self.vmeta = torch.as_tensor(vmeta, dtype=torch.float64).reshape(self.B, 16).contiguous().to(device)
        n_state, n_ws = L.cp_track_state_bytes(self.B, self.cap), L.cp_track_workspace_bytes(self.B, self.K, self.cap)
        if n_state == 0 or n_ws == 0:
            raise RuntimeError("DeviceTracker: unsupported B / K / cap")
        self.state = torch.empty(n_state, dtype=torch.uint8, device=device)
        self.ws = _abi._workspace(n_ws, device)
        self.recs = torch.empty(self.B, self.cap, 9, 5, dtype=torch.float64, device=device)
        self.planes = torch.empty(9 * self.B, self.inp_h, self.inp_w, dtype=torch.float32, device=device)
        self.hdr_bytes = ((4 + 4 * self.B) * 4 + 255) // 256 * 256
        self._seed_ring, self._seed_calls, self._seed_dev = [], 0, None   # staging of seed()
        self.reset()

    def reset(self):
        _abi._check(_abi.lib().cp_track_reset(_abi._stream(), _abi._ptr(self.state), self.B, self.cap), "cp_track_reset")
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
        _abi._check(_abi.lib().cp_track_step(_abi._stream(), ctypes.byref(self.P), *_abi._ptrs(self.vmeta, post, count, det_pnp),
                                             self.B, *_abi._ptrs(self.state, self.recs, self.ws), self.ws.numel()), "cp_track_step")
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
        _abi._check(_abi.lib().cp_track_seed(_abi._stream(), ctypes.byref(self.P), _abi._ptr(self.vmeta), p, p + n_seed,
                                             p + n_seed + 4 * self.B, self.B, S, _abi._ptr(self.state), _abi._ptr(self.recs)),
                    "cp_track_seed")

    def check_due(self):
        """The periodic overflow check of ``step`` (every STATUS_EVERY frames; synchronises when it runs)."""
        if self.STATUS_EVERY and self.frames % self.STATUS_EVERY == 0:  # the device-resident loop never calls read(): surface overflows here
            self.check()

    def dropped(self):
        """Per video: list entries dropped so far because a frame needed more than `cap` tracks (cp_track_status; the
        tracker then keeps the first `cap` entries in the reference's order -- matched, new by score, coasting)."""
        out = (ctypes.c_int * self.B)()
        _abi._check(_abi.lib().cp_track_status(_abi._stream(), _abi._ptr(self.state), self.B, out), "cp_track_status")
        return list(out)

    def check(self):
        d = self.dropped()
        if any(d):
            raise RuntimeError("DeviceTracker: more than cap = %d tracks in a frame of video(s) %s (entries dropped: %s); "
                               "raise cap or the thresholds" % (self.cap, [b for b, v in enumerate(d) if v], [v for v in d if v]))

    def render(self):
        """-> (pre_hm [B,1,H,W], pre_hm_hp [B,8,H,W]) drawn from the current tracks (views of one plane buffer)."""
        B, H, W = self.B, self.inp_h, self.inp_w
        _abi._check(_abi.lib().cp_render_gaussians(_abi._stream(), _abi._ptr(self.recs), B * self.cap * 9, _abi._ptr(self.planes),
                                                   9 * B, H, W, 1), "cp_render_gaussians")
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
