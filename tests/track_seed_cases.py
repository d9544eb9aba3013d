"""Deterministic seeds (``meta['pre_dets']``) for the 5-frame stub video of oracle/tools/track_golden.py, in the 19-key
format the reference's evaluator builds (tools/objectron_eval/eval_video_official.py:430-449; 'ct' is optional and
``Tracker.init_track`` fills it in).  Shared by tools/make_track_seed_goldens.py (which runs the REFERENCE on them ->
tests/golden/track_run_seeded.json) and by tests/test_track_seed_cpu.py / tests/test_track_seed_gpu.py.

``annotations(f)`` stands for the labels of frame f.  What it holds, in order:
  0  object A of the video, a little off its detection: the detections continue it; given WITH 'ct'
  1  object B, likewise, WITHOUT 'ct' (the tracker takes the box centre)
  2  a cuboid where the video has nothing: it matches no detection, coasts and ages
  3  the same kind of cuboid elsewhere with score 0.05 <= new_thresh: never becomes a track
  4  a long, close cuboid whose `kps_gt` has one vertex left of x = 0 AND one right of x = width: the ground-truth
     branch draws them without a bounds test, centred outside the input.  (Only two of its nine points are outside, so
     `pnp_shell` keeps the filtered pose of the coasting track: a track without 'kps_pnp_kf' would send the
     non-ground-truth branch to 'kps_mean_kf', whose (2, 1) columns current numpy refuses to put into the integer table.)
  5  a cuboid right of the frame: its box clipped to the input is degenerate (w = 0), so nothing is drawn for it, but
     it is a track
Objects A and B follow the video (frame f's labels come from frame f of tests/golden/track_run.json); the others stand still.
"""
import copy
import json
import os

import numpy as np

from oracle import pnp as opnp
from oracle.tools import track_golden as tg

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W = H = 512
MODES = {  # name -> extra argv on top of TRACK_ARGV / BASELINE_ARGV
    "gt_first": ["--gt_pre_hm_hmhp_first"],
    "gt_every": ["--gt_pre_hm_hmhp"],
    "gt_first_empty": ["--gt_pre_hm_hmhp_first", "--empty_pre_hm"],
}
_SHIFT = np.array([1.5, -1.0])   # labels sit this far (pixels) from what the stub network detects


def _bounding_box(pts):
    return np.array([pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()])


def _seed(kps_ori, kps_3d, scale, score=1, with_ct=False):
    """The evaluator's dict from normalised projections [9, 2] (centre first), camera-frame vertices [9, 3], size [3]."""
    kps_ori = np.asarray(kps_ori, np.float64)
    px = kps_ori * np.array([W, H], np.float64)
    kps = px[1:].flatten()
    scale = np.asarray(scale, np.float64)
    d = {"bbox": _bounding_box(px), "score": score, "cls": 0, "obj_scale": scale / scale[1],
         "obj_scale_uncertainty": np.ones(3) * 1e-4, "tracking": np.zeros(2), "tracking_hp": np.zeros(16), "kps": kps,
         "kps_displacement_mean": kps, "kps_displacement_std": np.ones(16) * 1e-4, "kps_heatmap_mean": kps,
         "kps_heatmap_std": np.ones(16) * 1e-4, "kps_heatmap_height": np.ones(8), "kps_fusion_mean": kps,
         "kps_fusion_std": np.ones(16) * 1e-4, "kps_pnp": kps_ori, "kps_gt": kps_ori, "kps_3d_cam": np.asarray(kps_3d, np.float64),
         "kps_ori": kps_ori}
    if with_ct:
        b = d["bbox"]
        d["ct"] = [float((b[0] + b[2]) / 2), float((b[1] + b[3]) / 2)]
    return d


def _cuboid(scale, quat, t, **kw):
    """A posed cuboid seen by the demo camera -> seed."""
    scale = np.asarray(scale, np.float64)
    q = np.asarray(quat, np.float64)
    rvec = opnp.matrix_to_rodrigues(opnp.quat_xyzw_to_matrix(q / np.linalg.norm(q)))
    t = np.asarray(t, np.float64)
    V = np.vstack([np.zeros((1, 3)), opnp.cuboid_vertices(scale)])
    uv = opnp.project_points(V, rvec, t, tg.K_DEMO)
    cam = V @ opnp.rodrigues_to_matrix(rvec).T + t
    return _seed(uv / np.array([W, H], np.float64), cam, scale, **kw)


_video = None


def _video_tracks():
    global _video
    if _video is None:
        with open(os.path.join(GOLD, "track_run.json")) as fh:
            _video = [fr["tracks"] for fr in json.load(fh)["frames"]]
    return _video


def _followed(track, with_ct):
    px = np.asarray(track["kps"], np.float64).reshape(8, 2) + _SHIFT
    px = np.vstack([px.mean(0, keepdims=True), px])
    cam = np.asarray(track["kps_3d_cam_kf"], np.float64).reshape(9, 3)
    return _seed(px / np.array([W, H], np.float64), cam, track["obj_scale_kf"], with_ct=with_ct)


def annotations(f):
    """The seeds that stand for frame f's labels (fresh dicts on every call: ``init_track`` writes into them)."""
    by_id = {t["tracking_id"]: t for t in _video_tracks()[f]}
    return [
        _followed(by_id[1], True),
        _followed(by_id[2], False),
        _cuboid([0.20, 0.25, 0.16], [0.1, 0.3, -0.2, 0.9], [-0.95, 0.2, 3.0]),
        _cuboid([0.22, 0.20, 0.18], [0.3, -0.1, 0.2, 0.9], [0.75, -0.85, 3.1], score=0.05),
        _cuboid([1.22, 0.7, 0.36], [-0.492, -0.473, -0.22, 0.697], [0.03, -0.2, 1.51]),
        _cuboid([0.2, 0.2, 0.2], [0.2, 0.2, 0.1, 0.95], [1.45, 0.1, 3.0]),
    ]


def pre_dets_for(mode, frame_id):
    """What the evaluator puts into meta['pre_dets'] for frame ``frame_id`` (eval_video_official.py:327-456), or None:
    with --gt_pre_hm_hmhp_first only frame 0 gets seeds (its own labels); with --gt_pre_hm_hmhp every frame does -- its own
    labels for frame 0, the previous frame's afterwards."""
    if "--gt_pre_hm_hmhp" in MODES[mode]:
        return annotations(max(frame_id - 1, 0))
    return annotations(0) if frame_id == 0 else None


def frame_inputs(get_affine_transform, mode):
    """tg.frame_inputs with the evaluator's seeds on the frames that get them."""
    out = []
    for img, meta in tg.frame_inputs(get_affine_transform):
        seeds = pre_dets_for(mode, meta["id"])
        if seeds is not None:
            meta = dict(meta, pre_dets=seeds)
        out.append((img, meta))
    return out


def run_video(detector, get_affine_transform, mode):
    """tg.run_video on the seeded frames."""
    out = []
    for img, meta in frame_inputs(get_affine_transform, mode):
        ret = detector.run(img, meta_inp=copy.deepcopy(meta), preprocessed_flag=True)
        out.append(tg.summarise(ret, detector))
    return out
