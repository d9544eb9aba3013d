"""Non-finite inputs of the tracking chain, shared by tests/test_track_nonfinite_cpu.py (host build of track_common.h /
post_common.h) and tests/test_track_nonfinite_gpu.py (cp_track_step / cp_postprocess on the device).

The contract under test ("Non-finite detections"): in the association **a cost that is not a number below
1e18 is a forbidden pair**.  A detection with a non-finite centre or box therefore never matches, may start a track, coasts
and is retired after ``max_age``; the assignment solvers terminate whatever reaches them.

Everything here is data: cost matrices, poisoned copies of the seeded videos of ``make_goldens.tracker_mode`` and the
records of the post-process cases.  Nothing in this module calls the code under test.
"""
import copy

import numpy as np

NAN, INF = float("nan"), float("inf")
FORBIDDEN = 1e18


# ---------------------------------------------------------------------------------------------------------------------
# a. hostile cost matrices
SOLVER_SHAPES = [(4, 5), (5, 4), (1, 1), (1, 6), (12, 12)]
SOLVER_PATTERNS = ["row", "col", "col0", "entry", "all"]
SOLVER_VALUES = {"nan": NAN, "inf": INF, "1e18": FORBIDDEN, "-inf": -INF}   # -inf: harness entry points only


def sanitise(c):
    """The rule of trk_associate / Tracker._associate on a cost matrix."""
    c = np.array(c, np.float64)
    c[~(c < FORBIDDEN)] = FORBIDDEN
    return c


def comparable(c):
    """Sanitised form finite with |c| <= 1e18: the solvers' answers are defined and are compared with the oracles."""
    s = sanitise(c)
    return bool(np.isfinite(s).all() and (np.abs(s) <= FORBIDDEN).all())


def _tracker_like(nd, nt, rng):
    """The tracker's own pattern: squared float32 distances, about a third of the pairs forbidden at exactly 1e18."""
    d32 = (rng.rand(nd, nt) * 90.0).astype(np.float32)
    c = d32 + (rng.rand(nd, nt) < 0.3) * FORBIDDEN
    c[c > FORBIDDEN] = FORBIDDEN
    return np.ascontiguousarray(c, np.float64)


def solver_cases():
    """-> list of (name, matrix).  Every shape x pattern x value, one finite +-1e308 matrix per shape, and the tie-heavy
    worst cases at the device's upper size (100 detections x 128 tracks: all equal, all forbidden)."""
    out = []
    for nd, nt in SOLVER_SHAPES:
        rng = np.random.RandomState(1000 * nd + nt)
        base = _tracker_like(nd, nt, rng)
        for pat in SOLVER_PATTERNS:
            for vname, v in SOLVER_VALUES.items():
                c = base.copy()
                if pat == "row":
                    c[min(1, nd - 1), :] = v
                elif pat == "col":
                    c[:, min(2, nt - 1)] = v
                elif pat == "col0":
                    c[:, 0] = v
                elif pat == "entry":
                    c[nd // 2, nt // 2] = v
                else:
                    c[:, :] = v
                out.append(("%dx%d-%s-%s" % (nd, nt, pat, vname), c))
        big = np.where(rng.rand(nd, nt) < 0.5, 1e308, -1e308)
        out.append(("%dx%d-huge" % (nd, nt), np.ascontiguousarray(big)))
        # column 0 at -1e308, the rest at +1e308: every row reduces to (0, inf, inf, ...), one star, and the first adjustment
        # subtracts inf from inf -- no zero can appear any more, which is the loop Munkres' bounds exist for (n >= 2)
        cols = np.full((nd, nt), 1e308)
        cols[:, 0] = -1e308
        out.append(("%dx%d-hugecols" % (nd, nt), cols))
    out.append(("100x128-equal", np.full((100, 128), 7.0)))
    out.append(("100x128-forbidden", np.full((100, 128), FORBIDDEN)))
    return out


def is_harness_only(name):
    return name.endswith("--inf")


# ---------------------------------------------------------------------------------------------------------------------
# b. poisoned videos (detection dicts of make_goldens.tracker_frames / tracker_frames_ties)
VIDEO_MODES = ["greedy", "hungarian", "hungarian_scipy", "baseline", "baseline_hungarian", "ties_hungarian"]
GPU_MODES = ["greedy", "hungarian", "hungarian_scipy", "baseline_hungarian"]
ASSOC_FIELDS = {"boxct": ("bbox", "ct"), "tracking": ("tracking",)}    # post 24..29 / 46..47
ASSOC_VALUES = {"nan": NAN, "inf": INF}
ASSOC_POSITIONS = ["f2d0", "f1last", "f2all"]   # detection 0 of frame 2 | last detection of frame 1 (its track lands in a
#                                                 later slot) | every detection of frame 2
# the ids of frames 2..4 with detection 0 of frame 2 poisoned in bbox + ct, on the video of make_goldens.tracker_frames():
# the poisoned detection starts track 5, which coasts in frame 3 and is gone in frame 4 (max_age 2)
F2D0_IDS = [[3, 4, 5, 1, 2], [1, 3, 4, 6, 5], [1, 3, 4, 6]]


def _where(position, frames):
    if position == "f2d0":
        return [(2, 0)]
    if position == "f1last":
        return [(1, len(frames[1]) - 1)]
    return [(2, i) for i in range(len(frames[2]))]


def _set(det, key, value):
    old = np.asarray(det[key])
    det[key] = np.full(old.shape, value, old.dtype if old.dtype.kind == "f" else np.float64)


def assoc_cases():
    """-> list of (name, keys, value, position): poison that reaches the association."""
    return [("%s-%s-%s" % (f, v, p), ASSOC_FIELDS[f], ASSOC_VALUES[v], p)
            for f in ASSOC_FIELDS for v in ASSOC_VALUES for p in ASSOC_POSITIONS]


# payload poison: the centre and the box stay finite, so the association must not notice.  (key, name, value or vector)
PAYLOAD_CASES = [
    ("kps_fusion_mean", "nan", NAN), ("kps_fusion_mean", "inf", INF), ("kps_fusion_mean", "-inf", -INF),
    ("kps_fusion_std", "nan", NAN), ("kps_fusion_std", "inf", INF), ("kps_fusion_std", "-inf", -INF),
    ("kps_fusion_std", "zero", 0.0), ("kps_fusion_std", "negative", -1.5),
    ("obj_scale", "nan", NAN), ("obj_scale", "inf", INF), ("obj_scale", "-inf", -INF),
    ("obj_scale_uncertainty", "nan", NAN), ("obj_scale_uncertainty", "inf", INF), ("obj_scale_uncertainty", "-inf", -INF),
    ("obj_scale_uncertainty", "zero", 0.0),
]
PAYLOAD_AT = (1, 0)   # detection 0 of frame 1: a strong detection whose track is matched again in the frames that follow


def poisoned(frames, where, keys, value):
    """Deep copy of `frames` with `keys` of the detections `where` = [(frame, index)] set to `value`."""
    out = copy.deepcopy(frames)
    for f, i in where:
        for k in keys:
            _set(out[f][i], k, value)
    return out


def assoc_video(frames, keys, value, position):
    where = _where(position, frames)
    return poisoned(frames, where, keys, value), where


def score_video(frames, frame, index, value):
    out = copy.deepcopy(frames)
    out[frame][index]["score"] = value
    return out


# ---------------------------------------------------------------------------------------------------------------------
# c. post-process records: K = 8 decode records (float32 [8, 118]) whose scores / boxes are poisoned.
# decode layout (include/centerpose_hip.h: cp_decode): 0:4 bbox | 4 score | ...
POST_K = 8
POST_CASES = {
    # name -> list of (record, field, value); field "score" or "box" (all four) or "x2" (one corner)
    "score-nan": [(1, "score", NAN)],
    "score-inf": [(2, "score", INF)],
    "score--inf": [(3, "score", -INF)],
    "box-nan": [(1, "box", NAN)],
    "box-inf": [(2, "box", INF)],
    "corner-nan": [(0, "x2", NAN)],
    "corner-inf": [(4, "x2", INF)],
    "mixed": [(0, "score", INF), (1, "box", NAN), (2, "score", NAN), (5, "x2", INF), (6, "box", -INF)],
}


def post_inputs(dets, b=0, case=None):
    """Image `b` of make_goldens.host_cases() cut to POST_K records that all overlap (record k = record 0's box moved by
    1.5 k output pixels, scores 0.9 .. 0.45: the Gaussian soft-NMS decays and removes some of them), then poisoned as
    POST_CASES[case] says.  -> (decode dict of [1, POST_K, w] arrays for the Python mirror, raw float32 [POST_K, 118])."""
    from centerpose_amd import hip

    d = {k: np.array(v[b:b + 1, :POST_K], np.float32) for k, v in dets.items()}
    d["bboxes"] = d["bboxes"][:, :1] + 1.5 * np.arange(POST_K, dtype=np.float32)[None, :, None]
    d["scores"] = np.linspace(0.9, 0.45, POST_K, dtype=np.float32).reshape(d["scores"].shape)
    for k, field, value in POST_CASES.get(case, []):
        if field == "score":
            d["scores"].reshape(-1)[k] = value
        elif field == "box":
            d["bboxes"][0, k, :] = value
        else:
            d["bboxes"][0, k, 2] = value
    raw = np.zeros((POST_K, hip.DET_STRIDE), np.float32)
    for key, (off, w) in hip.DET_FIELDS.items():
        raw[:, off:off + w] = d[key].reshape(POST_K, w)
    return d, raw
