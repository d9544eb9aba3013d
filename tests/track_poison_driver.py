"""Child process of tests/test_track_nonfinite_cpu.py: runs jobs that could spin -- the assignment solvers on hostile
matrices, whole poisoned videos through the host build of track_common.h and through lib/utils/tracker.py -- so that a
regression ends at the parent's time limit instead of stalling the suite.

    python tests/track_poison_driver.py <libcp_track_host.so> <jobs.pkl> <results.pkl>

jobs: a list of dicts, results: one dict per job.
  {"kind": "solve", "entry": "munkres" | "lsap" | "api1" | "api2", "matrix": float64 [nd, nt]}
      -> {"match": int32 [nd]}  or  {"error": message}           (api*: hip.linear_assignment, solver 1 / 2)
  {"kind": "video", "mode": key of make_goldens.tracker_mode, "frames": detection dicts, "params": overrides,
   "python": run lib/utils/tracker.py as well, "echo_pnp": the filtered PnP is a stand-in that projects every vertex where
   the filter put it (so that with use_pnp = 1 the render reads the filter: position, covariance and fused std)}
      -> {"tracks": [float64 [n, 520] per frame], "recs": [float64 [n, 9, 5] per frame], "py": [summaries per frame]}
"""
import copy
import ctypes
import os
import pickle
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def solve(L, job):
    from centerpose_amd import hip

    c = np.ascontiguousarray(job["matrix"], np.float64)
    nd, nt = c.shape
    if job["entry"] in ("munkres", "lsap"):
        fn = L.cp_track_host_munkres if job["entry"] == "munkres" else L.cp_track_host_lsap
        fn.restype = None
        got = np.full(nd, -7, np.int32)
        fn(_ptr(c), nd, nt, _ptr(got))
        return {"match": got}
    try:
        pairs = hip.linear_assignment(c, 1 if job["entry"] == "api1" else 2)
    except RuntimeError as e:
        return {"error": str(e)}
    got = np.full(nd, -1, np.int32)
    got[pairs[:, 0]] = pairs[:, 1]
    return {"match": got}


def track_params(mode, overrides=None):
    """The parameters of test_tracker_logic_matches_reference_golden for `mode` (+ overrides)."""
    from centerpose_amd import hip
    from oracle.tools import make_goldens as mg

    _, hung, baseline, _ = mg.tracker_mode(mode)
    o = mg.TrackOpt(bool(hung))
    kw = dict(new_thresh=o.new_thresh, pre_thresh=0.3, R=o.R, conf_lo=3, conf_hi=9, max_age=o.max_age, kalman=1,
              scale_pool=1, use_pnp=0, hps_uncertainty=1, show_axes=0, cat_rule=0, render_hm_mode=1, render_hmhp_mode=2,
              pre_hm=1, pre_hm_hp=1, K=100, hungarian=hung, baseline=int(baseline))
    kw.update(overrides or {})
    return hip.TrackParams(**kw)


def video_meta():
    vm = np.zeros(16)
    vm[[0, 4]] = 1.0
    vm[6:10] = 512
    return vm


def echo_pnp(pts, scales):
    """cp_pnp_solve's 40-double rows for `pts` [n, 8, 2]: status 1, unit pose, projected cuboid = the points themselves."""
    rows = np.zeros((len(pts), 40))
    rows[:, 0] = 1.0
    rows[:, 6] = rows[:, 30] = 1.0      # location (0, 0, 1) in both frames
    rows[:, 27] = rows[:, 34] = 1.0     # quaternion (0, 0, 0, 1)
    rows[:, 8:24] = np.asarray(pts, np.float64).reshape(len(pts), 16)
    return rows


def video(L, job):
    from centerpose_amd.lib.utils.tracker import Tracker, Tracker_baseline
    from oracle.tools import make_goldens as mg
    from tests.test_track_logic_cpu import HostTracker, _post_from_dict

    mode = job["mode"]
    _, hung, baseline, solver = mg.tracker_mode(mode)
    L.cp_track_host_update.restype = ctypes.c_int
    ht = HostTracker(L, track_params(mode, job.get("params")), video_meta(), echo_pnp if job.get("echo_pnp") else None)
    py = None
    if job.get("python"):
        opt = mg.TrackOpt(bool(hung))
        opt.hungarian_solver = solver
        py = (Tracker_baseline if baseline else Tracker)(opt)
        py.init_track({"id": 0})
    res = {"tracks": [], "recs": [], "py": []}
    for dets in job["frames"]:
        post = np.stack([_post_from_dict(d, True) for d in dets]) if dets else np.zeros((0, 120))
        tracks, recs = ht.step(post)
        res["tracks"].append(tracks.copy())
        res["recs"].append(recs.copy())
        if py is not None:
            with np.errstate(all="ignore"):
                theirs, _ = py.step(copy.deepcopy(dets))
            res["py"].append([{"tracking_id": int(t["tracking_id"]), "age": int(t["age"]), "active": int(t["active"]),
                               "ct": np.asarray(t["ct"], np.float64).copy(),
                               "kps_mean_kf": np.asarray(t["kps_mean_kf"], np.float64).reshape(-1).copy(),
                               "kps_std_kf": np.asarray(t["kps_std_kf"], np.float64).copy(),
                               "obj_scale_kf": np.asarray(t["obj_scale_kf"], np.float64).copy()} for t in theirs])
    return res


def main(lib_path, jobs_path, out_path):
    L = ctypes.CDLL(lib_path)
    with open(jobs_path, "rb") as f:
        jobs = pickle.load(f)
    out = [solve(L, j) if j["kind"] == "solve" else video(L, j) for j in jobs]
    with open(out_path, "wb") as f:
        pickle.dump(out, f)


if __name__ == "__main__":
    main(*sys.argv[1:4])
