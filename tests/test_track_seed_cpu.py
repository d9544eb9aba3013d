"""Seeding the tracker from annotations and the ground-truth previous-frame maps, without a GPU:

* the detector mirror's ``run()`` against tests/golden/track_run_seeded.json -- the REFERENCE's own ``run()`` on the stub
  video with ``meta['pre_dets']`` on the frames its evaluator gives them (tools/make_track_seed_goldens.py), in the three flag
  sets of the reference's tracking benchmark;
* the seeding functions of centerpose_amd/csrc/track_common.h (what track.hip's track_seed_kernel runs), compiled for the
  host by tests/native/track_seed_host.cpp, against the mirror's ``Tracker.init_track`` / ``Tracker_baseline.init_track`` and
  ``_track_records`` in its ground-truth mode;
* ``hip.pack_seeds``.
"""
import contextlib
import copy
import ctypes
import io
import json
import os
import subprocess

import numpy as np
import pytest

from centerpose_amd import hip
from centerpose_amd.lib.opts import opts
from centerpose_amd.lib.utils.image import get_affine_transform
from oracle.tools import make_goldens as mg
from oracle.tools import track_golden as tg
from tests import test_tracking_loop as ttl
from tests import track_seed_cases as sc

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(REPO, "tests", "golden", "track_run_seeded.json")
STRIDE, SEED = hip.TRACK_STRIDE, hip.SEED_STRIDE
TR = dict(ID=0, AGE=1, ACTIVE=2, FLAGS=3, POST=4, KF_X=242, KF_P=274, POOL_PREC=402, POOL_ACC=405, POOL_N=408, MEAN_KF=409,
          STD_KF=425, SCALE_KF=441)
Params = hip.TrackParams


def seeded_opt(gpus, extra, baseline=False):
    argv = [a if a != "-1" else gpus for a in (tg.BASELINE_ARGV if baseline else tg.TRACK_ARGV)] + list(extra)
    with contextlib.redirect_stdout(io.StringIO()):
        o = opts().parser.parse_args(argv)
        o = tg.demo_flags(o)
        o = opts().init(opts().parse(o))
    return o


def seeded_detector(monkeypatch, gpus, extra, baseline=False):
    """ttl._detector with extra flags on the command line."""
    from centerpose_amd.lib.detectors import base_detector as bd
    from centerpose_amd.lib.detectors.object_pose import ObjectPoseDetector

    stub = tg.StubNetwork(tg.video_heads())
    monkeypatch.setattr(bd, "create_model", lambda *a, **k: stub)
    monkeypatch.setattr(bd, "load_model", lambda m, *a, **k: m)
    with contextlib.redirect_stdout(io.StringIO()):
        det = ObjectPoseDetector(seeded_opt(gpus, extra, baseline))
    stub._engine = lambda: ttl._Engine(stub, det.opt.device)
    return det


def gold(mode):
    with open(GOLD) as fh:
        return json.load(fh)[mode]["frames"]


@pytest.mark.parametrize("mode", sorted(sc.MODES))
def test_mirror_run_matches_seeded_reference_golden(monkeypatch, mode):
    """The mirror's run() on the seeded video == the reference's, frame by frame: which seeds become tracks and with which
    ids, the ground-truth maps the network is fed (their sums and their extent, blobs centred outside the input included),
    the seeded tracks being continued by the video's detections, coasting, ageing and being retired."""
    from centerpose_amd.lib.detectors import base_detector as bd
    from centerpose_amd.lib.utils.pnp import cuboid_pnp_solver as cps

    g = gold(mode)
    det = seeded_detector(monkeypatch, "-1", sc.MODES[mode])
    det.process = ttl._cpu_process(det)
    monkeypatch.setattr(cps, "solve_pnp_batch", ttl._oracle_pnp_rows)
    monkeypatch.setattr(bd, "solve_pnp_batch", ttl._oracle_pnp_rows)
    with contextlib.redirect_stdout(io.StringIO()):
        frames = sc.run_video(det, get_affine_transform, mode)
    ttl._compare(frames, g)
    # the golden itself is not degenerate: five seeds accepted, two continued, three coast and are retired together
    assert [t["tracking_id"] for t in g[0]["tracks"]] == [1, 2, 3, 4, 5]
    assert [(t["age"], t["active"]) for t in g[0]["tracks"]][:3] == [(1, 2), (1, 2), (2, 0)]
    if mode == "gt_first_empty":
        assert all(f["pre_hm_sum"] == 0 and f["pre_hm_hp_nonzero"] == 0 for f in g)
    else:
        assert g[0]["pre_hm_hp_nonzero"] > 10 * gold("gt_first")[1]["pre_hm_hp_nonzero"] > 0
    if mode != "gt_every":
        assert len(g[-1]["tracks"]) == 2


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    out = os.path.join(REPO, "tests", "_build", "libcp_track_seed_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off",
                    os.path.join(REPO, "tests", "native", "track_seed_host.cpp"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    assert L.cp_seed_host_stride() == SEED and L.cp_seed_host_track_stride() == STRIDE
    assert L.cp_seed_host_params_bytes() == ctypes.sizeof(Params)
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _vm(meta):
    v = np.zeros(16)
    v[0:6] = np.asarray(meta["trans_input"], np.float64).reshape(-1)
    v[6:10] = [meta["width"], meta["height"], meta["inp_width"], meta["inp_height"]]
    return v


def _identity_vm():
    vm = np.zeros(16)
    vm[[0, 4]] = 1.0
    vm[6:10] = 512
    return vm


def host_seed(L, P, vm, seeds, gt=0, hm_plane=0, hp_plane0=1):
    """-> (tracks [n, STRIDE], recs [cap, 9, 5], id_count, dropped)"""
    seeds = np.ascontiguousarray(seeds, np.float64).reshape(-1, SEED)
    tracks = np.zeros((P.cap, STRIDE))
    recs = np.zeros((P.cap, 9, 5))
    idc, dropped = ctypes.c_int(-7), ctypes.c_int(-7)
    n = L.cp_seed_host_seed(ctypes.byref(P), _ptr(np.ascontiguousarray(vm, np.float64)), _ptr(seeds), len(seeds), int(gt),
                            hm_plane, hp_plane0, _ptr(tracks), _ptr(recs), ctypes.byref(idc), ctypes.byref(dropped))
    return tracks[:n], recs, idc.value, dropped.value


def _params(o, cap=hip.TRACK_CAP, baseline=False, **kw):
    d = dict(new_thresh=o.new_thresh, pre_thresh=0.3, R=o.R, conf_lo=3, conf_hi=9, max_age=o.max_age, kalman=int(o.kalman),
             scale_pool=int(o.scale_pool), use_pnp=0, hps_uncertainty=1, show_axes=0, cat_rule=0, render_hm_mode=1,
             render_hmhp_mode=2, pre_hm=1, pre_hm_hp=1, K=100, cap=cap, hungarian=0, baseline=int(baseline))
    d.update(kw)
    return Params(**d)


def _post_from_dict(d):
    r = np.zeros(120)
    for k, (off, w) in hip.POST_FIELDS.items():
        if k in d:
            r[off:off + w] = np.asarray(d[k], np.float64).reshape(-1)
    r[64:80] = np.asarray(d["kps_fusion_mean"], np.float64)   # only the fused estimate is given: heat-map side "missing"
    r[8:24] = np.asarray(d["kps_fusion_std"], np.float64)
    r[80:96] = -1.0
    return r


def _check_seeded(tracks, py_tracks, o, baseline):
    assert len(tracks) == len(py_tracks)
    for t, g in zip(tracks, py_tracks):
        assert (int(t[0]), int(t[1]), int(t[2])) == (g["tracking_id"], g["age"], g["active"])
        np.testing.assert_allclose(t[4 + 28:4 + 30], g["ct"], rtol=1e-12)
        if o.kalman:
            np.testing.assert_allclose(t[TR["KF_X"]:TR["KF_X"] + 32], np.asarray(g["kf"].x).reshape(-1), rtol=1e-8, atol=1e-8)
            P32 = np.asarray(g["kf"].P, np.float64)
            blocks = np.stack([P32[4 * v:4 * v + 4, 4 * v:4 * v + 4] for v in range(8)])
            off = P32.copy()
            for v in range(8):
                off[4 * v:4 * v + 4, 4 * v:4 * v + 4] = 0
            assert not off.any()
            np.testing.assert_allclose(t[TR["KF_P"]:TR["KF_P"] + 128].reshape(8, 4, 4), blocks, rtol=1e-8, atol=1e-8)
        if o.scale_pool:
            assert len(g["scale_pool"]) == 1 and t[TR["POOL_N"]] == 1
            mean, unc = (np.asarray(x, np.float64) for x in g["scale_pool"][0])
            w = np.ones(3) if baseline else unc ** -2.0
            np.testing.assert_allclose(t[TR["POOL_PREC"]:TR["POOL_PREC"] + 3], w, rtol=1e-6)
            np.testing.assert_allclose(t[TR["POOL_ACC"]:TR["POOL_ACC"] + 3], w * mean, rtol=1e-6)


@pytest.mark.parametrize("baseline", [False, True])
@pytest.mark.parametrize("kalman,scale_pool", [(True, True), (True, False), (False, True), (False, False)])
def test_host_seeding_matches_python_tracker(host, baseline, kalman, scale_pool):
    """trk_seed_walk / trk_seed_track against ``init_track`` of the mirror's Tracker and Tracker_baseline: which seeds become
    tracks (score > new_thresh, in order), ids, age, active, the centre (given, or the box centre), ``init_kf`` of the class
    and the one-sample pool.  Then three frames of detections through the frame stages against the mirror's ``step``: seeded
    tracks are continued, coast and are retired like any other."""
    from centerpose_amd.lib.utils.tracker import Tracker, Tracker_baseline

    class Opt(mg.TrackOpt):
        pass

    o = Opt(False)
    o.kalman, o.scale_pool, o.max_age = kalman, scale_pool, 2
    P = _params(o, baseline=baseline)
    vm = _identity_vm()
    given = sc.annotations(0)
    before = copy.deepcopy(given)
    seeds, counts = hip.pack_seeds([given], P)
    assert counts.tolist() == [len(given)]
    for a, b in zip(given, before):   # pack_seeds only reads
        assert set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)
    tracks, _, idc, dropped = host_seed(host, P, vm, seeds[0])
    py = (Tracker_baseline if baseline else Tracker)(o)
    py.tracks, py.id_count = ["stale"], 41   # 'pre_dets' resets the list and the id counter
    py.init_track({"id": 0, "pre_dets": given})
    assert (idc, dropped) == (py.id_count, 0) and len(py.tracks) == 5
    assert "ct" not in before[1] and "ct" in py.tracks[1]
    _check_seeded(tracks, py.tracks, o, baseline)
    if not (kalman or scale_pool) or (baseline and not kalman):
        # no read-out without a filter or a pool (the device tracker refuses that configuration), and Tracker_baseline's
        # association reads the filter's velocity: without --kalman its step() raises
        return
    # ---- three frames: objects A and B move on, a third object appears, a weak detection never becomes a track ----
    rng = np.random.RandomState(3)
    cap = P.cap
    prev = np.zeros((cap, STRIDE))
    prev[:len(tracks)] = tracks
    n_prev, id_count = len(tracks), ctypes.c_int(idc)
    host.cp_seed_host_update.restype = ctypes.c_int
    base = [np.asarray(py.tracks[0]["ct"], float), np.asarray(py.tracks[1]["ct"], float), np.array([250.0, 90.0]),
            np.array([440.0, 90.0])]
    for f in range(1, 4):
        dets = []
        for i, c0 in enumerate(base):
            vel = np.array([3.0, -2.0]) * (1 + i)
            ct = c0 + vel * f + rng.randn(2)
            kps = ct[None, :] + rng.uniform(-0.5, 0.5, (8, 2)) * 50
            dets.append({"score": 0.2 if i == 3 else float(rng.uniform(0.5, 0.99)), "cls": 0,
                         "bbox": [ct[0] - 30, ct[1] - 30, ct[0] + 30, ct[1] + 30], "ct": [float(ct[0]), float(ct[1])],
                         "tracking": (-vel + rng.randn(2)).astype(np.float32),
                         "tracking_hp": (np.tile(-vel, 8) + rng.randn(16) * 0.5).astype(np.float32),
                         "kps": kps.reshape(-1).astype(np.float32), "kps_fusion_mean": kps.reshape(-1) + rng.randn(16) * 0.3,
                         "kps_fusion_std": rng.uniform(0.4, 6.0, 16), "obj_scale": rng.uniform(0.5, 1.5, 3).astype(np.float32),
                         "obj_scale_uncertainty": rng.uniform(0.05, 0.3, 3).astype(np.float32)})
        post = np.stack([_post_from_dict(d) for d in dets])
        nxt = np.zeros((cap, STRIDE))
        pts, scl = np.zeros((cap, 16), np.float32), np.zeros((cap, 3), np.float32)
        n = host.cp_seed_host_update(ctypes.byref(P), _ptr(vm), _ptr(post), len(post), _ptr(prev), n_prev,
                                     ctypes.byref(id_count), _ptr(nxt), _ptr(pts), _ptr(scl))
        theirs, _ = py.step(copy.deepcopy(dets))
        assert n == len(theirs), f
        for t, g in zip(nxt[:n], theirs):
            assert (int(t[0]), int(t[1]), int(t[2])) == (g["tracking_id"], g["age"], g["active"]), f
            np.testing.assert_allclose(t[4 + 28:4 + 30], g["ct"], rtol=1e-12)
            if kalman:
                np.testing.assert_allclose(t[TR["MEAN_KF"]:TR["MEAN_KF"] + 16], np.asarray(g["kps_mean_kf"]).reshape(-1),
                                           rtol=1e-8, atol=1e-8)
                np.testing.assert_allclose(t[TR["STD_KF"]:TR["STD_KF"] + 16], g["kps_std_kf"], rtol=1e-8, atol=1e-8)
            if scale_pool:
                np.testing.assert_allclose(t[TR["SCALE_KF"]:TR["SCALE_KF"] + 3], g["obj_scale_kf"], rtol=1e-6)
        prev, n_prev = nxt, n
        if f == 1:   # A and B continued (active 2), the other three seeds coast, the new object got the next id
            assert [(g["tracking_id"], g["active"]) for g in theirs] == [(1, 2), (2, 2), (6, 1), (3, 0), (4, 0), (5, 0)]
    assert sorted(g["tracking_id"] for g in theirs) == [1, 2, 6]   # the coasting seeds are gone (max_age 2)


def _gt_metas():
    """The video's meta (identity crop) and a 640 x 480 frame cropped off-centre into the 512 x 512 input."""
    m0 = dict(tg.frame_inputs(get_affine_transform)[0][1])
    c, s = np.array([300.0, 200.0], dtype=np.float32), 600.0
    m1 = dict(m0, c=c, s=s, width=640, height=480, trans_input=get_affine_transform(c, s, 0, [512, 512]),
              trans_output=get_affine_transform(c, s, 0, [128, 128]))
    return [m0, m1]


def mirror_gt_records(det, tracks, meta, with_hm=True, with_hm_hp=True):
    """``_track_records`` in its ground-truth mode as [n, 9, 5] rows (channel -1 = not drawn), planes 0 and 1..8."""
    out = np.zeros((len(tracks), 9, 5))
    out[:, :, 0] = -1
    for i, t in enumerate(tracks):
        hm, hp, _ = det._track_records([copy.deepcopy(t)], dict(meta, id=0), with_hm, with_hm_hp)
        for r in hm:
            out[i, 0] = r
        for r in hp:
            out[i, 1 + int(r[0])] = (1 + r[0],) + tuple(r[1:])
    return out


@pytest.mark.parametrize("pre_hm,pre_hm_hp", [(1, 1), (1, 0), (0, 1)])
def test_host_ground_truth_records_equal_mirror(host, monkeypatch, pre_hm, pre_hm_hp):
    """trk_render_records_gt against ``_track_records`` in 'gt' mode, record for record and exactly: no pre_thresh test,
    k = 1, the centre's radius on every vertex, vertices drawn wherever they land (the seed with a vertex on either side of
    the frame), nothing for the seed whose clipped box is degenerate; centre only with pre_hm, vertices only with pre_hm_hp."""
    det = seeded_detector(monkeypatch, "-1", sc.MODES["gt_every"])
    o = det.opt
    for m, meta in enumerate(_gt_metas()):
        given = sc.annotations(0)
        given[0]["score"] = 0.31   # above new_thresh: a track, and drawn although a non-gt frame would ...
        P = _params(mg.TrackOpt(False), pre_hm=pre_hm, pre_hm_hp=pre_hm_hp, pre_thresh=0.5)  # ... apply pre_thresh
        seeds, _ = hip.pack_seeds([given], P, [True])
        tracks, recs, _, _ = host_seed(host, P, _vm(meta), seeds[0], gt=1)
        det.tracker.init_track({"id": 0, "pre_dets": copy.deepcopy(given)})
        want = mirror_gt_records(det, det.tracker.tracks, meta, bool(pre_hm), bool(pre_hm_hp))
        assert len(tracks) == len(want) == 5
        assert np.array_equal(recs[:5], want), (recs[:5] - want)
        assert (recs[5:, :, 0] == -1).all()
        if m:
            continue   # (the wider second frame holds every seed)
        assert (want[4, :, 0] == -1).all()                                # the degenerate box
        if pre_hm_hp:
            xs = want[3, 1:, 1]
            assert (want[3, 1:, 0] > 0).all() and xs.min() < 0 and xs.max() >= meta["inp_width"]   # centred outside, both sides
    assert o.gt_pre_hm_hmhp


def test_host_ground_truth_records_withdraw_non_finite(host, monkeypatch):
    """A kps_gt coordinate that is not finite, or that does not fit the integer it is converted to, withdraws that vertex
    record and nothing else; a non-finite box draws nothing."""
    det = seeded_detector(monkeypatch, "-1", sc.MODES["gt_every"])
    meta = _gt_metas()[0]
    P = _params(mg.TrackOpt(False))
    clean = sc.annotations(0)[:2]
    det.tracker.init_track({"id": 0, "pre_dets": copy.deepcopy(clean)})
    want = mirror_gt_records(det, det.tracker.tracks, meta)
    bad = copy.deepcopy(clean)
    g = np.array(bad[0]["kps_gt"], np.float64)
    g[1, 0], g[2, 1], g[3, 0], g[4, 1], g[5, 0] = np.nan, np.inf, 1e30, -1e7, -np.inf
    bad[0]["kps_gt"] = g
    bad[1]["bbox"] = np.array([np.nan, 10.0, 200.0, 300.0])
    seeds, _ = hip.pack_seeds([bad], P, [True])
    tracks, recs, _, _ = host_seed(host, P, _vm(meta), seeds[0], gt=1)
    assert len(tracks) == 2
    for j in range(9):
        if 1 <= j <= 5:
            assert recs[0, j, 0] == -1, j
        else:
            assert np.array_equal(recs[0, j], want[0, j]), j
    assert (recs[1, :, 0] == -1).all()
    assert np.isfinite(recs[:2][recs[:2, :, 0] >= 0]).all()


def test_host_seeding_truncates_and_reports_overflow(host):
    """cap = 4 and six accepted seeds (a weak one and a NaN score in between): ids 1..4 in seed order, two dropped, no id
    spent on them."""
    P = _params(mg.TrackOpt(False), cap=4)
    a = sc.annotations(0)
    weak, nan = copy.deepcopy(a[3]), copy.deepcopy(a[2])
    nan["score"] = float("nan")
    strong = [copy.deepcopy(a[i % 3]) for i in range(6)]
    for i, s in enumerate(strong):
        s["score"] = 0.4 + 0.05 * i
    given = [strong[0], weak, strong[1], nan, strong[2], strong[3], strong[4], strong[5]]
    seeds, _ = hip.pack_seeds([given], P)
    tracks, recs, idc, dropped = host_seed(host, P, _identity_vm(), seeds[0])
    assert len(tracks) == 4 and (idc, dropped) == (4, 2)
    assert tracks[:, TR["ID"]].tolist() == [1, 2, 3, 4]
    np.testing.assert_allclose(tracks[:, TR["POST"]], [0.4, 0.45, 0.5, 0.55])


def test_pack_seeds_layout_counts_and_missing_keys():
    P = _params(mg.TrackOpt(False))
    a = sc.annotations(0)
    seeds, counts = hip.pack_seeds([None, a, []], P, [False, True, False])
    assert seeds.shape == (3, 6, SEED) and seeds.dtype == np.float64 and counts.tolist() == [-1, 6, 0]
    assert not seeds[0].any() and not seeds[2].any()
    for i, d in enumerate(a):
        for k, (off, w) in hip.SEED_FIELDS.items():
            want = np.asarray(d[k], np.float64).reshape(-1) if k in d else np.zeros(w)
            assert np.array_equal(seeds[1, i, off:off + w], want), (i, k)
        assert seeds[1, i, hip.SEED_PRESENT] == (15 if "ct" in d else 14)
    assert hip.pack_seeds([a[:2], None, None], P, S=8)[0].shape == (3, 8, SEED)
    for key, gt in (("kps_fusion_std", False), ("obj_scale", False), ("bbox", False), ("kps_gt", True)):
        b = [dict(d) for d in a]
        del b[2][key]
        with pytest.raises(KeyError, match=key):
            hip.pack_seeds([None, b, None], P, [False, gt, False])
    b = [dict(d) for d in a]
    del b[2]["kps_gt"]
    hip.pack_seeds([b], P, [False])   # not needed where the maps are not the ground-truth ones
    with pytest.raises(ValueError):
        hip.pack_seeds([a], P, S=3)


def test_cp_track_seed_refuses_bad_arguments_before_any_launch():
    """S in 1..CP_TRACK_CAP, B > 0, cap in range, non-null pointers: CP_ERR_INVALID, and no device is needed to be told so."""
    L = hip.lib()
    assert "cp_track_seed" in hip.exported_symbols()
    P = _params(mg.TrackOpt(False))
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused on its arguments
    ok = dict(params=ctypes.byref(P), vmeta=p, seeds=p, count=p, gt=None, B=3, S=6, state=p, recs=p)
    for change in (dict(S=0), dict(S=hip.TRACK_CAP + 1), dict(B=0), dict(vmeta=None), dict(seeds=None), dict(count=None),
                   dict(state=None), dict(recs=None), dict(params=None)):
        a = dict(ok, **change)
        rc = L.cp_track_seed(None, a["params"], a["vmeta"], a["seeds"], a["count"], a["gt"], a["B"], a["S"], a["state"], a["recs"])
        assert rc == -1, change
        assert b"cp_track_seed" in L.cp_last_error()
    bad_cap = _params(mg.TrackOpt(False), cap=hip.TRACK_CAP + 1)
    assert L.cp_track_seed(None, ctypes.byref(bad_cap), p, p, p, None, 3, 6, p, p) == -1
