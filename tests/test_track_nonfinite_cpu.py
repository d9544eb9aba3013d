"""The tracking chain on non-finite detections, on the CPU: the host build of centerpose_amd/csrc/track_common.h (the text
track_associate_kernel runs on one lane) and of post_common.h, against oracle/munkres.py, scipy and the reference-shaped
Python mirrors, on the inputs of tests/track_poison_cases.py.

The contract ("Non-finite detections"): a cost that is not a number below 1e18 is a forbidden pair; the
assignment solvers terminate on any matrix.  Before it was written down, one NaN box centre made trk_munkres spin for ever
and trk_lsap drop every match of the frame.  Whatever could spin runs in a child process (tests/track_poison_driver.py)
under a time limit that is a guard, not a measurement: 60 s against an expected few milliseconds per call.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from centerpose_amd import hip
from oracle.tools import make_goldens as mg
from tests import track_poison_cases as pc
from tests.test_track_logic_cpu import TR, host  # noqa: F401  (the fixture that builds tests/native/track_host.cpp)

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHILD_LIMIT = 60  # seconds, per child process


def run_child(host_lib, jobs, tmp):
    """`jobs` through tests/track_poison_driver.py in a child process; a child that spins fails here at CHILD_LIMIT."""
    jp, rp = os.path.join(tmp, "jobs.pkl"), os.path.join(tmp, "results.pkl")
    with open(jp, "wb") as f:
        pickle.dump(jobs, f)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "track_poison_driver.py"), host_lib._name, jp, rp],
                       capture_output=True, text=True, timeout=CHILD_LIMIT, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(rp, "rb") as f:
        out = pickle.load(f)
    assert len(out) == len(jobs)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a. the solvers on hostile matrices
ENTRIES = ("munkres", "lsap", "api1", "api2")


@pytest.fixture(scope="module")
def solved(host, tmp_path_factory):  # noqa: F811
    """{(case name, entry, "raw" | "san"): result} -- every matrix as it is and in its sanitised form."""
    jobs, keys = [], []
    for name, c in pc.solver_cases():
        for entry in ENTRIES:
            if entry.startswith("api") and pc.is_harness_only(name):
                continue
            forms = [("raw", c)]
            if pc.comparable(c) and not np.array_equal(pc.sanitise(c), c):
                forms.append(("san", pc.sanitise(c)))
            for form, m in forms:
                jobs.append({"kind": "solve", "entry": entry, "matrix": m})
                keys.append((name, entry, form))
    res = run_child(host, jobs, str(tmp_path_factory.mktemp("solve")))
    return dict(zip(keys, res))


def _is_matching(match, nd, nt):
    m = np.asarray(match)
    used = m[m >= 0]
    return len(m) == nd and bool(((m >= -1) & (m < nt)).all()) and len(set(used.tolist())) == len(used)


def test_solvers_return_a_matching_on_every_hostile_matrix(solved):
    """Every call came back (the child met its time limit) and what it left is a matching: distinct columns, all in range,
    -1 otherwise -- NaN, +inf, -inf, 1e18 in one row, one column, column 0, one entry or everywhere, and finite +-1e308
    whose reductions overflow.  (-7 is the driver's fill value: a row the solver never wrote.)"""
    n = 0
    for name, c in pc.solver_cases():
        for entry in ("munkres", "lsap"):
            got = solved[(name, entry, "raw")]["match"]
            assert _is_matching(got, *c.shape), (name, entry, got.tolist())
            n += 1
    assert n == 2 * (len(pc.SOLVER_SHAPES) * (len(pc.SOLVER_PATTERNS) * len(pc.SOLVER_VALUES) + 2) + 2)


def test_solvers_equal_their_oracles_on_the_sanitised_matrices(solved):
    """Where the sanitised matrix is finite with |c| <= 1e18 the answer is defined: trk_munkres returns the pairs of
    oracle/munkres.py, trk_lsap those of scipy.optimize.linear_sum_assignment, through the harness and through
    cp_linear_assignment, and the two optimum values agree."""
    from scipy.optimize import linear_sum_assignment

    from oracle.munkres import linear_assignment as munkres_ref

    n = 0
    for name, c in pc.solver_cases():
        if not pc.comparable(c):
            continue
        s = pc.sanitise(c)
        form = "raw" if np.array_equal(s, c) else "san"
        nd, nt = s.shape
        want1 = -np.ones(nd, np.int32)
        ref = munkres_ref(s)
        want1[ref[:, 0]] = ref[:, 1]
        r, col = linear_sum_assignment(s)
        want2 = -np.ones(nd, np.int32)
        want2[r] = col
        for entry, want in (("munkres", want1), ("api1", want1), ("lsap", want2), ("api2", want2)):
            if (name, entry, form) not in solved:
                continue
            res = solved[(name, entry, form)]
            assert "match" in res, (name, entry, res)
            assert np.array_equal(res["match"], want), (name, entry, res["match"].tolist(), want.tolist())
        v1 = sum(s[i, j] for i, j in enumerate(want1) if j >= 0)
        v2 = sum(s[i, j] for i, j in enumerate(want2) if j >= 0)
        assert len(ref) == min(nd, nt) and np.isclose(v1, v2, rtol=1e-12, atol=1e-9), (name, v1, v2)
        n += 1
    # nan / inf / 1e18 in five patterns on five shapes, and the two 100 x 128 worst cases (which thus met no cap)
    # (and a +-1e308 matrix where all of it sanitises into range: the 1 x 1 one, if its entry is +1e308)
    n_huge = sum(pc.comparable(c) for name, c in pc.solver_cases() if "-huge" in name)
    assert n == len(pc.SOLVER_SHAPES) * len(pc.SOLVER_PATTERNS) * 3 + 2 + n_huge


def test_linear_assignment_refuses_non_finite_input_and_names_the_entry(solved):
    """cp_linear_assignment: CP_ERR_INVALID with the first offending row and column, before any work; a finite +-1e308
    matrix either solves or is refused (overflow met a loop bound / the infeasible exit) -- and came back."""
    n_bad = n_huge = 0
    for name, c in pc.solver_cases():
        if pc.is_harness_only(name):
            continue
        for entry in ("api1", "api2"):
            res = solved[(name, entry, "raw")]
            if np.isfinite(c).all():
                if "-huge" in name:
                    assert "error" in res or _is_matching(res["match"], *c.shape), (name, entry, res)
                    n_huge += 1
                else:
                    assert "match" in res, (name, entry, res)
                continue
            i, j = [int(v[0]) for v in np.nonzero(~np.isfinite(c))]   # the first one in row-major order
            assert "error" in res and "row %d, column %d" % (i, j) in res["error"], (name, entry, res)
            n_bad += 1
    assert n_bad == 2 * len(pc.SOLVER_SHAPES) * len(pc.SOLVER_PATTERNS) * 2 and n_huge == 4 * len(pc.SOLVER_SHAPES)
    # the matrix built to overflow in the adjustment step: Munkres stops at its bound and says so, with a partial matching
    # (5 x 4 is solved transposed, where the same matrix reduces to zeros and has an answer)
    for name in ("4x5-hugecols", "12x12-hugecols"):
        assert "iteration bound" in solved[(name, "api1", "raw")].get("error", ""), solved[(name, "api1", "raw")]
        assert (solved[(name, "munkres", "raw")]["match"] >= 0).sum() == 1, name


# ---------------------------------------------------------------------------------------------------------------------
# b. whole frames on poisoned videos
def _frames(mode):
    return mg.tracker_mode(mode)[0]


# with a PnP (the driver's stand-in) render_hmhp_mode 2 draws the filtered vertices, gated by the fused std, with k from the
# filter covariance: the render then reads everything the payload poison reaches
RENDER_VIA_FILTER = {"use_pnp": 1}


@pytest.fixture(scope="module")
def videos(host, tmp_path_factory):  # noqa: F811
    """{(mode, case): result of the driver}; case "clean", the association poison, the payload poison (twice: the
    goldens' parameters and the render that reads the filter), the score poison."""
    jobs, keys = [], []

    def add(mode, case, frames, python, params=None):
        jobs.append({"kind": "video", "mode": mode, "frames": frames, "python": python, "params": params,
                     "echo_pnp": params is not None})
        keys.append((mode, case))

    for mode in pc.VIDEO_MODES:
        fr = _frames(mode)
        add(mode, "clean", fr, True)
        add(mode, "clean/filter", fr, False, RENDER_VIA_FILTER)
        for name, fkeys, value, position in pc.assoc_cases():
            add(mode, "assoc/" + name, pc.assoc_video(fr, fkeys, value, position)[0], True)
        for key, vname, value in pc.PAYLOAD_CASES:
            bad = pc.poisoned(fr, [pc.PAYLOAD_AT], (key,), value)
            add(mode, "payload/%s-%s" % (key, vname), bad, False)
            add(mode, "payload/%s-%s/filter" % (key, vname), bad, False, RENDER_VIA_FILTER)
        add(mode, "score/nan-new", pc.score_video(fr, 0, 0, pc.NAN), True)
        add(mode, "score/inf-new", pc.score_video(fr, 0, len(fr[0]) - 1, pc.INF), True)
        add(mode, "score/nan-matched", pc.score_video(fr, 2, 0, pc.NAN), True)
        add(mode, "score/inf-matched", pc.score_video(fr, 2, 0, pc.INF), True)
    res = run_child(host, jobs, str(tmp_path_factory.mktemp("video")))
    return dict(zip(keys, res))


def _ids(tracks):
    return [int(t[TR["ID"]]) for t in tracks]


def _assert_ids_unique_and_increasing(res, what):
    seen = set()
    for f, tracks in enumerate(res["tracks"]):
        ids = _ids(tracks)
        assert len(set(ids)) == len(ids), (what, f, ids)
        new = sorted(set(ids) - seen)
        assert not seen or not new or new[0] > max(seen), (what, f, ids)   # a new id is above every id handed out before
        assert all(int(t[TR["AGE"]]) == 1 and int(t[TR["ACTIVE"]]) == 1 for t in tracks if int(t[TR["ID"]]) in new)
        seen |= set(ids)


def _assert_same_as_python(res, what):
    """Record for record against lib/utils/tracker.py on the same dicts, with the tolerances of
    test_tracker_logic_random_scenarios_vs_python_tracker (NaN / inf compare equal to themselves)."""
    assert len(res["py"]) == len(res["tracks"])
    for f, (mine, theirs) in enumerate(zip(res["tracks"], res["py"])):
        assert len(mine) == len(theirs), (what, f, _ids(mine), [g["tracking_id"] for g in theirs])
        for t, g in zip(mine, theirs):
            assert (int(t[0]), int(t[1]), int(t[2])) == (g["tracking_id"], g["age"], g["active"]), (what, f)
            np.testing.assert_allclose(t[4 + 28:4 + 30], g["ct"], rtol=1e-12, err_msg=str((what, f)))
            np.testing.assert_allclose(t[TR["MEAN_KF"]:TR["MEAN_KF"] + 16], g["kps_mean_kf"], rtol=1e-8, atol=1e-8)
            np.testing.assert_allclose(t[TR["STD_KF"]:TR["STD_KF"] + 16], g["kps_std_kf"], rtol=1e-8, atol=1e-8)
            np.testing.assert_allclose(t[TR["SCALE_KF"]:TR["SCALE_KF"] + 3], g["obj_scale_kf"], rtol=1e-6)


@pytest.mark.parametrize("mode", pc.VIDEO_MODES)
def test_association_poison_matches_the_python_tracker(videos, mode):
    """NaN / +inf in bbox + ct or in `tracking`, at detection 0 of frame 2, at the last detection of frame 1 and at every
    detection of frame 2: the host build and lib/utils/tracker.py agree record for record, clean video included."""
    _assert_same_as_python(videos[(mode, "clean")], (mode, "clean"))
    for name, _, _, _ in pc.assoc_cases():
        _assert_same_as_python(videos[(mode, "assoc/" + name)], (mode, name))


@pytest.mark.parametrize("mode", pc.VIDEO_MODES)
def test_association_poison_invariants(videos, mode):
    """Stated on their own, whatever the mirror does: ids unique and increasing; the poisoned track is retired and with it
    the last non-finite number, max_age frames after the poison; no clean detection loses its match, unless the track it
    continued in the clean run was last fed by the poisoned detection."""
    frames = _frames(mode)
    max_age = mg.TrackOpt.max_age
    clean = videos[(mode, "clean")]
    assert all(np.isfinite(t).all() for t in clean["tracks"])
    _assert_ids_unique_and_increasing(clean, (mode, "clean"))
    score = TR["POST"]   # field 0 of the post record: unique per detection of these videos, untouched by this poison

    def partners(res):
        """per frame: {score of a matched detection: score in the record its track held in the frame before}"""
        out = [{}]
        for f in range(1, len(res["tracks"])):
            before = {int(t[TR["ID"]]): float(t[score]) for t in res["tracks"][f - 1]}
            out.append({float(t[score]): before[int(t[TR["ID"]])] for t in res["tracks"][f]
                        if int(t[TR["ACTIVE"]]) >= 1 and int(t[TR["ID"]]) in before})
        return out

    want = partners(clean)
    assert sum(len(w) for w in want) >= 10
    for name, fkeys, value, position in pc.assoc_cases():
        res = videos[(mode, "assoc/" + name)]
        what = (mode, name)
        _assert_ids_unique_and_increasing(res, what)
        where = pc.assoc_video(frames, fkeys, value, position)[1]
        bad_scores = {float(frames[f][i]["score"]) for f, i in where}
        for f, tracks in enumerate(res["tracks"]):
            if f >= where[0][0] + max_age:
                assert np.isfinite(tracks).all(), (what, f)
        got = partners(res)
        for f, pairs in enumerate(want):
            for s, ps in pairs.items():
                if s not in bad_scores and ps not in bad_scores:
                    assert got[f].get(s) == ps, (what, f, s, got[f].get(s), ps)


@pytest.mark.parametrize("mode", [m for m in pc.VIDEO_MODES if not m.startswith("ties_")])
@pytest.mark.parametrize("value", sorted(pc.ASSOC_VALUES))
def test_poisoned_detection_starts_a_track_that_coasts_and_is_retired(videos, mode, value):
    """Detection 0 of frame 2 with NaN / +inf in bbox + ct (post 24..29), on the video of make_goldens.tracker_frames(): it
    matches nothing, starts track 5, which coasts in frame 3 and is gone in frame 4 -- the same ids behind every
    association mode (the ties video is another video: its ids are pinned by the comparison with the mirror)."""
    res = videos[(mode, "assoc/boxct-%s-f2d0" % value)]
    assert [_ids(t) for t in res["tracks"][2:5]] == pc.F2D0_IDS


@pytest.mark.parametrize("mode", pc.VIDEO_MODES)
def test_payload_poison_stays_in_its_own_track(videos, mode):
    """kps_fusion_mean / kps_fusion_std / obj_scale / obj_scale_uncertainty of one detection set to NaN, +-inf, 0 or a
    negative number, centre and box finite: the association does not notice (the ids, ages and activity of the clean run),
    every other track is bit-identical to the clean run, and nothing non-finite is drawn.  What the poisoned track's own
    filter holds is not specified."""
    pf, pi = pc.PAYLOAD_AT
    own_score = float(_frames(mode)[pf][pi]["score"])
    for suffix in ("", "/filter"):
        clean = videos[(mode, "clean" + suffix)]
        assert sum(int((r[:, 1:, 0] >= 0).sum()) for r in clean["recs"]) >= 40, (mode, suffix)   # vertices are being drawn
        for key, vname, _ in pc.PAYLOAD_CASES:
            what = (mode, key, vname, suffix)
            res = videos[(mode, "payload/%s-%s%s" % (key, vname, suffix))]
            own_id = [int(t[TR["ID"]]) for t in clean["tracks"][pf] if float(t[TR["POST"]]) == own_score]
            assert len(own_id) == 1, what
            if "baseline" in mode and key.startswith("kps_fusion"):
                # Tracker_baseline advances a track's centre by its filtered velocity (tracker_baseline.py:134-140), so there
                # the fused keypoints DO reach the association, through the filter: this is association poison.  The track
                # loses its detection, which may start a track or, in the greedy walk, take a neighbour's -- as after any
                # lost track -- so only the invariants are left to state.
                _assert_ids_unique_and_increasing(res, what)
                for f, a in enumerate(res["tracks"]):
                    assert len(a) >= len(clean["tracks"][f]) - 1, (what, f)
                    _assert_records_drawable(res["recs"][f], what, f)
                continue
            for f, (a, b) in enumerate(zip(res["tracks"], clean["tracks"])):
                assert [tuple(int(v) for v in t[:3]) for t in a] == [tuple(int(v) for v in t[:3]) for t in b], (what, f)
                for t, u, r, q in zip(a, b, res["recs"][f], clean["recs"][f]):
                    if int(u[TR["ID"]]) != own_id[0]:
                        assert t.tobytes() == u.tobytes() and r.tobytes() == q.tobytes(), (what, f, int(u[TR["ID"]]))
                _assert_records_drawable(res["recs"][f], what, f)


def _assert_records_drawable(recs, what, f, inp_w=512, inp_h=512):
    """trk_render_records' promise: channel -1, or a finite record inside the input."""
    for r in np.asarray(recs).reshape(-1, 5):
        if r[0] == -1:
            continue
        assert np.isfinite(r).all(), (what, f, r)
        assert r[0] >= 0 and 0 <= r[1] < inp_w and 0 <= r[2] < inp_h and 0 <= r[3] <= max(inp_w, inp_h), (what, f, r)


@pytest.mark.parametrize("mode", pc.VIDEO_MODES)
def test_score_poison(videos, mode):
    """`score > new_thresh` and `score >= pre_thresh` with a score that is not a number: NaN never starts a track, +inf
    does; a matched detection keeps its track whatever its score, and a record with a NaN score (or an infinite k) draws
    nothing."""
    frames = _frames(mode)
    clean = videos[(mode, "clean")]
    for case in ("nan-new", "inf-new", "nan-matched", "inf-matched"):
        res = videos[(mode, "score/" + case)]
        _assert_same_as_python(res, (mode, case))
        _assert_ids_unique_and_increasing(res, (mode, case))
        for f, recs in enumerate(res["recs"]):
            _assert_records_drawable(recs, (mode, case), f)
    # frame 0: every detection above new_thresh starts a track, in detection order
    strong = [d["score"] > mg.TrackOpt.new_thresh for d in frames[0]]
    assert len(clean["tracks"][0]) == sum(strong)
    assert strong[0] and len(videos[(mode, "score/nan-new")]["tracks"][0]) == sum(strong) - 1
    assert not np.isnan(videos[(mode, "score/nan-new")]["tracks"][0][:, TR["POST"]]).any()
    inf0 = videos[(mode, "score/inf-new")]["tracks"][0]
    assert len(inf0) == sum(strong[:-1]) + 1 and np.isinf(inf0[-1, TR["POST"]])
    for case, test in (("nan-matched", np.isnan), ("inf-matched", np.isinf)):
        res = videos[(mode, "score/" + case)]
        for f, (a, b) in enumerate(zip(res["tracks"], clean["tracks"])):
            assert [tuple(int(v) for v in t[:3]) for t in a] == [tuple(int(v) for v in t[:3]) for t in b], (mode, case, f)
        hit = [i for i, t in enumerate(res["tracks"][2]) if test(t[TR["POST"]])]
        assert len(hit) == 1 and int(res["tracks"][2][hit[0], TR["ACTIVE"]]) >= 1
        rec = res["recs"][2][hit[0]]
        if case == "nan-matched":
            assert (rec[:, 0] == -1).all()                  # NaN >= pre_thresh is false: nothing of this track is drawn
        else:
            assert rec[0, 0] == -1 and (rec[1:, 0] >= 0).any()   # the centre blob's k would be +inf; the vertices have k = 1


# ---------------------------------------------------------------------------------------------------------------------
# c. post-process: scores and boxes that are not numbers
from tests.test_post_logic_cpu import _run as _post_run  # noqa: E402
from tests.test_post_logic_cpu import host as post_host  # noqa: E402,F401


def _post_meta(m):
    from centerpose_amd.lib.utils.image import get_affine_transform

    meta = np.zeros(8)
    meta[:6] = get_affine_transform(m["c"], m["s"], 0, (m["out_width"], m["out_height"]), inv=1).reshape(-1)
    meta[6] = m["s"] / max(m["out_width"], m["out_height"])
    return meta


def _mirror(d, meta, nms):
    from centerpose_amd.lib.detectors.object_pose import ObjectPoseDetector

    opt = mg.HostOpt()
    opt.nms = nms
    fake = type("S", (), {"opt": opt})()
    with np.errstate(all="ignore"):
        return ObjectPoseDetector.merge_outputs(fake, [ObjectPoseDetector.post_process(fake, d, meta, 1)])


@pytest.mark.parametrize("nms", [True, False])
@pytest.mark.parametrize("case", sorted(pc.POST_CASES))
def test_post_process_on_non_finite_scores_and_boxes(post_host, case, nms):  # noqa: F811
    """K = 8 overlapping records with NaN / +-inf scores and NaN / inf boxes through the host build of post_common.h and
    through ObjectPoseDetector.post_process + merge_outputs (soft_nms_nvidia): the same survivors in the same order, and
    the rule both follow -- a NaN score never passes the threshold; a non-finite box neither suppresses another record nor
    is suppressed, so the records with finite boxes fare exactly as if the others had not been there.
    (Before the rule was stated both sides broke it, differently: fmin / fmax drop a NaN corner, Python's min / max keep
    whichever operand comes first, and the decayed score of the victim became NaN, which no threshold removes.)"""
    dets, metas = mg.host_cases()
    meta = _post_meta(metas[0])
    thr = mg.HostOpt.vis_thresh
    d, raw = pc.post_inputs(dets, 0, case)
    rec = _post_run(post_host, raw, meta, thr, nms)
    ref = _mirror(d, metas[0], nms)
    off = {k: o for k, (o, w) in hip.POST_FIELDS.items()}
    assert len(rec) == len(ref), (len(rec), len(ref))
    for r, t in zip(rec, ref):
        np.testing.assert_allclose(r[0], t["score"], rtol=1e-12)
        np.testing.assert_allclose(r[off["bbox"]:off["bbox"] + 4], np.asarray(t["bbox"], np.float64), rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(r[off["kps"]:off["kps"] + 16], np.asarray(t["kps"], np.float64).reshape(-1), rtol=1e-9,
                                   atol=1e-9)
    # the rule, stated on its own
    assert not np.isnan(rec[:, 0]).any()
    # each record alone, no threshold: its transformed box and the score it came with (a NaN score yields no record)
    alone = [_post_run(post_host, raw[k:k + 1], meta, -np.inf, False) for k in range(pc.POST_K)]
    odd = [k for k in range(pc.POST_K) if raw[k, 4] > thr and not np.isfinite(alone[k][0, 24:28]).all()]
    box_ok = np.isfinite(rec[:, 24:28]).all(1)
    # a record with a non-finite box that passes the threshold survives with the score it came with ...
    assert sorted(rec[~box_ok, 0].tolist()) == sorted(float(alone[k][0, 0]) for k in odd)
    # ... and the others fare as if it had not been there
    rest = [k for k in range(pc.POST_K) if k not in odd]
    assert rec[box_ok].tobytes() == _post_run(post_host, raw[rest], meta, thr, nms).tobytes()
    if case in ("box-nan", "box-inf", "corner-nan", "corner-inf", "mixed"):
        assert odd
