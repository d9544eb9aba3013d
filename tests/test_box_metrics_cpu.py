"""The Objectron box metrics' numerics (centerpose_amd/csrc/box3d_common.h) compiled for the host by
tests/native/box3d_host.cpp and pinned to the REFERENCE evaluator's own output on seeded cases
(tests/golden/box_eval_ref.npz, tools/make_box_eval_goldens.py); BoxEvaluator's bookkeeping with that host build
injected, against the reference's HitMiss records and APs; the C ABI's exports and argument checks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from centerpose_amd import box_metrics, hip

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(REPO, "tests", "golden", "box_eval_ref.npz")
IOU_TOL = 1e-6  # divergence sum vs qhull, with the 1e-6 on-plane epsilon
REL_TOL = 1e-9
TIE = 1e-9
c_void_p = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(c_void_p)


@pytest.fixture(scope="module")
def host():
    out = os.path.join(REPO, "tests", "_build", "libcp_box3d_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(REPO, "tests", "native", "box3d_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
    lib = ctypes.CDLL(out)
    for f in (lib.box_host_iou, lib.box_host_eval, lib.box_host_fit, lib.box_host_rotate):
        f.restype = None
    lib.box_host_rotate.argtypes = [c_void_p, ctypes.c_double, c_void_p]
    lib.box_host_volume.restype = ctypes.c_double
    return lib


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


def host_iou(host, a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    iou, fl = np.zeros(len(a)), np.zeros(len(a), np.int32)
    host.box_host_iou(_p(a), _p(b), len(a), _p(iou), _p(fl))
    assert not fl.any()
    return iou


def host_eval(host, pred3d, gt3d, pred2d, mo2c, proj, single, num_symmetry):
    args = [np.ascontiguousarray(x, np.float64) for x in (pred3d, gt3d, pred2d, mo2c, proj)]
    single = np.ascontiguousarray(single, np.int32)
    out = np.zeros((len(args[0]), hip.BOX_EVAL_STRIDE))
    host.box_host_eval(*[_p(x) for x in args], _p(single), len(single), int(num_symmetry), _p(out))
    return out


def eval_golden(run, g):
    """every evaluate case of the golden through `run` (one call per num_symmetry) -> [P, 9]"""
    out = np.zeros((len(g["ev_nsym"]), hip.BOX_EVAL_STRIDE))
    for ns in np.unique(g["ev_nsym"]):
        m = np.where(g["ev_nsym"] == ns)[0]
        out[m] = run(g["ev_pred3d"][m], g["ev_gt3d"][m], g["ev_pred2d"][m], g["ev_mo2c"][m], g["ev_proj"][m],
                     g["ev_single"][m], int(ns))
    return out


def check_against_reference(out, g):
    """IoU to IOU_TOL; the reported rotation is the reference's, or one whose IoU ties the reference's best to < 1e-9
    (a cuboid turned by 180 degrees is the same cuboid with its vertices renamed: ADD and azimuth differ), and ADD,
    ADD-S, azimuth, polar are the reference's values at that rotation to 1e-9 relative; the 2D error and its index
    as the reference's."""
    ref = g["ev_ref"]
    close = lambda a, b: abs(a - b) <= REL_TOL * max(1.0, abs(b))  # noqa: E731
    for p in range(len(ref)):
        assert abs(out[p, 0] - ref[p, 0]) <= IOU_TOL, (p, out[p, 0], ref[p, 0])
        b3, rb3 = int(out[p, 6]), int(ref[p, 6])
        if rb3 < 0:
            assert b3 == -1 and out[p, 0] == 0 and out[p, 1] == 1.0 and out[p, 2] == 1.0, (p, out[p])
            assert close(out[p, 3], ref[p, 3]) and close(out[p, 4], ref[p, 4]), (p, out[p], ref[p])
        else:
            rots = g["ev_rot_iou"][p]
            if b3 != rb3:
                assert b3 >= 0 and abs(rots[b3] - rots[rb3]) < TIE, (p, b3, rb3, rots[b3], rots[rb3])
            for col, name in ((1, "add"), (2, "adds"), (3, "az"), (4, "pol")):
                want = g["ev_rot_" + name][p, b3]
                assert close(out[p, col], want), (p, name, out[p, col], want)
        assert close(out[p, 5], ref[p, 5]), (p, out[p, 5], ref[p, 5])
        assert int(out[p, 7]) == int(ref[p, 7]), p
        assert out[p, 8] == 0, p


def test_iou_against_reference(host, g):
    iou = host_iou(host, g["iou_a"], g["iou_b"])
    err = np.abs(iou - g["iou_ref"])
    assert err.max() <= IOU_TOL, (err.argmax(), err.max())
    generic = np.isin(g["iou_kind"], (0, 3, 4, 9))
    assert err[generic].max() < 1e-12  # away from the plane epsilon only rounding separates hull and divergence


def test_iou_degenerate_cases_exact(host, g):
    """disjoint (2), faces touching with opposite normals (5), edge (6) and vertex (7) contact: qhull has no volume to
    give and the reference returns 0 -- exactly 0 here too; identical boxes (1) give 1 to rounding (the reference's
    0.9999999999999988), a shared face plane (4) is counted once"""
    iou = host_iou(host, g["iou_a"], g["iou_b"])
    k = g["iou_kind"]
    for kind in (2, 5, 6, 7):
        assert np.all(g["iou_ref"][k == kind] == 0.0)
        assert np.all(iou[k == kind] == 0.0), (kind, iou[k == kind])
    assert np.all(np.abs(iou[k == 1] - 1.0) < 1e-12)
    assert np.all(np.abs(iou[k == 4] - g["iou_ref"][k == 4]) < 1e-12)
    # symmetric in its arguments up to rounding
    assert np.abs(host_iou(host, g["iou_b"], g["iou_a"]) - iou).max() < 1e-12


def test_fit_is_the_least_squares_solution(host, g):
    """Box.fit's lstsq of [scaled unit box | 1] against noisy vertices: the closed form is exact (diagonal normal
    matrix), not re-orthogonalised"""
    from tools.make_box_eval_goldens import aabb

    for v in np.concatenate([g["iou_a"], g["iou_b"]]):
        v = np.ascontiguousarray(v)
        R, t, s = np.zeros(9), np.zeros(3), np.zeros(3)
        host.box_host_fit(_p(v), _p(R), _p(t), _p(s))
        edges = [[1, 5], [2, 6], [3, 7], [4, 8], [1, 3], [5, 7], [2, 4], [6, 8], [1, 2], [3, 4], [5, 6], [7, 8]]
        s_ref = np.array([np.mean([np.linalg.norm(v[b] - v[e]) for b, e in edges[4 * a:4 * a + 4]]) for a in range(3)])
        sol = np.linalg.lstsq(np.concatenate([aabb(s_ref), np.ones((9, 1))], 1), v, rcond=None)[0]
        assert np.allclose(s, s_ref, rtol=1e-14, atol=0)
        assert np.allclose(R.reshape(3, 3), sol[:3, :3].T, rtol=0, atol=1e-12)
        assert np.allclose(t, sol[3], rtol=0, atol=1e-12)
        vol = host.box_host_volume(_p(v))
        i, j, k = v[2] - v[1], v[3] - v[1], v[5] - v[1]
        assert abs(vol - abs(np.linalg.det(np.array([i, j, k])))) <= 1e-14 * vol


def test_inside(host):
    from tools.make_box_eval_goldens import box, rot

    v = np.ascontiguousarray(box(rot([0.3, 1, 0.2], 0.7), [0.1, -0.2, -2.0], [0.4, 0.6, 0.3]))
    host.box_host_inside.restype = ctypes.c_int
    for p, want in (([0.1, -0.2, -2.0], 1), ([0.1, 0.2, -2.0], 0), (v[8] * 0.999 + v[0] * 0.001, 1), (v[8] + 1e-3, 0)):
        p = np.ascontiguousarray(p, np.float64)
        assert host.box_host_inside(_p(v), _p(p)) == want


def test_rotation_matches_scipy(host, g):
    """the evaluate_3d rotation: Rodrigues about v[3] - v[1] as scipy's from_rotvec(...).as_matrix() builds it,
    applied as (v - v[0]) @ R + v[0]"""
    from scipy.spatial.transform import Rotation

    for v in g["ev_pred3d"][:10]:
        v = np.ascontiguousarray(v)
        for th in list(np.linspace(0, 2 * np.pi, 7)) + [1e-4]:
            up = v[3] - v[1]
            R = Rotation.from_rotvec(th * up / np.linalg.norm(up)).as_matrix()
            want = (v - v[0]) @ R + v[0]
            got = np.zeros((9, 3))
            host.box_host_rotate(_p(v), th, _p(got))
            assert np.abs(got - want).max() < 1e-14


def test_eval_against_reference(host, g):
    out = eval_golden(lambda *a: host_eval(host, *a), g)
    check_against_reference(out, g)
    # the golden covers every branch: no IoU > 0, the mug break, a 2D best away from index 0, n in {1, 2, 7, 100, 180}
    assert (g["ev_ref"][:, 6] < 0).any() and g["ev_single"].any() and (g["ev_ref"][:, 7] > 0).any()
    assert set(np.unique(g["ev_nsym"])) == {1, 2, 7, 100, 180}


def test_mug_break_evaluates_index_zero_only(host, g):
    m = np.where(g["ev_single"] == 1)[0]
    out = eval_golden(lambda *a: host_eval(host, *a), g)
    assert np.all(out[m, 6] <= 0) and np.all(out[m, 7] == 0)


def sequence_images(g):
    """the golden's multi-image sequence as BoxEvaluator.evaluate input"""
    images, ib, ii = [], 0, 0
    for im, (nb, ni) in enumerate(zip(g["seq_nbox"], g["seq_ninst"])):
        boxes = [(g["seq_box2d"][k], g["seq_box3d"][k], g["seq_relscale"][k], g["seq_box2d"][k],
                  {"score": float(g["seq_score"][k])}) for k in range(ib, ib + nb)]
        label = {k: g["seq_" + k][ii:ii + ni] for k in ("2d_instance", "3d_instance", "scale_instance", "Mo2c_instance",
                                                        "visibility")}
        images.append((boxes, label, (g["seq_plane"][im, 0], g["seq_plane"][im, 1]), g["seq_proj"][im]))
        ib, ii = ib + nb, ii + ni
    return images


def check_sequence(ev, res, g):
    for m in box_metrics.METRICS:
        hit, miss = ev.hit_miss_arrays(m)
        assert np.array_equal(hit, g["seq_%s_hit" % m]), m
        assert np.array_equal(miss, g["seq_%s_miss" % m]), m
        assert np.array_equal(res["ap"][m], g["seq_%s_ap" % m]), (m, res["ap"][m], g["seq_%s_ap" % m])
    means = [res[k] for k in ("mean_error_scale", "mean_error_2d", "mean_iou_3d", "mean_error_azimuth",
                              "mean_error_polar")]
    assert np.allclose(means, g["seq_means"], rtol=1e-9, atol=1e-12), (means, g["seq_means"])
    assert res["matched"] == int(g["seq_matched"]) and res["flagged"] == 0


def test_evaluator_bookkeeping_against_reference(host, g):
    ev = box_metrics.BoxEvaluator(num_symmetry=int(g["seq_nsym"]), pair_metrics=lambda *a: host_eval(host, *a))
    imgs = sequence_images(g)
    ev.evaluate(imgs[:2])  # any split into calls gives the same records
    ev.evaluate(imgs[2:])
    check_sequence(ev, ev.finalize(), g)


def test_evaluator_without_instances_raises():
    ev = box_metrics.BoxEvaluator(pair_metrics=lambda *a: pytest.fail("no pair expected"))
    with pytest.raises(ValueError):
        ev.finalize()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "centerpose_hip.h")).read(), flags=re.S)
    return set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", text))


def test_box_symbols_exported_and_declared():
    L = hip.lib()
    for name in ("cp_box_iou", "cp_box_eval"):
        assert hasattr(L, name) and name in hip.exported_symbols() and name in _declared()
    assert hip.ABI_VERSION == L.cp_abi_version() == 7
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    assert re.search(r"#define CP_BOX_EVAL_STRIDE %d\b" % hip.BOX_EVAL_STRIDE, header)
    assert len(hip.BOX_EVAL_FIELDS) == hip.BOX_EVAL_STRIDE


def test_box_argument_checks():
    """refused before anything is launched (placeholder pointers are never dereferenced)"""
    L = hip.lib()
    p = c_void_p(4096)
    assert L.cp_box_iou(None, p, p, 0, p) == -1
    assert L.cp_box_iou(None, None, p, 4, p) == -1
    assert L.cp_box_iou(None, p, p, 4, None) == -1
    assert L.cp_box_eval(None, p, p, p, p, p, p, 0, 100, p) == -1
    assert L.cp_box_eval(None, p, p, p, p, p, p, 4, 0, p) == -1
    assert b"num_symmetry" in L.cp_last_error()
    for k in range(7):
        args = [p] * 7
        args[k] = None
        assert L.cp_box_eval(None, *args[:6], 4, 100, args[6]) == -1


def test_clip_leaves_out_the_wraparound_repeat(host):
    """An on-plane LAST vertex: the reference's _clip_poly emits it as `prev` at i = 0 and again as `cur` at i = n - 1
    (five points from four).  clip_poly gives the same points without that closing repeat of output[0], so a pass grows
    a polygon by at most one vertex and a face clipped by 6 planes fits MAXV = 10."""
    host.box_host_clip.restype = ctypes.c_int
    host.box_host_clip.argtypes = [c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_void_p,
                                   c_void_p]
    quad = np.array([[1., 0, 0], [1, 1, 0], [-1, 1, 0], [0, 0, 0]])  # front, front, behind, on the plane x = 0
    reference = [quad[3], quad[0], quad[1], np.array([0., 1, 0]), quad[3]]  # iou.py:128-160 traced by hand
    out, fl = np.zeros((10, 3)), np.zeros(1, np.int32)
    m = host.box_host_clip(_p(np.ascontiguousarray(quad)), 4, 0.0, 1.0, 0, _p(out), _p(fl))
    assert m == 4 and fl[0] == 0
    assert np.array_equal(out[:m], np.array(reference[:-1]))
    # every clip of the golden's boxes stays within the capacity (box_host_iou asserts no CLIP_OVERFLOW)
    rng = np.random.RandomState(3)
    for _ in range(200):
        n = rng.randint(3, 9)
        ang = np.sort(rng.uniform(0, 2 * np.pi, n))
        poly = np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang), rng.randn(n) * 0.1], 1))
        poly[-1, 0] = 0.0 if rng.rand() < 0.5 else poly[-1, 0]  # often a last vertex on the plane
        m = host.box_host_clip(_p(poly), n, 0.0, 1.0 if rng.rand() < 0.5 else -1.0, 0, _p(out), _p(fl))
        assert m <= n + 1 and fl[0] == 0


class _Recorder(object):
    """a pair_metrics stand-in: records what BoxEvaluator hands the device and returns fixed records"""

    def __init__(self, rows):
        self.rows, self.calls = np.asarray(rows, np.float64), []

    def __call__(self, pred3d, gt3d, pred2d, mo2c, proj, single, num_symmetry):
        self.calls.append(dict(pred3d=pred3d, gt3d=gt3d, single=np.asarray(single), num_symmetry=num_symmetry))
        return self.rows[:len(single)]


def _two_instance_frame():
    from tools.make_box_eval_goldens import box, gl_projection, mo2c, project, rot

    P = gl_projection()
    objs = [(rot([0, 1, 0], 0.3), np.array([-0.4, -0.2, -2.5]), np.array([0.3, 0.4, 0.3])),
            (rot([0, 1, 0], -0.8), np.array([0.5, -0.1, -3.0]), np.array([0.2, 0.3, 0.25]))]
    g3 = np.array([box(R, t, s) for R, t, s in objs])
    label = {"2d_instance": np.array([project(P, v) for v in g3]), "3d_instance": g3,
             "scale_instance": np.array([s for _, _, s in objs]), "Mo2c_instance": np.array([mo2c(R, t) for R, t, _ in objs]),
             "visibility": np.array([0.9, 0.8]), "MugFlag_instance": np.array([True, False])}
    # predictions up to scale (half size, half distance: the same projection), in reverse order of the instances
    boxes = [(project(P, g3[k] * 0.5), g3[k] * 0.5, objs[k][2], None, {"score": 0.9 - 0.1 * k}) for k in (1, 0)]
    normal = rot([0, 1, 0], 0.3) @ np.array([0, 1., 0])
    plane = (objs[0][1] - normal * objs[0][2][1] / 2, normal)  # under the first object
    return boxes, label, plane, P


def test_evaluator_mug_flag_and_scale_paths():
    """MugFlag_instance of the MATCHED instance becomes the pair's single-rotation flag only with mug_symmetric=False;
    use_absolute_scale=True hands the detector's 3D points over unchanged, False rescales them on the ground plane"""
    frame = _two_instance_frame()
    rows = [[0.8, 0.05, 0.05, 3., 2., 0.01, 0, 0, 0]] * 2
    for mug_symmetric, want in ((False, [0, 1]), (True, [0, 0])):
        rec = _Recorder(rows)
        box_metrics.BoxEvaluator(num_symmetry=100, mug_symmetric=mug_symmetric, pair_metrics=rec).evaluate([frame])
        assert rec.calls[0]["single"].tolist() == want and rec.calls[0]["num_symmetry"] == 100
        assert np.array_equal(rec.calls[0]["gt3d"], frame[1]["3d_instance"][[1, 0]])
    rec = _Recorder(rows)
    box_metrics.BoxEvaluator(use_absolute_scale=True, pair_metrics=rec).evaluate([frame])
    assert np.array_equal(rec.calls[0]["pred3d"], np.array([frame[0][0][1], frame[0][1][1]]))
    rec = _Recorder(rows)
    ev = box_metrics.BoxEvaluator(use_absolute_scale=False, pair_metrics=rec)
    ev.evaluate([frame])
    scaled = rec.calls[0]["pred3d"]
    # the box standing on the plane (instance 0, the second prediction) is put back at its metric size
    assert np.allclose(scaled[1], frame[1]["3d_instance"][0], rtol=0, atol=1e-12)
    for k in range(2):
        f = box_metrics.BoxEvaluator.compute_scale(frame[0][k][1], frame[2])
        assert np.array_equal(scaled[k], frame[0][k][1] * f)


def test_evaluator_flagged_pairs():
    """a singular ray solve (flag 1, NaN viewpoint errors): a miss at every viewpoint threshold, counted in 'flagged',
    left out of the viewpoint means; a singular Mo2c (flag 2) or a clip overflow (flag 4) raises before anything is
    recorded"""
    frame = _two_instance_frame()
    rows = [[0.8, 0.05, 0.05, np.nan, np.nan, 0.01, 0, 0, 1], [0.7, 0.05, 0.05, 3., 2., 0.01, 0, 0, 0]]
    ev = box_metrics.BoxEvaluator(pair_metrics=_Recorder(rows))
    ev.evaluate([frame])
    res = ev.finalize()
    assert res["flagged"] == 1 and res["matched"] == 2
    assert res["mean_error_azimuth"] == 3.0 and res["mean_error_polar"] == 2.0
    assert res["mean_iou_3d"] == (0.8 + 0.7) / 2
    hit, _ = ev.hit_miss_arrays("azimuth")
    assert hit[:, 0, 0].sum() == 0  # the NaN record never hits
    for flag in (2, 4):
        bad = [[0.8, 0.05, 0.05, 3., 2., np.nan, 0, 0, flag]] * 2
        ev = box_metrics.BoxEvaluator(pair_metrics=_Recorder(bad))
        with pytest.raises(ValueError):
            ev.evaluate([frame])
        assert ev.matched == 0 and ev.total_instances == 0
