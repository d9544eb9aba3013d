"""Writes tests/golden/box_eval_ref.npz: the reference evaluator's own Objectron box metrics on seeded float64 cases.

Runs only where the reference project exists ($CENTERPOSE_REFERENCE, as oracle/tools/ref_harness.py): it imports the
reference's `src/tools/objectron_eval/eval_image_official.py` unmodified (with `objectron/dataset/{box,iou,
metrics_nvidia}.py` behind it) and calls its methods on an `object.__new__` Evaluator with a small `opt`.  The modules
that file imports for the detector, TFRecords and drawing are stubbed as empty modules, `eigenpy.switchToNumpyArray`
is a no-op, `np.float = float`, and `rotation_util` gets a shim whose `as_dcm()` is scipy's `as_matrix()` (scipy >= 1.6
has no `as_dcm`).  Only the outputs are stored.

  python tools/make_box_eval_goldens.py      # rewrites the .npz bit for bit

Contents (float64 unless noted):
  iou_a, iou_b [M,9,3], iou_ref [M], iou_kind [M] int   IoU3D.IoU(Box(a), Box(b)).iou() (0 where it raises)
  ev_pred3d, ev_gt3d [P,9,3], ev_pred2d [P,9,2], ev_mo2c, ev_proj [P,4,4], ev_single [P] int, ev_nsym [P] int
  ev_ref [P,8]       evaluate_3d / evaluate_2d: iou, ADD, ADD-S, azimuth, polar, 2D error, best 3D index (-1 none),
                     best 2D index (the last index each method reports as an improvement)
  ev_rot_{iou,add,adds,az,pol} [P,180]  evaluate_iou, compute_average_distance and evaluate_viewpoint of every
                     rotation of the 3D sweep (NaN past n): a rotation that ties the best IoU to < 1e-9 may be the
                     one reported
  seq_*              a multi-image sequence through the reference's own Evaluator.evaluate (stubbed parser and
                     detector) and finalize(): its HitMiss records and AP arrays per metric
"""
import contextlib
import io
import os
import re
import sys
import types

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REF = os.environ.get("CENTERPOSE_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "box_eval_ref.npz")
METRICS = ("scale", "iou", "pixel", "azimuth", "polar", "add", "adds")

# the sequence's camera: Objectron's 1440 x 1920 frame at eval_resolution_ratio 1 and an OpenGL projection of it
SEQ_W, SEQ_H = 1440, 1920


def _import_reference():
    src = os.path.join(REF, "src", "tools", "objectron_eval")
    if not os.path.isfile(os.path.join(src, "eval_image_official.py")):
        raise SystemExit("reference evaluator not found under %s (set CENTERPOSE_REFERENCE)" % REF)
    for name in ("tensorflow", "tqdm", "simplejson", "cv2", "objectron.dataset.parser", "lib", "lib.utils",
                 "lib.utils.pnp", "lib.utils.pnp.cuboid_pnp_shell", "lib.detectors", "lib.detectors.detector_factory",
                 "lib.opts", "eval_opts", "eval_utils", "eigenpy"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["eigenpy"].switchToNumpyArray = lambda: None
    sys.modules["lib.utils.pnp.cuboid_pnp_shell"].pnp_shell = None
    sys.modules["lib.detectors.detector_factory"].detector_factory = {}
    sys.modules["lib.opts"].opts = None
    sys.modules["eval_opts"].eval_opts = None
    sys.modules["eval_utils"].draw_axes = None
    sys.modules["cv2"].cvtColor = lambda img, code: img
    sys.modules["cv2"].COLOR_RGB2BGR = 4
    tf = sys.modules["tensorflow"]
    tf.train = types.SimpleNamespace(Example=types.SimpleNamespace(FromString=lambda s: s))
    np.float = float
    import matplotlib

    matplotlib.use("Agg")
    sys.path.insert(0, src)
    import objectron  # noqa: F401  (the package itself; its parser submodule is the stub above)

    sys.modules["objectron.dataset.parser"] = types.ModuleType("objectron.dataset.parser")
    import eval_image_official as E
    from scipy.spatial.transform import Rotation

    class _RotShim:
        @staticmethod
        def from_rotvec(v):
            r = Rotation.from_rotvec(v)
            return types.SimpleNamespace(as_dcm=r.as_matrix)

        @staticmethod
        def from_dcm(m):
            return Rotation.from_matrix(m)

    E.rotation_util = _RotShim
    import objectron.dataset.box as B
    import objectron.dataset.iou as I

    return E, B, I


def _evaluator(E, num_symmetry, mug_symmetric=True, use_absolute_scale=False):
    ev = object.__new__(E.Evaluator)
    ev.opt = types.SimpleNamespace(eval_num_symmetry=num_symmetry, eval_mug_symmetric=mug_symmetric, c="chair",
                                   use_absolute_scale=use_absolute_scale, eval_MobilePose_postprocessing=False,
                                   eval_gt_scale=False, eval_debug=False, eval_debug_json=False, eval_skip=-10 ** 9,
                                   eval_subset_list=None, batch_size=1, eval_resolution_ratio=1)
    ev.height, ev.width = SEQ_H, SEQ_W
    ev._vis_thresh = 0.1
    ev._error_scale = ev._error_2d = ev._iou_3d = ev._azimuth_error = ev._polar_error = 0.
    ev._matched = 0
    nb = E._NUM_BINS
    ev._scale_thresholds = np.linspace(0.0, 1., num=nb)
    ev._iou_thresholds = np.linspace(0.0, 1., num=nb)
    ev._pixel_thresholds = np.linspace(0.0, E._MAX_PIXEL_ERROR, num=nb)
    ev._azimuth_thresholds = np.linspace(0.0, E._MAX_AZIMUTH_ERROR, num=nb)
    ev._polar_thresholds = np.linspace(0.0, E._MAX_POLAR_ERROR, num=nb)
    ev._add_thresholds = np.linspace(0.0, E._MAX_DISTANCE, num=nb)
    ev._adds_thresholds = np.linspace(0.0, E._MAX_DISTANCE, num=nb)
    for m in METRICS:
        setattr(ev, "_%s_ap" % m, E.metrics.AveragePrecision(nb))
    ev.NUM_SAMPLE = 0
    ev.filename_list = []
    return ev


# ---------------------------------------------------------------------------------------------------------- geometry
def aabb(s):
    w, h, d = np.asarray(s, np.float64) / 2.
    return np.array([[0, 0, 0], [-w, -h, -d], [-w, -h, d], [-w, h, -d], [-w, h, d], [w, -h, -d], [w, -h, d], [w, h, -d],
                     [w, h, d]], np.float64)


def rot(axis, a):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def rand_rot(rng):
    q = rng.randn(4)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def box(R, t, s):
    return aabb(s) @ np.asarray(R).T + np.asarray(t)


def mo2c(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M


def gl_projection(fx=1.5, fy=2.0, cx=0.01, cy=-0.02, near=0.05, far=100.):
    return np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, -(far + near) / (far - near), -2 * far * near / (far - near)],
                     [0, 0, -1, 0]])


def project(P, pts):
    """the evaluator's viewport convention: (p + 1) / 2 of the OpenGL projection, x and y swapped"""
    q = P @ np.hstack([pts, np.ones((len(pts), 1))]).T
    v = (q[:2] / q[3] + 1.0) / 2.0
    return np.stack([v[1], v[0]], 1)


def object_pose(rng, z=(-3.0, -1.2)):
    """an upright object in the camera frame (the evaluator's OpenGL convention: the camera looks along -z), yawed about
    its own up axis and tilted a little"""
    R = rot([1, 0, 0], rng.uniform(0.2, 0.6)) @ rot([0, 1, 0], rng.uniform(-np.pi, np.pi))
    t = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.4, 0.1), rng.uniform(*z)])
    s = np.array([rng.uniform(0.2, 0.6), rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.6)])
    return R, t, s


# ---------------------------------------------------------------------------------------------------------- cases
def iou_cases(rng):
    """(a, b, kind): 0 random pair, 1 identical, 2 disjoint, 3 nested, 4 shared face plane, 5 touching faces with
    opposite normals, 6 edge contact, 7 vertex contact, 8 vertices within 1e-6 of a plane, 9 noisy non-cuboid"""
    cases = []
    for _ in range(60):  # random pairs across the IoU range
        R, t, s = object_pose(rng)
        a = box(R, t, s)
        k = rng.randint(4)
        if k == 0:
            b = box(R @ rot([0, 1, 0], rng.uniform(-0.6, 0.6)), t + rng.randn(3) * 0.05, s * rng.uniform(0.8, 1.2, 3))
        elif k == 1:
            b = box(rand_rot(rng), t + rng.randn(3) * 0.1, s * rng.uniform(0.5, 1.5, 3))
        elif k == 2:
            b = box(R, t + rng.randn(3) * 0.2, s * rng.uniform(0.7, 1.3, 3))
        else:
            b = box(rot(rng.randn(3), rng.uniform(0, 0.3)) @ R, t + rng.randn(3) * 0.02, s)
        cases.append((a, b, 0))
    for _ in range(4):
        R, t, s = object_pose(rng)
        a = box(R, t, s)
        cases.append((a, a.copy(), 1))
        cases.append((a, box(R, t + R @ np.array([s[0] * 1.7, 0, 0]), s), 2))
        cases.append((a, box(R, t + R @ np.array([0.01, -0.02, 0.01]) * s, s * 0.5), 3))
        # shared face plane: b is a's half along x, sharing a's +x face (same outward normal)
        sb = s * np.array([0.5, 1, 1])
        cases.append((a, box(R, t + R @ np.array([s[0] / 4, 0, 0]), sb), 4))
        # shared face plane, partly overlapping in that plane
        cases.append((a, box(R, t + R @ np.array([s[0] / 4, 0.3 * s[1], -0.2 * s[2]]), sb), 4))
        cases.append((a, box(R, t + R @ np.array([s[0], 0, 0]), s), 5))  # face to face, opposite normals
        cases.append((a, box(R, t + R @ np.array([s[0], s[1], 0]), s), 6))  # along an edge
        cases.append((a, box(R, t + R @ np.array([s[0], s[1], s[2]]), s), 7))  # at a vertex
        # b's -x face within 1e-6 of a's +x face plane, in a's frame (metre-sized boxes: the hull of such a sliver
        # and the divergence sum differ by O(1e-6 x face area / volume) in IoU)
        sl = np.array([0.8, 0.9, 1.0])
        for eps in (4e-7, -4e-7, 9e-7):
            cases.append((box(R, t, sl), box(R, t + R @ np.array([sl[0] / 2 + sl[0] / 2 * 0.6 + eps, 0.1 * sl[1], 0]),
                                             sl * np.array([0.6, 0.8, 0.7])), 8))
    for _ in range(12):  # noisy, non-cuboid vertex sets: the lstsq fit
        R, t, s = object_pose(rng)
        a = box(R, t, s) + rng.randn(9, 3) * 0.01
        b = box(R @ rot([0, 1, 0], rng.uniform(-0.3, 0.3)), t + rng.randn(3) * 0.03, s) + rng.randn(9, 3) * 0.01
        cases.append((a, b, 9))
    return cases


def eval_cases(rng):
    """(pred3d, gt3d, pred2d, mo2c, proj, single, nsym)"""
    P = gl_projection()
    cases = []
    for nsym in (1, 2, 7, 100, 180):
        for i in range(7):
            R, t, s = object_pose(rng)
            gt = box(R, t, s)
            M = mo2c(R, t)
            if i == 5:  # far from the ground truth: no rotation has IoU > 0
                pr = box(R, t + np.array([2.0, 0, -1.0]), s)
            else:
                yaw = rng.uniform(-np.pi, np.pi) if i % 2 else rng.uniform(-0.2, 0.2)
                pr = box(R @ rot([0, 1, 0], yaw) @ rot(rng.randn(3), rng.uniform(0, 0.05)),
                         t + rng.randn(3) * 0.03, s * rng.uniform(0.9, 1.1, 3))
                if i == 6:
                    pr = pr + rng.randn(9, 3) * 0.005
            p2 = project(P, gt) + rng.randn(9, 2) * 0.004
            single = 1 if (i == 3 and nsym > 1) else 0  # the mug break: index 0 only
            cases.append((pr, gt, p2, M, P, single, nsym))
    return cases


def run_eval_case(E, c):
    pr, gt, p2, M, P, single, nsym = c
    ev = _evaluator(E, nsym, mug_symmetric=not single)
    flag = True if single else []
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        err2d = ev.evaluate_2d(p2, None, gt, M, P, flag)
    b2 = int(buf.getvalue().strip().splitlines()[-1].split(":")[0])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        az, pol, iou, _, _, add, adds = ev.evaluate_3d(pr, gt, M, flag)
    lines = [ln for ln in buf.getvalue().splitlines() if re.match(r"^\d+: ", ln)]
    b3 = int(lines[-1].split(":")[0]) if lines else -1
    rots = np.full((5, 180), np.nan)  # per rotation: IoU, ADD, ADD-S, azimuth, polar error
    for k, th in enumerate(np.linspace(0, np.pi * 2, nsym)):
        rb = ev._get_rotated_box(pr, th)
        rots[0, k] = ev.evaluate_iou(rb, gt)[0]
        rots[1:3, k] = ev.compute_average_distance(rb, gt)
        rots[3:5, k] = ev.evaluate_viewpoint(rb, gt)
    return np.array([iou, add, adds, az, pol, err2d, b3, b2], np.float64), rots


def sequence(rng):
    """images of 1-3 labelled objects standing on one ground plane, each with its detector-style boxes: matched
    detections (near the pose, or turned about the up axis), unmatched ones (nearest annotation below the visibility
    threshold), repeated scores.  Predictions are up to scale, as PnP returns them, and go back to metric scale on the
    ground plane (compute_scale); sizes stay close to the annotation's, so no sweep meets a plateau of nested boxes
    whose many equal IoUs would leave the reported rotation to rounding."""
    P = gl_projection()
    imgs = []
    for im in range(6):
        n = 1 + im % 3
        Rc = rot([1, 0, 0], rng.uniform(0.2, 0.5))  # camera pitch: the level frame -> the camera frame
        h_cam = rng.uniform(1.0, 1.5)
        normal = Rc @ np.array([0, 1., 0])
        center = Rc @ np.array([0, -h_cam, -2.5])
        objs = []
        for k in range(n):
            s = np.array([rng.uniform(0.25, 0.5), rng.uniform(0.3, 0.6), rng.uniform(0.25, 0.5)])
            p = np.array([-0.9 + 0.9 * k + rng.uniform(-0.1, 0.1), -h_cam + s[1] / 2, rng.uniform(-3.5, -2.0)])
            objs.append((Rc @ rot([0, 1, 0], rng.uniform(-np.pi, np.pi)), Rc @ p, s))
        inst2d, inst3d, scale, M, vis = [], [], [], [], []
        for k, (R, t, s) in enumerate(objs):
            g3 = box(R, t, s)
            inst3d.append(g3)
            inst2d.append(project(P, g3))
            scale.append(s)
            M.append(mo2c(R, t))
            vis.append(0.05 if (im == 4 and k == 1) else rng.uniform(0.3, 1.0))
        inst2d, inst3d = np.array(inst2d), np.array(inst3d)
        plane = (center, normal)
        boxes = []
        for k, (R, t, s) in enumerate(objs):
            for rep in range(1 if im % 2 else 2):
                depth = rng.uniform(0.6, 1.4)
                yaw = rng.uniform(-0.3, 0.3) if rep == 0 else rng.uniform(1.0, 2.5)
                pr3 = box(R @ rot([0, 1, 0], yaw), t + rng.randn(3) * 0.02, s * rng.uniform(0.95, 1.05, 3)) * depth
                pr2 = project(P, pr3) + rng.randn(9, 2) * 0.003
                rel = s * rng.uniform(0.9, 1.1, 3)
                score = [0.9, 0.7, 0.7, 0.55, 0.3][(im + k + rep) % 5]
                res = {"score": score, "kps_displacement_mean": np.zeros(16), "kps_heatmap_mean": np.zeros(16)}
                boxes.append((pr2, pr3, rel, pr2.copy(), res))
        label = {"2d_instance": inst2d, "3d_instance": inst3d, "scale_instance": np.array(scale),
                 "Mo2c_instance": np.array(M), "visibility": np.array(vis), "image_id": im}
        imgs.append((boxes, label, plane, P))
    return imgs


def run_sequence(E, imgs, nsym):
    ev = _evaluator(E, nsym)
    by_id = {}

    class _Parser:
        def parse_example(self, ex):
            return np.zeros((4, 4, 3), np.uint8), by_id[ex][1], "img%d" % ex

        def parse_camera(self, ex):
            return by_id[ex][3], np.eye(4), np.eye(3)

        def parse_plane(self, ex):
            return by_id[ex][2]

    class _Detector:
        cur = None

        def run(self, image, filename=None, meta_inp=None):
            return {"boxes": [tuple(b) for b in by_id[int(filename.split("_")[0][3:])][0]]}

    ev.encoder = _Parser()
    ev.detector = _Detector()
    with contextlib.redirect_stdout(io.StringIO()):
        for i, img in enumerate(imgs):
            by_id[i] = img
            ev.NUM_SAMPLE += 1
            ev.evaluate([i])
    ev.finalize()
    out = {}
    for m in METRICS:
        ap = getattr(ev, "_%s_ap" % m)
        out["seq_%s_hit" % m] = np.array([[row for img in ap.true_positive[i] for row in img] for i in range(ap.size)],
                                         np.float64).reshape(ap.size, -1, 2)
        out["seq_%s_miss" % m] = np.array([[row for img in ap.false_positive[i] for row in img] for i in range(ap.size)],
                                          np.float64).reshape(ap.size, -1, 2)
        out["seq_%s_ap" % m] = np.asarray(ap.aps, np.float64)
    out["seq_means"] = np.array([E.safe_divide(v, ev._matched) for v in (ev._error_scale, ev._error_2d, ev._iou_3d,
                                                                         ev._azimuth_error, ev._polar_error)])
    out["seq_matched"] = np.array(ev._matched)
    return out


def main():
    E, B, I = _import_reference()
    rng = np.random.RandomState(20261015)
    out = {}
    cases = iou_cases(rng)
    refs = []
    for a, b, _ in cases:
        try:
            refs.append(I.IoU(B.Box(a), B.Box(b)).iou())
        except Exception:
            refs.append(0.)
    out["iou_a"] = np.array([c[0] for c in cases])
    out["iou_b"] = np.array([c[1] for c in cases])
    out["iou_kind"] = np.array([c[2] for c in cases], np.int32)
    out["iou_ref"] = np.array(refs, np.float64)
    ev = eval_cases(rng)
    res = [run_eval_case(E, c) for c in ev]
    out["ev_pred3d"] = np.array([c[0] for c in ev])
    out["ev_gt3d"] = np.array([c[1] for c in ev])
    out["ev_pred2d"] = np.array([c[2] for c in ev])
    out["ev_mo2c"] = np.array([c[3] for c in ev])
    out["ev_proj"] = np.array([c[4] for c in ev])
    out["ev_single"] = np.array([c[5] for c in ev], np.int32)
    out["ev_nsym"] = np.array([c[6] for c in ev], np.int32)
    out["ev_ref"] = np.array([r[0] for r in res])
    for k, name in enumerate(("iou", "add", "adds", "az", "pol")):
        out["ev_rot_" + name] = np.array([r[1][k] for r in res])
    imgs = sequence(rng)
    # 100 rotations, as the reference's shell scripts: n - 1 = 99 is odd, so no rotation is the half turn that maps a
    # cuboid onto itself with renamed vertices (an IoU tie whose winner would rest on rounding and decide ADD / azimuth)
    out["seq_nsym"] = np.array(100, np.int32)
    out.update(run_sequence(E, imgs, 100))
    # the sequence's inputs, flattened: per image the number of boxes / instances, then the concatenated arrays
    out["seq_nbox"] = np.array([len(b) for b, _, _, _ in imgs], np.int32)
    out["seq_ninst"] = np.array([len(l["visibility"]) for _, l, _, _ in imgs], np.int32)
    out["seq_box2d"] = np.concatenate([np.array([x[0] for x in b]) for b, _, _, _ in imgs])
    out["seq_box3d"] = np.concatenate([np.array([x[1] for x in b]) for b, _, _, _ in imgs])
    out["seq_relscale"] = np.concatenate([np.array([x[2] for x in b]) for b, _, _, _ in imgs])
    out["seq_score"] = np.concatenate([np.array([x[4]["score"] for x in b]) for b, _, _, _ in imgs])
    for k in ("2d_instance", "3d_instance", "scale_instance", "Mo2c_instance", "visibility"):
        out["seq_" + k] = np.concatenate([l[k] for _, l, _, _ in imgs])
    out["seq_plane"] = np.array([np.stack(p) for _, _, p, _ in imgs])
    out["seq_proj"] = np.array([P for _, _, _, P in imgs])
    buf = io.BytesIO()
    np.savez(buf, **out)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print("wrote %s: %d IoU cases, %d evaluate cases, %d images" % (OUT, len(cases), len(ev), len(imgs)))


if __name__ == "__main__":
    main()
