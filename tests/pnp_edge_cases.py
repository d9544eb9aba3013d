"""Case generator for the PnP edge tests (tests/test_pnp_edges_cpu.py checks its premises on the oracle alone,
tests/test_pnp_edges_gpu.py runs the device solver on it).  No tests in here.

Every family is a seeded builder that returns a ``Cases`` record: ``pts [N,npts,2] float32``, ``scale [N,3] float32``,
``cam [N,4] float64`` (fx, fy, cx, cy), the generating ``R [N,3,3]`` / ``t [N,3]`` (NaN where a row has none), ``exact``
(the image points are the float32-rounded projections of that pose, nothing else) and a ``names`` list.  The data are
built with oracle/pnp.py alone (cuboid_vertices, rodrigues_to_matrix, matrix_to_rodrigues, project_points); the one
projection written out here (``project_R``, which takes the rotation MATRIX so that rotations by pi - 1e-12 do not pass
through a rotation vector first) is pinned to oracle.pnp.project_points by the CPU test.

``oracle_rows`` is the reference side of every comparison: oracle/pnp.solve_cuboid_pnp per row, with the reason when
there is no pose.  ``LIMITS`` / ``GENERATING_LIMITS`` are the comparison limits of the GPU tests; how they were set is
written beside them, and ``python -m tests.pnp_edge_cases`` prints the oracle-only measurements they come from.
"""
import warnings
from types import SimpleNamespace

import numpy as np

from oracle import pnp as opnp

CAM0 = np.array([663.0287679036459, 663.0287679036459, 300.2775065104167, 395.00066121419275])
INVALID = -10000.0
M_GL = np.array([[0, 1, 0], [1, 0, 0], [0, 0, -1]], np.float64)  # cuboid_pnp_solver.py:179-196
PLANAR_THRESHOLD = 1e-3  # cvFindExtrinsicCameraParams2 / oracle.pnp.is_planar / pnp.hip
SWITCH_MARGINS = (0.5, 0.1, 0.01, 1e-4)
SWITCH_MIN_DISTANCE = 1e-6  # relative; closer than this the device's Jacobi and numpy's SVD may disagree legitimately
THETAS = (0.0, 1e-12, 1e-8, 1e-4, np.pi - 1e-4, np.pi - 1e-8, np.pi - 1e-12, np.pi)
AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), tuple(np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)))

# Rows per family (one oracle solve each; tests/test_pnp_edges_cpu.py asserts these and the <= 200 solves per test).
ROWS = {"planar_switch": 64, "singular_rotation": 72, "validity_patterns": 88, "camera_and_placement": 58,
        "useless_inputs": 13}


def Kmat(cam4):
    fx, fy, cx, cy = [float(v) for v in cam4]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def project_R(verts, R, t, cam4):
    """oracle.pnp.project_points with the rotation given as a matrix."""
    P = verts @ np.asarray(R, np.float64).T + np.asarray(t, np.float64).reshape(1, 3)
    return np.stack([cam4[0] * P[:, 0] / P[:, 2] + cam4[2], cam4[1] * P[:, 1] / P[:, 2] + cam4[3]], axis=1)


def rel_verts(scale_f32):
    s = np.asarray(scale_f32, np.float32).astype(np.float64)
    return opnp.cuboid_vertices(s / s[1])  # cuboid_pnp_shell.py:12


def random_rotation(rng):
    q = rng.randn(4)
    return opnp.quat_xyzw_to_matrix(q / np.linalg.norm(q))


def rotation_angle(R):
    """Angle of a rotation matrix, accurate at 0 and at pi (atan2 of |sin| and cos, not acos of the trace)."""
    s = 0.5 * np.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2 + (R[1, 0] - R[0, 1]) ** 2)
    return float(np.arctan2(s, 0.5 * (np.trace(R) - 1.0)))


def scatter_ratio(pts_row, scale_row):
    """e2 / e1 of the valid model points' scatter, in float64 exactly as oracle.pnp.is_planar forms it."""
    verts = rel_verts(scale_row)
    per = len(pts_row) // 8
    obj = np.array([verts[k // per] for k in range(len(pts_row)) if not (pts_row[k, 0] < -5000 or pts_row[k, 1] < -5000)])
    Mc = obj.mean(axis=0)
    w = np.linalg.svd((obj - Mc).T @ (obj - Mc), compute_uv=False)
    return w[2] / w[1]


class _Builder:
    def __init__(self, npts):
        self.npts = npts
        self.pts, self.scale, self.cam, self.R, self.t, self.exact, self.names = [], [], [], [], [], [], []

    def add(self, name, sc, R, t, cam4=CAM0, noise=0.0, rng=None, valid=None, exact=None):
        sc32 = np.asarray(sc, np.float32)
        uv = project_R(rel_verts(sc32), R, t, cam4)
        p = np.repeat(uv, self.npts // 8, axis=0)
        if noise > 0:
            p = p + rng.randn(self.npts, 2) * noise
        if valid is not None:
            p[~np.asarray(valid, bool)] = INVALID
        self.pts.append(p.astype(np.float32))
        self.scale.append(sc32)
        self.cam.append(np.asarray(cam4, np.float64))
        self.R.append(np.asarray(R, np.float64))
        self.t.append(np.asarray(t, np.float64))
        self.exact.append(noise == 0 if exact is None else exact)
        self.names.append(name)
        return len(self.names) - 1

    def done(self, **extra):
        return SimpleNamespace(pts=np.stack(self.pts), scale=np.stack(self.scale), cam=np.stack(self.cam), R=np.stack(self.R),
                               t=np.stack(self.t), exact=np.array(self.exact, bool), names=list(self.names), npts=self.npts,
                               **extra)


def take(c, idx):
    """The rows ``idx`` of a Cases record."""
    idx = list(idx)
    return SimpleNamespace(pts=c.pts[idx].copy(), scale=c.scale[idx].copy(), cam=c.cam[idx].copy(), R=c.R[idx].copy(),
                           t=c.t[idx].copy(), exact=c.exact[idx].copy(), names=[c.names[i] for i in idx], npts=c.npts)


def _pose(rng, z=(6.0, 12.0)):
    return random_rotation(rng), np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(*z)])


# ----------------------------------------------------------------------------------------------------------------
def planar_switch(seed=101):
    """Cuboids (a, 1, th) and (th, 1, a), all 16 points valid: the scatter's eigenvalues are 4 (a^2, 1, th^2), so e2 / e1 is
    th^2 for a > 1 and th^2 / a^2 for a < 1; th puts it at 1e-3 (1 +- m).  ``side`` is +1 where the DLT start must be taken
    (ratio above the threshold), -1 where the homography start must; ``ratio`` is the float64 ratio of the float32 sizes."""
    rng = np.random.RandomState(seed)
    b = _Builder(16)
    side, ratio, margin = [], [], []
    for a in (2.0, 0.5):
        for thin in ("z", "x"):
            for m in SWITCH_MARGINS:
                for sgn in (+1, -1):
                    th = np.sqrt(PLANAR_THRESHOLD * (1 + sgn * m)) * min(a, 1.0)
                    sc = (a, 1.0, th) if thin == "z" else (th, 1.0, a)
                    R, t = _pose(rng)
                    for noise in (0.0, 0.5):
                        i = b.add("a=%g thin=%s m=%+g noise=%g" % (a, thin, sgn * m, noise), sc, R, t, noise=noise, rng=rng)
                        r = scatter_ratio(b.pts[i], b.scale[i])
                        if abs(r / PLANAR_THRESHOLD - 1) < SWITCH_MIN_DISTANCE:  # (float32 rounding of th moved it too close)
                            raise AssertionError("planar_switch case %s lies at %.3e of the threshold" % (b.names[i], r / 1e-3 - 1))
                        side.append(sgn)
                        ratio.append(r)
                        margin.append(m)
    return b.done(side=np.array(side), ratio=np.array(ratio), margin=np.array(margin))


def singular_rotation(seed=102):
    """Exact data.  Rotations by THETAS about AXES: once as the OpenCV-frame rotation R, once as the OpenGL-frame rotation
    M R (R = M^T rot(axis, theta)), the frame in which write_pose calls rot_to_rvec / axis_angle_quat a second time.  The
    last row is a planar set (one cuboid face, both candidates) seen exactly edge-on along the image's vertical: every
    image point has the same u, the homography's normalisation has no x spread (homography_dlt returns None), and
    cvFindExtrinsicCameraParams2 / planar_init fall back to r = t = 0."""
    b = _Builder(16)
    frame, theta = [], []
    t = np.array([0.1, -0.05, 8.0])
    sc = (1.3, 1.0, 0.7)
    for fr in ("cv", "gl"):
        for ax in AXES:
            for th in THETAS:
                Rax = opnp.rodrigues_to_matrix(np.array(ax) * th)
                b.add("%s axis=(%.2g,%.2g,%.2g) theta=%.17g" % ((fr,) + tuple(ax) + (th,)), sc, Rax if fr == "cv" else M_GL.T @ Rax, t)
                frame.append(fr)
                theta.append(th)
    # The same angles with image points that float32 holds EXACTLY (relative size (2, 1, 4) at t = (0.5, -0.25, 6): depths 4 and 8,
    # f = 512, integer pixels).  A float32-rounded image leaves the recovered rotation ~1e-7 rad from pi, where the
    # antisymmetric part of R still gives the axis to 1e-9 and rot_to_rvec's near-pi branch is a convenience; with an exact image
    # the walk ends within 1e-15 of pi, the antisymmetric part is rounding noise, and only that branch returns an axis.
    cam_int = np.array([512.0, 512.0, 256.0, 256.0])
    for fr in ("cv", "gl"):
        for name, D in (("0", np.eye(3)), ("pi about x", np.diag([1.0, -1.0, -1.0])), ("pi about y", np.diag([-1.0, 1.0, -1.0])),
                        ("pi about z", np.diag([-1.0, -1.0, 1.0]))):
            if fr == "cv" and name == "0":
                continue  # (the walk would end at a rotation vector of ~1e-17 or exactly 0: r / |r| is rounding there)
            i = b.add("%s integer pixels theta=%s" % (fr, name), (2.0, 1.0, 4.0), D if fr == "cv" else M_GL.T @ D, np.array([0.5, -0.25, 6.0]),
                      cam4=cam_int)
            assert np.array_equal(b.pts[i], np.round(b.pts[i]))
            frame.append(fr)
            theta.append(0.0 if name == "0" else np.pi)
    # face x = -w/2 (vertices 0-3) with the camera centre in its plane: X_cam = 0 for all four vertices
    valid = np.zeros(16, bool)
    valid[:8] = True
    cam = np.array([663.0, 663.0, 300.25, 395.0])
    fail = b.add("planar_init fails: face x=-w/2 edge-on", sc, np.eye(3), np.array([0.65, 0.2, 8.0]), cam4=cam, valid=valid)
    frame.append("none")
    theta.append(0.0)
    return b.done(frame=frame, theta=np.array(theta), planar_init_fails=fail)


# slot patterns (True = valid).  npts = 16: slot k is candidate k % 2 of vertex k // 2; npts = 8: slot k is vertex k.
def _slots(n, on):
    v = np.zeros(n, bool)
    v[list(on)] = True
    return v


VALIDITY_16 = {
    "odd slots": _slots(16, range(1, 16, 2)),
    "even slots": _slots(16, range(0, 16, 2)),
    "two vertices dropped": _slots(16, [k for k in range(16) if k // 2 not in (2, 5)]),
    "six on six vertices, odd slots": _slots(16, [1, 3, 5, 9, 11, 15]),
    "six on three vertices": _slots(16, [0, 1, 6, 7, 10, 11]),            # vertices 0, 3, 5
    "six on four vertices": _slots(16, [0, 1, 6, 7, 10, 12]),             # vertices 0, 3, 5, 6 (a tetrahedron)
    "one face twice plus one vertex": _slots(16, list(range(8)) + [13]),  # face x = -w/2 (vertices 0-3) + vertex 6
    "four non-coplanar": _slots(16, [0, 7, 10, 13]),                      # vertices 0, 3, 5, 6
}
VALIDITY_8 = {
    "seven valid": _slots(8, [0, 1, 2, 3, 4, 6, 7]),
    "six valid": _slots(8, [0, 1, 3, 4, 6, 7]),
    "four non-coplanar": _slots(8, [0, 3, 5, 6]),
}
DEGENERATE_PATTERNS = ("six on three vertices", "six on four vertices", "one face twice plus one vertex")
# Patterns whose correspondences do not determine the initialisation: three or four distinct points leave the homography /
# the DLT normal matrix with a null space of dimension 2 or more, five distinct points (a face and one vertex) leave the
# DLT's with dimension 2, and four points leave EPnP's 12 x 12 with dimension 4, of which its three linearisations use the
# first one, two and three basis vectors.  Which vector of such a space an eigen-solver returns is decided by rounding, and
# the pose (or "behind the camera") that follows from it is not a function of the data: the oracle's own answer changes
# from pose to None, or by more than 100 degrees, when ONE image coordinate moves by ONE float32 ulp
# (tests/test_pnp_edges_cpu.py: test_underdetermined_patterns_have_no_defined_answer asserts it for every pattern).  The GPU tests
# therefore compare these rows with the oracle in nothing; they assert a defined status, finite numbers and that the row
# is consistent with its own pose (``defined`` is False for them).
UNDERDETERMINED_PATTERNS = DEGENERATE_PATTERNS + ("four non-coplanar",)
VALIDITY_POSES = 4


def validity_patterns(npts, seed=103):
    """Each slot pattern on VALIDITY_POSES random poses, exact and with 1 px of noise (the same poses for every pattern)."""
    pats = VALIDITY_16 if npts == 16 else VALIDITY_8
    b = _Builder(npts)
    pattern = []
    for name, valid in pats.items():
        rng = np.random.RandomState(seed)
        for p in range(VALIDITY_POSES):
            sc = (rng.uniform(0.5, 2.0), 1.0, rng.uniform(0.5, 2.0))
            R, t = _pose(rng)
            for noise in (0.0, 1.0):
                b.add("%s / pose %d noise=%g" % (name, p, noise), sc, R, t, noise=noise, rng=rng, valid=valid)
                pattern.append(name)
    return b.done(pattern=pattern, defined=np.array([p not in UNDERDETERMINED_PATTERNS for p in pattern]))


def camera_and_placement(seed=104):
    """Anisotropic cameras, a principal point far from the image centre, a different camera on every row (every row's camera is
    the named one times 1 + 0.003 row), objects far off-axis (projections partly outside a 600 x 800 image, some coordinates
    negative), strong perspective (z = 1.6 for a cuboid of height 1), z = 200, needles and slabs.  Exact data everywhere,
    and 0.5 px of noise where a pose is still defined by the image (not at z = 200, where the cuboid is 3 px high)."""
    rng = np.random.RandomState(seed)
    b = _Builder(16)
    kind = []
    subs = [
        ("fx<fy", (400.0, 950.0, CAM0[2], CAM0[3]), None, (6.0, 12.0), None, True),
        ("fx>fy", (950.0, 400.0, CAM0[2], CAM0[3]), None, (6.0, 12.0), None, True),
        ("principal point (100,700)", (400.0, 950.0, 100.0, 700.0), None, (6.0, 12.0), None, True),
        ("off-axis t=(3.5,-4,8)", tuple(CAM0), (3.5, -4.0, 8.0), None, None, True),
        ("z=1.6", tuple(CAM0), (0.05, -0.03, 1.6), None, None, True),
        ("z=200", tuple(CAM0), (2.0, -3.0, 200.0), None, None, False),
        ("size (0.05,1,0.05)", tuple(CAM0), None, (6.0, 12.0), (0.05, 1.0, 0.05), False),
        ("size (20,1,20)", tuple(CAM0), None, (40.0, 60.0), (20.0, 1.0, 20.0), False),
    ]
    for name, cam, tfix, zr, size, noisy in subs:
        n_pose = 4 if noisy else 6
        for p in range(n_pose):
            R, t = _pose(rng, zr if zr else (6.0, 12.0))
            if tfix is not None:
                t = np.array(tfix)
            sc = size if size is not None else (rng.uniform(0.5, 2.0), 1.0, rng.uniform(0.5, 2.0))
            for noise in ((0.0, 0.5) if noisy else (0.0,)):
                row = len(b.names)
                c = np.array(cam) * np.array([1 + 0.003 * row, 1 - 0.002 * row, 1.0, 1.0]) + np.array([0, 0, 0.25 * row, -0.5 * row])
                b.add("%s / pose %d noise=%g" % (name, p, noise), sc, R, t, cam4=c, noise=noise, rng=rng)
                kind.append(name)
    return b.done(kind=kind)


USELESS_UNDERDETERMINED = ("scale[0]=scale[2]=0",)  # eight model points on a segment: no pose is defined (see UNDERDETERMINED_PATTERNS)
USELESS = ("good", "one coordinate NaN", "one coordinate +Inf", "one coordinate -Inf", "all points NaN", "scale[1]=0",
           "scale[0]=NaN", "scale=-scale", "scale[0]=scale[2]=0", "fx=0", "cx=NaN", "mirrored through the principal point", "u mirrored about the principal point")


def useless_inputs(seed=105):
    """One good row (16 points, 0.3 px of noise) and the same row with one thing changed (USELESS, in this order)."""
    rng = np.random.RandomState(seed)
    R, t = _pose(rng)
    sc = (1.4, 0.8, 0.6)  # (not normalised: scale = -scale must give the same ratios)
    b = _Builder(16)
    for name in USELESS:
        b.add(name, sc, R, t, noise=0.3, rng=np.random.RandomState(seed + 1), exact=False)
    c = b.done()
    n = {name: i for i, name in enumerate(USELESS)}
    c.pts[n["one coordinate NaN"], 5, 0] = np.nan
    c.pts[n["one coordinate +Inf"], 5, 1] = np.inf
    c.pts[n["one coordinate -Inf"], 5, 0] = -np.inf
    c.pts[n["all points NaN"]] = np.nan
    c.scale[n["scale[1]=0"], 1] = 0.0
    c.scale[n["scale[0]=NaN"], 0] = np.nan
    c.scale[n["scale=-scale"]] *= -1
    c.scale[n["scale[0]=scale[2]=0"], [0, 2]] = 0.0
    c.cam[n["fx=0"], 0] = 0.0
    c.cam[n["cx=NaN"], 2] = np.nan
    i = n["mirrored through the principal point"]
    c.pts[i] = (2 * c.cam[i, 2:4][None, :] - c.pts[i].astype(np.float64)).astype(np.float32)
    # (a point reflection of the image is a rotation by pi about the optical axis: R' = diag(-1, -1, 1) R is a proper pose in
    # front of the camera, which the oracle finds.  Mirroring u alone is a reflection: no rotation explains it, the DLT's
    # 3 x 3 block has a negative determinant, the sign fix turns t with it and the walk ends behind the camera.)
    i = n["u mirrored about the principal point"]
    c.pts[i, :, 0] = (2 * c.cam[i, 2] - c.pts[i, :, 0].astype(np.float64)).astype(np.float32)
    for k in range(len(USELESS)):  # a changed row has no generating pose to be compared with
        if k != n["good"]:
            c.R[k], c.t[k] = np.nan, np.nan
    c.index = n
    return c


def planar_rows(n, seed=106):
    """n rows with one cuboid face valid (both candidates of vertices 0-3): the homography start, 1 px of noise."""
    rng = np.random.RandomState(seed)
    b = _Builder(16)
    for i in range(n):
        R, t = _pose(rng)
        b.add("planar %d" % i, (rng.uniform(0.5, 2.0), 1.0, rng.uniform(0.5, 2.0)), R, t, noise=1.0, rng=rng, valid=_slots(16, range(8)))
    return b.done()


def five_point_rows(n, seed=107):
    """n rows with five valid points on five vertices: EPnP, 1 px of noise."""
    rng = np.random.RandomState(seed)
    b = _Builder(16)
    for i in range(n):
        R, t = _pose(rng)
        b.add("five points %d" % i, (rng.uniform(0.5, 2.0), 1.0, rng.uniform(0.5, 2.0)), R, t, noise=1.0, rng=rng,
              valid=_slots(16, [0, 2, 5, 9, 14]))
    return b.done()


def good_rows(n, npts=16, seed=108):
    """n well-posed rows of the suite's usual distribution (filler and neighbours for the batch-composition tests)."""
    rng = np.random.RandomState(seed)
    b = _Builder(npts)
    for i in range(n):
        R, t = _pose(rng)
        b.add("good %d" % i, (rng.uniform(0.5, 2.0), 1.0, rng.uniform(0.5, 2.0)), R, t, noise=0.5, rng=rng)
    return b.done()


def no_point_row(npts=16):
    b = _Builder(npts)
    b.add("no valid point", (1.0, 1.0, 1.0), np.eye(3), np.array([0.0, 0.0, 8.0]), valid=np.zeros(npts, bool))
    return b.done()


def concat(*cs):
    return SimpleNamespace(pts=np.concatenate([c.pts for c in cs]), scale=np.concatenate([c.scale for c in cs]),
                           cam=np.concatenate([c.cam for c in cs]), R=np.concatenate([c.R for c in cs]),
                           t=np.concatenate([c.t for c in cs]), exact=np.concatenate([c.exact for c in cs]),
                           names=sum([c.names for c in cs], []), npts=cs[0].npts)


def mixed_rows(npts):
    """About 40 rows (npts = 16; 14 for npts = 8) that cover every family and every way a row can end: fewer than 4 points
    (-1), failure (0), pose (1), behind the camera (2), and both rare branches (EPnP, planar) with and without a pose."""
    if npts == 8:
        v = validity_patterns(8)
        return concat(take(v, range(0, len(v.names), 2)), good_rows(1, 8), no_point_row(8))
    ps, sr, vp, cp, ui = planar_switch(), singular_rotation(), validity_patterns(16), camera_and_placement(), useless_inputs()
    one_face_once = take(vp, [0])
    one_face_once.pts[0, 8:] = INVALID
    one_face_once.pts[0, 0:8:2] = INVALID  # four coplanar points: EPnP without barycentric coordinates -> failure (0)
    one_face_once.names = ["four coplanar points"]
    return concat(take(ps, [12, 13, 14, 15, 44]), take(sr, [0, 7, 32, 34, 39, 63, 66, 69, 71]), take(vp, range(1, 64, 8)),
                  take(vp, [3 + 8 * k for k in (2, 4, 5, 6)]), one_face_once, take(cp, [1, 20, 33, 38, 44, 50]),
                  take(ui, [0, 1, 3, 4, 5, 7, 9, 11, 12]), planar_rows(1), five_point_rows(1), no_point_row())


FAMILIES = {"planar_switch": planar_switch, "singular_rotation": singular_rotation,
            "validity_patterns": lambda: validity_patterns(16), "validity_patterns_8": lambda: validity_patterns(8),
            "camera_and_placement": camera_and_placement}


# ----------------------------------------------------------------------------------------------------------------
# The reference side
# ----------------------------------------------------------------------------------------------------------------
def oracle_row(pts, scale, cam4, **lm):
    """oracle/pnp.solve_cuboid_pnp on one row as the device receives it (float32 points and sizes, widened).  Returns a record with
    ``kind`` = "pose" (+ every compared quantity, both frames), "none" (+ ``why``: few_points / solver_failed / behind_camera)
    or "undefined" (the oracle raised: the reference has no defined answer; + ``error``)."""
    why = []
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        try:
            s = opnp.solve_cuboid_pnp(pts.astype(np.float64), scale.astype(np.float64), Kmat(cam4), opencv_return=True, reject=why, **lm)
        except (np.linalg.LinAlgError, ValueError, ZeroDivisionError, FloatingPointError) as e:
            return SimpleNamespace(kind="undefined", error=type(e).__name__)
        if s is None:
            return SimpleNamespace(kind="none", why=why[0])
        # the OpenGL-frame outputs as solve_cuboid_pnp(opencv_return=False) forms them from the same (rvec, tvec)
        rvec_gl = opnp.matrix_to_rodrigues(M_GL @ opnp.rodrigues_to_matrix(s["rvec"]))
        return SimpleNamespace(kind="pose", rvec=s["rvec"], tvec=s["tvec"], proj=s["projected_points"], reproj=s["reproj_err"],
                               iters=s["iters"],
                               quat_cv=s["quaternion_xyzw"], loc_gl=M_GL @ s["tvec"], quat_gl=opnp.axis_angle_quat_xyzw(rvec_gl))


def oracle_rows(c, **lm):
    return [oracle_row(c.pts[i], c.scale[i], c.cam[i], **lm) for i in range(len(c.names))]


def geodesic_deg(Ra, Rb):
    return float(np.degrees(rotation_angle(Ra.T @ Rb)))


def quat_diff(qa, qb):
    """max |qa -+ qb| over the elements finite in both, sign chosen by their dot product; inf when the non-finite elements
    are not the same ones."""
    fa, fb = np.isfinite(qa), np.isfinite(qb)
    if not np.array_equal(fa, fb):
        return np.inf
    if not fa.any():
        return 0.0
    sgn = -1.0 if float(np.dot(qa[fa], qb[fa])) < 0 else 1.0
    return float(np.abs(qa[fa] - sgn * qb[fb]).max())


QUANTITIES = ("rot_deg", "t_rel", "proj_px", "reproj_px", "loc_rel", "quat_cv", "quat_gl")


def pose_diff(a, b):
    """The seven compared figures between two poses given as records with rvec, tvec, proj, reproj, quat_cv, loc_gl, quat_gl."""
    nt = np.linalg.norm(b.tvec)
    return {"rot_deg": geodesic_deg(opnp.rodrigues_to_matrix(a.rvec), opnp.rodrigues_to_matrix(b.rvec)),
            "t_rel": float(np.linalg.norm(a.tvec - b.tvec) / nt),
            "proj_px": float(np.abs(a.proj - b.proj).max()),
            "reproj_px": float(abs(a.reproj - b.reproj)),
            "loc_rel": float(np.linalg.norm(a.loc_gl - b.loc_gl) / nt),
            "quat_cv": quat_diff(a.quat_cv, b.quat_cv),
            "quat_gl": quat_diff(a.quat_gl, b.quat_gl)}


def device_pose(row):
    """One [40] row of cp_pnp_solve as the same record (layout: centerpose_hip.h)."""
    return SimpleNamespace(rvec=row[1:4], tvec=row[4:7], reproj=row[7], proj=row[8:24].reshape(8, 2), quat_cv=row[24:28],
                           loc_gl=row[28:31], quat_gl=row[31:35])


# The suite's existing limits (tests/test_gpu_parity.py: test_pnp_known_pose_and_vs_float64_oracle): 1e-3 deg, 1e-6 relative
# on tvec (and on the OpenGL location, which is a permutation of it), 1e-4 px on the projections (and on the RMS
# reprojection error, a mean of such differences), 1e-6 on quaternion elements.
BASE_LIMITS = {"rot_deg": 1e-3, "t_rel": 1e-6, "proj_px": 1e-4, "reproj_px": 1e-4, "loc_rel": 1e-6, "quat_cv": 1e-6, "quat_gl": 1e-6}


# Two runs whose RMS reprojection errors differ by more than this did not stop at the same minimum (a thin cuboid under noise
# has the planar pose ambiguity's second minimum: planar_switch row 61, 0.398 px from the generating pose against 1.301 px from
# the initialisation, 143 degrees apart); such a pair says nothing about how far apart two walks to ONE minimum stop.
SAME_MINIMUM_PX = 1e-2


def oracle_spread(c, rows=None):
    """How far two correct Levenberg-Marquardt solvers of the family's problems may end from each other, measured on the oracle
    ALONE: its answer against its own answer with max_iter = 40, and against its answer when started from the generating
    pose (rows that have one).  Returns {quantity: worst figure} over the rows where all runs have a pose."""
    worst = {q: 0.0 for q in QUANTITIES}
    for i in (range(len(c.names)) if rows is None else rows):
        if not getattr(c, "defined", np.ones(len(c.names), bool))[i]:
            continue
        a = oracle_row(c.pts[i], c.scale[i], c.cam[i])
        if a.kind != "pose":
            continue
        others = [oracle_row(c.pts[i], c.scale[i], c.cam[i], max_iter=40)]
        if np.isfinite(c.R[i]).all() and int((c.pts[i] > -5000).all(axis=1).sum()) >= 6:
            others.append(oracle_row(c.pts[i], c.scale[i], c.cam[i], init=(opnp.matrix_to_rodrigues(c.R[i]), c.t[i])))
        for o in others:
            if o.kind != "pose" or abs(o.reproj - a.reproj) > SAME_MINIMUM_PX:
                continue
            d = pose_diff(o, a)
            for q in QUANTITIES:
                worst[q] = max(worst[q], d[q])
    return worst


def limits_from_spread(spread):
    """The issue's rule: a limit stays at the suite's unless the oracle's own spread exceeds a tenth of it; then it is 10 x
    the spread."""
    return {q: (BASE_LIMITS[q] if spread[q] <= 0.1 * BASE_LIMITS[q] else 10.0 * spread[q]) for q in QUANTITIES}


def generating_distance(c, rows=None):
    """Worst distance of the ORACLE's pose from the generating pose over the exact rows (rotation in degrees, tvec relative):
    what float32 rounding of the image points alone costs a correct solver."""
    worst = {"rot_deg": 0.0, "t_rel": 0.0}
    for i in (range(len(c.names)) if rows is None else rows):
        if not (c.exact[i] and np.isfinite(c.R[i]).all() and getattr(c, "defined", np.ones(len(c.names), bool))[i]):
            continue
        a = oracle_row(c.pts[i], c.scale[i], c.cam[i])
        if a.kind == "pose":
            worst["rot_deg"] = max(worst["rot_deg"], geodesic_deg(opnp.rodrigues_to_matrix(a.rvec), c.R[i]))
            worst["t_rel"] = max(worst["t_rel"], float(np.linalg.norm(a.tvec - c.t[i]) / np.linalg.norm(c.t[i])))
    return worst


# ---- measured on the oracle alone (python -m tests.pnp_edge_cases; numpy 1.x / LAPACK of this project's environment) ----
# SPREAD_MEASURED: oracle vs oracle with max_iter = 40 and vs oracle started from the generating pose, worst over the family.
# Every figure is below a tenth of its base limit (rot 1e-4 deg, t 1e-7, proj 1e-5 px, ...), so by the rule above EVERY family
# keeps the suite's limits -- z = 200, the needles and slabs and the thin cuboids under noise included (the candidates for
# a wider limit did not need one: the walk converges quadratically and stops far inside FLT_EPSILON times the conditioning).
SPREAD_MEASURED = {
    "planar_switch": {"rot_deg": 2.2e-06, "t_rel": 8.6e-09, "proj_px": 4.6e-07, "reproj_px": 2.3e-09, "loc_rel": 8.6e-09, "quat_cv": 1.9e-08, "quat_gl": 1.7e-08},
    "singular_rotation": {"rot_deg": 5.6e-08, "t_rel": 2.0e-10, "proj_px": 7.0e-08, "reproj_px": 5.7e-11, "loc_rel": 2.0e-10, "quat_cv": 3.3e-10, "quat_gl": 7.5e-09},
    "validity_patterns": {"rot_deg": 2.9e-07, "t_rel": 5.5e-10, "proj_px": 2.3e-07, "reproj_px": 1.9e-11, "loc_rel": 5.5e-10, "quat_cv": 2.5e-09, "quat_gl": 2.0e-09},
    "validity_patterns_8": {"rot_deg": 1.3e-06, "t_rel": 1.7e-09, "proj_px": 8.6e-07, "reproj_px": 1.9e-11, "loc_rel": 1.7e-09, "quat_cv": 7.8e-09, "quat_gl": 6.5e-09},
    "camera_and_placement": {"rot_deg": 8.9e-07, "t_rel": 3.5e-09, "proj_px": 3.7e-07, "reproj_px": 3.0e-09, "loc_rel": 3.5e-09, "quat_cv": 6.6e-09, "quat_gl": 7.1e-09},
}
LIMITS = {fam: limits_from_spread(sp) for fam, sp in SPREAD_MEASURED.items()}  # == BASE_LIMITS for every family

# GENERATING_MEASURED: the oracle's own distance from the generating pose on exact (float32-rounded) image points.  The suite's
# limits for that comparison are 1e-3 deg and 1e-6 relative; the same rule gives 10 x the oracle's figure where it exceeds a
# tenth of them -- z = 200 (a cuboid 3 px high: float32 rounding of a pixel coordinate is 3e-5 px) and, for tvec, the thin cuboids.
GENERATING_MEASURED = {
    "planar_switch": {"rot_deg": 5.9e-05, "t_rel": 3.3e-07},
    "singular_rotation": {"rot_deg": 1.3e-05, "t_rel": 1.2e-07},
    "validity_patterns": {"rot_deg": 1.3e-05, "t_rel": 1.0e-07},
    "validity_patterns_8": {"rot_deg": 1.4e-05, "t_rel": 1.1e-07},
    "camera_and_placement": {"rot_deg": 3.2e-04, "t_rel": 1.5e-06},
}
GENERATING_LIMITS = {fam: {q: (BASE_LIMITS[q] if m[q] <= 0.1 * BASE_LIMITS[q] else 10.0 * m[q]) for q in m}
                     for fam, m in GENERATING_MEASURED.items()}


if __name__ == "__main__":
    import time

    for fam, make in FAMILIES.items():
        t0 = time.time()
        sp = oracle_spread(make())
        print(fam, "%.1f s" % (time.time() - t0))
        for q in QUANTITIES:
            print("    %-10s spread %.3e -> limit %.3e" % (q, sp[q], limits_from_spread(sp)[q]))
        print("    oracle vs generating pose:", generating_distance(make()))
