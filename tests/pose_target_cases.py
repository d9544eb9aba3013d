"""Seeded ObjectPose target cases shared by tools/make_pose_target_goldens.py and the tests: synthetic annotation JSON
(camera, poses, boxes, projected cuboids, edge cases written into the projected cuboid) and, where the reference tree is
present, a runner of its own ObjectPoseDataset.__getitem__ on them.  The golden file stores the packed records and the
reference's outputs, so the GPU tests read nothing but the file."""
import json
import os
import sys
import tempfile
import types
from types import SimpleNamespace

import numpy as np

from centerpose_amd.pose_targets import pack_annotations
from tests import pose_targets_ref as R

REF = os.environ.get("CENTERPOSE_REFERENCE", "/root/reference")

BASE_OPT = dict(c="chair", mug=False, num_symmetry=12, input_res=256, output_res=64, flip=0.5, aug_rot=0.0, rotate=0.0,
                not_rand_crop=True, scale=0.1, shift=0.02, new_data_augmentation=False, no_color_aug=True,
                tracking_task=False, center_3D=False, mse_loss=False, hm_gauss=2, obj_scale=True,
                use_absolute_scale=False, obj_scale_uncertainty=False, dense_hp=False, hps_uncertainty=False,
                pre_img=False, pre_hm=False, pre_hm_hp=False, tracking=False, tracking_hp=False, reg_bbox=True,
                reg_offset=True, hm_hp=True, reg_hp_offset=True, debug=0, flip_idx=[[1, 5], [3, 7], [2, 6], [4, 8]],
                heads={"hm": 1, "wh": 2, "hps": 16, "reg": 2, "hm_hp": 8, "hp_offset": 2, "scale": 3})

# object specs: (symmetric key or None, kind); kinds other than "pose" rewrite the projected cuboid of a
# non-symmetric object (the variant projection does not read it)
#   pose        a posed box whose cuboid is its projection        edge    near the image border, partly out
#   corner_neg  corner 1 at x = -0.5: stored 0, not visible        out4    centre out of frame, 4 corners visible: dropped
#   out5        centre out of frame, 5 corners visible: kept       flat    corners far right of the frame: zero-area box
#   negy        scale[1] < 0 (the relative scale's sign)            twin    at the previous object's centre (overlap)
CASES = {
    # name: (seed, opt overrides, image (w, h), object specs)
    "chair_carry": (1, dict(c="chair"), (640, 480), [("True", "pose"), (None, "pose"), ("False", "pose"), (None, "edge"),
                                                     ("True", "twin")]),
    "bottle_s12": (2, dict(c="bottle", num_symmetry=12, not_rand_crop=False, scale=0.4, shift=0.05), (480, 640), [(None, "pose"), ("True", "pose"), ("False", "pose")]),
    "camera_s1": (3, dict(c="camera", scale=0.0, shift=0.0), (640, 480), [(None, "pose"), (None, "corner_neg"), (None, "out4"), (None, "out5"),
                                                    (None, "negy")]),
    "flip_on": (4, dict(c="chair", flip=1.0), (640, 480), [("True", "pose"), ("False", "corner_neg"), ("False", "edge")]),
    "flip_off": (5, dict(c="chair", flip=0.0), (640, 480), [("True", "pose"), ("False", "corner_neg"), ("False", "edge")]),
    "rot_flat": (6, dict(c="camera", aug_rot=1.0, rotate=30.0), (640, 480), [(None, "pose"), (None, "flat"),
                                                                             (None, "out5")]),
    "center3d": (7, dict(c="chair", center_3D=True, flip=1.0), (640, 480), [("True", "pose"), ("False", "edge"),
                                                                           ("False", "out5"), ("True", "edge")]),
    "scale_abs_unc": (8, dict(c="cup", num_symmetry=6, use_absolute_scale=True, hps_uncertainty=True,
                              obj_scale_uncertainty=True), (640, 480), [(None, "pose"), ("False", "negy"), ("True", "twin")]),
    "many": (9, dict(c="camera", output_res=96, input_res=384), (640, 480), [(None, "pose")] * 9 + [(None, "twin")] * 3),
}


def make_opt(over=None, **kw):
    o = dict(BASE_OPT)
    o.update(over or {})
    o.update(kw)
    return SimpleNamespace(**o)


def _quat_matrix(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _project(P, X, width, height):
    p = P @ np.append(X, 1.0)
    p = p[:3] / p[3]
    return [(p[1] + 1) / 2 * width, (p[0] + 1) / 2 * height]  # (x, y) in pixels, as the reference's viewport


def synth_annotations(rng, specs, width, height):
    """Annotation JSON (as a dict) for an image of width x height with one object per spec."""
    f = 1.5
    P = np.array([[f * 480 / height, 0, 0, 0], [0, f * 480 / width, 0, 0], [0, 0, -1.002, -0.2002], [0, 0, -1, 0]])
    objects, prev = [], None
    for sym, kind in specs:
        Z = -rng.uniform(1.5, 4.0)
        if kind == "twin" and prev is not None:
            px, py = prev[0] + rng.uniform(-6, 6), prev[1] + rng.uniform(-6, 6)
        elif kind == "edge":
            px, py = (rng.uniform(-20, 20) if rng.random() < 0.5 else width + rng.uniform(-20, 20)), rng.uniform(0, height)
        else:
            px, py = rng.uniform(0.15, 0.85) * width, rng.uniform(0.15, 0.85) * height
        prev = (px, py)
        X = np.array([(2 * py / height - 1) * -Z / P[0, 0], (2 * px / width - 1) * -Z / P[1, 1], Z])
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        dims = rng.uniform(0.1, 0.35, 3)
        Rm = _quat_matrix(q)
        corners = [X] + [X + Rm @ (np.array([sx, sy, sz]) * dims / 2) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
        cub = [_project(P, c, width, height) for c in corners]
        if kind == "corner_neg":
            cub[1][0] = -0.5
        elif kind in ("out4", "out5"):
            nin = 4 if kind == "out4" else 5
            cub[0] = [width + 3.0, height / 2]
            for i in range(8):
                cub[1 + i] = [width - 8.0 - i if i < nin else width + 6.0 + i, height / 2 - 20 + 5 * i]
        elif kind == "flat":
            cub = [[width / 2, height / 2]] + [[3.0 * width + i, height / 4 + 30 * i] for i in range(8)]
        scale = dims / dims[1] * (np.array([1.0, -1.0, 1.0]) if kind == "negy" else 1.0)
        o = {"projected_cuboid": [[float(a), float(b)] for a, b in cub], "quaternion_xyzw": [float(v) for v in q],
             "location": [float(v) for v in X], "keypoints_3d": [[float(v) for v in c] for c in corners],
             "scale": [float(v) for v in scale]}
        if sym is not None:
            o["symmetric"] = sym
        objects.append(o)
    return {"camera_data": {"camera_projection_matrix": P.tolist()}, "objects": objects}


def near_integer(recs, S, tol=1e-6):
    """True when a truncated value of a variant projection lies within tol of an integer (a case to re-draw)."""
    img, objs = recs["pt_image"], recs["pt_objects"]
    for k in range(int(img[R.I["num_objs"]])):
        n = int(objs[k, R.O["nsym"]])
        if n == 1:
            continue
        for s in range(n):
            _, raw = R.project(img, objs[k], s, S)
            if any(abs(v - round(v)) < tol for pt in raw for v in pt):
                return True
    return False


def annotations(name):
    """(opt, anns, width, height, seed) of case `name`; the annotation seed is the first one whose variant projections
    keep every truncated value at least 1e-6 away from an integer, for any affine (the projection does not depend on
    it)."""
    seed, over, (w, h), specs = CASES[name]
    opt = make_opt(over)
    from centerpose_amd.pose_targets import num_symmetry
    S = num_symmetry(opt)
    for sub in range(100):
        anns = synth_annotations(np.random.default_rng([seed, sub]), specs, w, h)
        recs = pack_annotations(anns, np.eye(2, 3), w, h, False, 0.0, opt)
        if not near_integer(recs, S):
            return opt, anns, w, h, seed * 1000 + sub
    raise RuntimeError("no clean draw for case %s" % name)


# ---- the reference's own __getitem__ ----

def _cv2_stub(sizes):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1

    def imread(path):
        h, w = sizes[path]
        return np.zeros((h, w, 3), np.uint8)

    def getAffineTransform(src, dst):  # the 3-point solve: dst_i = M [src_i, 1]
        src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
        A = np.hstack([src, np.ones((3, 1))])
        return np.linalg.solve(A, dst).T.copy()

    def warpAffine(img, M, dsize, flags=None):
        return np.zeros((dsize[1], dsize[0]) + img.shape[2:], img.dtype)

    cv2.imread, cv2.getAffineTransform, cv2.warpAffine = imread, getAffineTransform, warpAffine
    return cv2


def reference_available():
    return os.path.isfile(os.path.join(REF, "src", "lib", "datasets", "dataset_combined.py"))


def run_reference(opt, anns, width, height, seed):
    """The reference's ObjectPoseDataset.__getitem__ (unmodified) on one synthetic image: returns (ret, captured) with
    captured = {trans_output_rot, rot, flipped, width, height} read from its frame.  Stubs: cv2 (imread gives a zero
    image of the annotation's size, getAffineTransform a 3-point solve, warpAffine zeros), albumentations and
    lib.detectors.detector_factory; they, the reference's modules and its path entry are removed afterwards."""
    src = os.path.join(REF, "src")
    before, path = set(sys.modules), list(sys.path)
    sizes = {}
    try:
        sys.modules["cv2"] = _cv2_stub(sizes)
        sys.modules["albumentations"] = types.ModuleType("albumentations")
        df = types.ModuleType("lib.detectors.detector_factory")
        df.detector_factory = {}
        sys.modules["lib.detectors.detector_factory"] = df
        sys.path.insert(0, src)
        from lib.datasets.dataset_combined import ObjectPoseDataset  # noqa: E402

        with tempfile.TemporaryDirectory() as tmp:
            jpath, ipath = os.path.join(tmp, "0.json"), os.path.join(tmp, "0.png")
            with open(jpath, "w") as fh:
                json.dump(anns, fh)
            sizes[ipath] = (height, width)
            ds = ObjectPoseDataset.__new__(ObjectPoseDataset)
            ds.opt, ds.split, ds.max_objs = opt, "train", 10
            ds.images = [(ipath, "v0", "0", jpath)]
            ds._data_rng = np.random.RandomState(123)
            ds._eig_val = np.array([0.2141788, 0.01817699, 0.00341571], dtype=np.float32)
            ds._eig_vec = np.array([[-0.58752847, -0.69563484, 0.41340352], [-0.5832747, 0.00994535, -0.81221408],
                                    [-0.56089297, 0.71832671, 0.41158938]], dtype=np.float32)
            code = ObjectPoseDataset.__getitem__.__code__
            cap = {}

            def prof(frame, event, arg):
                if event == "return" and frame.f_code is code:
                    loc = frame.f_locals
                    cap.update({k: loc.get(k) for k in ("trans_output_rot", "rot", "flipped", "width", "height")})

            np.random.seed(seed % (2 ** 32))
            sys.setprofile(prof)
            try:
                ret = ds[0]
            finally:
                sys.setprofile(None)
    finally:
        for name in set(sys.modules) - before:
            del sys.modules[name]
        sys.path[:] = path
    return ret, cap


def reference_case(opt, anns, width, height, seed):
    """(records, reference ret) of one synthetic image: the reference's run and the packed records of the same draw."""
    ret, cap = run_reference(opt, anns, width, height, seed)
    recs = pack_annotations(anns, cap["trans_output_rot"], cap["width"], cap["height"], cap["flipped"], cap["rot"], opt)
    return recs, ret


def random_case(seed, category="chair", n_obj=4, **over):
    """A freshly seeded case for the live comparison: random symmetry keys, edge cases, flip / rotation / centre and
    scale options."""
    rng = np.random.default_rng(seed)
    kinds = ["pose", "pose", "edge", "twin", "corner_neg", "out4", "out5", "negy", "flat"]
    syms = ["True", "False", None] if category != "camera" else [None]
    opt = make_opt(dict(c=category, num_symmetry=int(rng.choice([4, 6, 12])), flip=0.5, aug_rot=0.5, rotate=20.0,
                        not_rand_crop=bool(rng.random() < 0.5), scale=0.4, shift=0.05,
                        center_3D=bool(rng.random() < 0.5), use_absolute_scale=bool(rng.random() < 0.5),
                        hps_uncertainty=True, obj_scale_uncertainty=True), **over)
    from centerpose_amd.pose_targets import num_symmetry
    S = num_symmetry(opt)
    specs = [(syms[int(rng.integers(len(syms)))], kinds[int(rng.integers(len(kinds)))]) for _ in range(n_obj)]
    w, h = (640, 480) if rng.random() < 0.5 else (480, 640)
    for sub in range(100):
        anns = synth_annotations(np.random.default_rng([seed, sub]), specs, w, h)
        recs = pack_annotations(anns, np.eye(2, 3), w, h, False, 0.0, opt)
        if not near_integer(recs, S):
            return opt, anns, w, h, seed * 1000 + sub
    raise RuntimeError("no clean draw for random case %d" % seed)
