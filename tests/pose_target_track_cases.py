"""Seeded two-frame cases of the tracking task's targets, shared by tools/make_pose_target_track_goldens.py and the tests:
synthetic annotation JSON for a current and a previous frame (tests/pose_target_cases.py's objects, with the 'name' and
'mug' keys, the previous frame a shifted copy with objects repeated, dropped or renamed), the packed random draws with
the edits that force each case's events, and, where the reference tree is present, a runner of its own unmodified
ObjectPoseDataset.__getitem__ that consumes exactly those draws.  The golden file stores the packed records and the
reference's outputs, so the GPU tests read nothing but the file."""
import copy
import json
import os
import sys
import tempfile
import types

import numpy as np

from centerpose_amd import hip
from centerpose_amd.pose_targets import num_symmetry
from centerpose_amd.pose_targets_track import draw_track_noise, pack_track_annotations
from tests import pose_target_cases as PC
from tests import pose_targets_track_ref as TR

D = hip.PTK_DRAW
TRACK_OPT = dict(tracking_task=True, pre_img=True, pre_hm=True, pre_hm_hp=True, tracking=True, tracking_hp=True,
                 input_w=256, input_h=256, down_ratio=4, max_frame_dist=3, same_aug_pre=False,
                 data_generation_mode_ratio=0, tracking_label_mode=1, hm_heat_random=True, hm_hp_heat_random=True,
                 hm_disturb=0.05, lost_disturb=0.4, fp_disturb=0.1, hm_hp_disturb=0.02, hp_lost_disturb=0.2,
                 hp_fp_disturb=0.1,
                 heads={"hm": 1, "wh": 2, "hps": 16, "reg": 2, "hm_hp": 8, "hp_offset": 2, "scale": 3, "tracking": 2,
                        "tracking_hp": 16})

# edits of the draws, applied in order (object = index in the previous frame):
#   ("keep", o)          the centre is not lost and not a false positive, small noise
#   ("lost", o)          the centre's lost uniform is 0: conf == 0
#   ("fp", o)            the centre's false-positive uniform is 0
#   ("jlost", o, j)      joint j's lost uniform is 0: conf_hp == 0        ("jfp", o, j)  its false-positive uniform is 0
#   ("leave", o)         the centre's noise carries it out of the input (needs the geometry: second pass)
#   ("clip", o, near)    one in-frame joint of the object lands beside the map, its window still overlapping (near) or not
#                        (second pass)
#   ("nofp",)            every false-positive uniform is 1        ("allfp",)  every one is 0, nothing is lost
CASES = {
    # name: (seed, opt overrides, image (w, h), current specs, previous = [(current index, name or None, mug)], edits)
    "chair_filter": (11, dict(c="chair"), (640, 480),
                     [("True", "pose"), ("True", "pose"), ("False", "pose"), (None, "pose"), ("True", "pose")],
                     [(0, None, False), (1, None, False), (2, None, False), (3, None, False), (4, None, False)],
                     [("keep", 0), ("fp", 0), ("jfp", 0, 2), ("lost", 1), ("keep", 2), ("jlost", 2, 3), ("keep", 3),
                      ("keep", 4)]),
    "label0_plain": (12, dict(c="camera", tracking_label_mode=0, hm_heat_random=False, hm_hp_heat_random=False),
                     (640, 480), [(None, "pose")] * 4,
                     [(0, None, False), (1, None, False), (2, None, False), (3, None, False)],
                     [("lost", 0), ("keep", 1), ("jlost", 1, 1), ("fp", 1), ("keep", 2), ("jfp", 2, 0), ("keep", 3)]),
    "leave_clip": (13, dict(c="camera", hm_disturb=2.0, hm_hp_disturb=2.0), (640, 480), [(None, "pose")] * 4,
                   [(0, None, False), (1, None, False), (2, None, False), (3, None, False)],
                   [("keep", 0), ("keep", 1), ("keep", 2), ("keep", 3), ("leave", 0), ("clip", 1, True),
                    ("clip", 2, False)]),
    "out_flip_twice": (14, dict(c="camera", flip=1.0, tracking_label_mode=0), (640, 480),
                       [(None, "pose"), (None, "out4"), (None, "out5"), (None, "pose")],
                       [(3, "obj_0", False), (0, None, False), (1, None, False), (2, None, False)],
                       [("keep", 0), ("keep", 1), ("keep", 2), ("keep", 3)]),
    "rot_flat": (15, dict(c="camera", aug_rot=1.0, rotate=30.0, flip=0.0), (640, 480),
                 [(None, "pose"), (None, "flat"), (None, "pose")], [(0, None, False), (1, None, False), (2, None, False)],
                 [("keep", 0), ("keep", 1), ("keep", 2), ("jlost", 0, 0)]),
    "center3d": (16, dict(c="chair", center_3D=True, flip=1.0), (640, 480),
                 [("True", "pose"), ("False", "pose"), ("False", "edge"), ("True", "pose")],
                 [(0, None, False), (1, None, False), (2, None, False), (3, None, False)],
                 [("keep", 0), ("fp", 0), ("keep", 1), ("lost", 3), ("jfp", 1, 4)]),
    "cup_mug_pre": (17, dict(c="cup", mug=False, num_symmetry=6), (640, 480),
                    [(None, "pose"), ("True", "pose"), ("False", "pose")],
                    [(0, None, True), (1, None, False), (2, None, True), (1, "obj_7", False)],
                    [("keep", 1), ("keep", 3)]),
    "cup_mug_cur": (18, dict(c="cup", mug=False, num_symmetry=6), (640, 480), [(None, "pose"), ("False", "pose")],
                    [(0, None, False), (1, None, True)], [("keep", 0)]),
    "big": (19, dict(c="camera", input_res=384, input_w=384, input_h=384, output_res=96, not_rand_crop=False, scale=0.4,
                     shift=0.05), (480, 640), [(None, "pose")] * 6 + [(None, "twin"), (None, "edge")],
            [(k, None, False) for k in range(8)], []),
}


def make_opt(over=None, **kw):
    o = dict(TRACK_OPT)
    o.update(over or {})
    o.update(kw)
    return PC.make_opt(o)


def name_objects(anns, mug=False):
    for k, o in enumerate(anns["objects"]):
        o["name"] = "obj_%d" % k
        o["mug"] = mug
    return anns


def previous_frame(rng, anns, pre_spec):
    """The previous frame's annotations: for each (k, name, mug) a copy of current object k moved by a few pixels (the
    cuboid) and centimetres (the pose the variant projection reads)."""
    objs = []
    for k, name, mug in pre_spec:
        o = copy.deepcopy(anns["objects"][k])
        d2, d3 = rng.uniform(-8, 8, 2), rng.normal(0, 0.02, 3)
        o["projected_cuboid"] = [[x + d2[0], y + d2[1]] for x, y in o["projected_cuboid"]]
        o["location"] = [float(a + b) for a, b in zip(o["location"], d3)]
        o["keypoints_3d"] = [[float(a + b) for a, b in zip(p, d3)] for p in o["keypoints_3d"]]
        if name is not None:
            o["name"] = name
        o["mug"] = mug
        objs.append(o)
    return {"camera_data": copy.deepcopy(anns["camera_data"]), "objects": objs}


def _joint(o, j, slot):
    return o, D["joints"] + D["joint_stride"] * j + D[slot]


def apply_edits(draws, edits, geometry=None):
    """``geometry``: {object: restatement result with zero noise} for the edits that need it (skipped without)."""
    d = draws.copy()
    for e in edits:
        kind, o = e[0], (e[1] if len(e) > 1 else None)
        if kind == "keep":
            d[o, D["ct_lost"]], d[o, D["ct_fp"]] = 0.99, 0.99
            d[o, D["ct_noise"]:D["ct_noise"] + 2] *= 0.02
        elif kind == "lost":
            d[o, D["ct_lost"]] = 0.0
        elif kind == "fp":
            d[o, D["ct_fp"]] = 0.0
        elif kind == "jlost":
            d[_joint(o, e[2], "j_lost")] = 0.0
        elif kind == "jfp":
            d[_joint(o, e[2], "j_fp")] = 0.0
        elif kind == "nofp":
            d[:, D["ct_fp"]] = 1.0
            d[:, D["joints"] + D["j_fp"]:hip.PTK_NUM_DRAWS:D["joint_stride"]] = 1.0
        elif kind == "allfp":
            d[:, D["ct_fp"]], d[:, D["ct_lost"]] = 0.0, 0.99
            d[:, D["joints"] + D["j_fp"]:hip.PTK_NUM_DRAWS:D["joint_stride"]] = 0.0
            d[:, D["joints"] + D["j_lost"]:hip.PTK_NUM_DRAWS:D["joint_stride"]] = 0.99
        elif geometry is not None and kind == "leave":
            (w, h, ct0), op = geometry[o]["geom"], geometry["op"]
            n = (op.input_w + 2 - ct0[0]) / (op.hm_disturb * w)
            if abs(n) > 3:
                n = (-3 - ct0[0]) / (op.hm_disturb * w)
            assert abs(n) <= 3, ("leave", o, n)  # inside truncnorm(-3, 3)'s support
            d[o, D["ct_noise"]] = n
        elif geometry is not None and kind == "clip":
            g, op = geometry[o], geometry["op"]
            # the joint and the side (left or right of the map) that need the smallest noise
            left, right = (-2, op.input_w + 1) if e[2] else (-(g["radius"] + 6), op.input_w + g["radius"] + 5)
            _, n, j = min((abs(v), v, jj) for v, jj in (
                ((t + (0.5 if t > 0 else -0.5) - x) / (op.hm_hp_disturb * g["geom"][0]), jj)
                for jj, (x, _) in g["gt"].items() for t in (left, right)))
            assert abs(n) <= 3 and g["radius"] >= 3, ("clip", o, n, g["radius"])  # inside truncnorm(-3, 3)'s support
            d[_joint(o, j, "j_noise")] = n
            d[_joint(o, j, "j_lost")], d[_joint(o, j, "j_fp")] = 0.99, 0.99
    return d


def _clean(recs, S):
    """No truncated value of a variant projection, in either frame, lies within 1e-6 of an integer (every variant of a
    previous object is checked, whichever the draw chooses)."""
    img = recs["pt_image"].copy()
    objs = np.concatenate([recs["pt_objects"], recs["ptk_pre_objects"][:, :hip.PT_OBJ_STRIDE]])
    img[hip.PT_IMG["num_objs"]] = len(objs)  # unused slots have a variant count of 0: nothing to project
    return not PC.near_integer({"pt_image": img, "pt_objects": objs}, S)


def annotations(name):
    """(opt, anns, anns_pre, width, height, seed, draws before the geometric edits) of case ``name``."""
    seed, over, (w, h), specs, pre_spec, edits = CASES[name]
    opt = make_opt(over)
    S = num_symmetry(opt)
    for sub in range(100):
        rng = np.random.default_rng([seed, sub])
        anns = name_objects(PC.synth_annotations(rng, specs, w, h))
        pre = previous_frame(rng, anns, pre_spec)
        draws = apply_edits(draw_track_noise(rng, len(pre["objects"])), edits)
        recs = pack_track_annotations(anns, pre, np.eye(2, 3), np.eye(2, 3), w, h, False, 0.0, opt, draws)
        if _clean(recs, S):
            return opt, anns, pre, w, h, seed * 1000 + sub, draws
    raise RuntimeError("no clean draw for case %s" % name)


# ---- the reference's own __getitem__, fed the packed draws ----

# line of the call in datasets/dataset_combined.py -> the slot it reads (the file is read-only: the numbers are fixed)
_RANDOM = {730: ("ct", "ct_lost"), 733: ("ct", "ct_heat"), 929: ("ct", "ct_fp"), 814: ("j", "j_lost"), 878: ("j", "j_fp")}
_RANDN = {932: ("ct", "ct_fp_noise", 0), 933: ("ct", "ct_fp_noise", 1), 881: ("j", "j_fp_noise", 0),
          882: ("j", "j_fp_noise", 1)}
_UNIFORM = {937: ("ct", "ct_fp_peak"), 887: ("j", "j_fp_peak"), 888: ("j", "j_fp_peak")}
_TRUNCNORM = {715: ("ct", "ct_noise"), 808: ("j", "j_noise")}
_CHOICE = 578


class _Shims:
    """np.random.random / randn / uniform / choice and stats.truncnorm(...).rvs for the reference's module: each looks at
    its caller's frame and returns the packed slot for that line, idx_obj and j; any other line falls through to the real
    generator (the frame choice at 424, the mode draw at 465, _get_aug_param, flip)."""

    def __init__(self, draws):
        self.draws, self.used = draws, set()

    def slot(self, frame, where, name, off=0):
        o = frame.f_locals["idx_obj"]
        at = D[name] + off if where == "ct" else D["joints"] + D["joint_stride"] * frame.f_locals["j"] + D[name] + off
        self.used.add((o, at))
        return float(self.draws[o, at])

    def install(self, mod):
        shims = self

        class Random:
            def __getattr__(self, n):
                return getattr(np.random, n)

            def random(self, *a):
                f = sys._getframe(1)
                return shims.slot(f, *_RANDOM[f.f_lineno]) if f.f_lineno in _RANDOM else np.random.random(*a)

            def randn(self, *a):
                f = sys._getframe(1)
                return shims.slot(f, *_RANDN[f.f_lineno]) if f.f_lineno in _RANDN else np.random.randn(*a)

            def uniform(self, *a):
                f = sys._getframe(1)
                return shims.slot(f, *_UNIFORM[f.f_lineno]) if f.f_lineno in _UNIFORM else np.random.uniform(*a)

            def choice(self, a, *r):
                f = sys._getframe(1)
                if f.f_lineno != _CHOICE:
                    return np.random.choice(a, *r)
                return min(int(shims.draws[f.f_locals["idx_obj"], hip.PTK_NUM_DRAWS] * a), a - 1)

        class Np:
            random = Random()

            def __getattr__(self, n):
                return getattr(np, n)

        class TruncNorm:
            def rvs(self, n):
                f = sys._getframe(1)
                where, name = _TRUNCNORM[f.f_lineno]
                return np.array([shims.slot(f, where, name, i) for i in range(n)])

        class Stats:
            @staticmethod
            def truncnorm(a, b, loc=0, scale=1):
                assert (a, b, loc, scale) == (-3, 3, 0, 1)
                return TruncNorm()

        mod.np, mod.stats = Np(), Stats()


def run_reference(opt, anns, anns_pre, width, height, seed, draws):
    """The reference's ObjectPoseDataset.__getitem__ (unmodified) on one synthetic pair of frames with the noise read
    from ``draws``: returns (ret, captured) with captured = {trans_output_rot, trans_input_pre, rot, flipped, width,
    height} read from its frame.  Stubs as pose_target_cases.run_reference, plus a one-video ds.videos that holds the
    previous frame only."""
    src = os.path.join(PC.REF, "src")
    before, path = set(sys.modules), list(sys.path)
    sizes = {}
    try:
        sys.modules["cv2"] = PC._cv2_stub(sizes)
        sys.modules["albumentations"] = types.ModuleType("albumentations")
        df = types.ModuleType("lib.detectors.detector_factory")
        df.detector_factory = {}
        sys.modules["lib.detectors.detector_factory"] = df
        sys.path.insert(0, src)
        import lib.datasets.dataset_combined as mod  # noqa: E402

        ObjectPoseDataset = mod.ObjectPoseDataset
        _Shims(draws).install(mod)
        with tempfile.TemporaryDirectory() as tmp:
            paths = []
            for i, a in enumerate((anns, anns_pre)):
                jpath, ipath = os.path.join(tmp, "%d.json" % i), os.path.join(tmp, "%d.png" % i)
                with open(jpath, "w") as fh:
                    json.dump(a, fh)
                sizes[ipath] = (height, width)
                paths.append((ipath, "v0", str(i), jpath))
            ds = ObjectPoseDataset.__new__(ObjectPoseDataset)
            ds.opt, ds.split, ds.max_objs = opt, "train", 10
            ds.images = [paths[0]]
            ds.videos = {"v0": [paths[1]]}
            ds._data_rng = np.random.RandomState(123)
            ds._eig_val = np.array([0.2141788, 0.01817699, 0.00341571], dtype=np.float32)
            ds._eig_vec = np.array([[-0.58752847, -0.69563484, 0.41340352], [-0.5832747, 0.00994535, -0.81221408],
                                    [-0.56089297, 0.71832671, 0.41158938]], dtype=np.float32)
            code = ObjectPoseDataset.__getitem__.__code__
            cap = {}

            def prof(frame, event, arg):
                if event == "return" and frame.f_code is code:
                    loc = frame.f_locals
                    cap.update({k: loc.get(k) for k in ("trans_output_rot", "trans_input_pre", "rot", "flipped", "width",
                                                        "height")})

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


def pack(opt, anns, anns_pre, cap, draws):
    return pack_track_annotations(anns, anns_pre, cap["trans_output_rot"], cap["trans_input_pre"], cap["width"],
                                  cap["height"], cap["flipped"], cap["rot"], opt, draws)


def reference_case(opt, anns, anns_pre, width, height, seed, draws, edits=()):
    """(records, reference ret) of one pair of frames.  The affines come from the real generator, which the shimmed
    draws do not advance, so a first run yields the geometry that the 'leave' / 'clip' edits need and a second run with
    the edited draws has the same affines."""
    if any(e[0] in ("leave", "clip") for e in edits):
        _, cap = run_reference(opt, anns, anns_pre, width, height, seed, draws)
        zero = draws.copy()
        zero[:, :hip.PTK_NUM_DRAWS] = 0.0
        zero[:, D["ct_lost"]] = 0.99
        recs = pack(opt, anns, anns_pre, cap, zero)
        op = TR.options(opt)
        geo = TR.image_targets(recs, num_symmetry(opt), opt.output_res, op, opt.use_absolute_scale)["pre"]
        geometry = dict(enumerate(geo))
        geometry["op"] = op
        draws = apply_edits(draws, [e for e in edits if e[0] in ("leave", "clip")], geometry)
    ret, cap = run_reference(opt, anns, anns_pre, width, height, seed, draws)
    return pack(opt, anns, anns_pre, cap, draws), ret


def golden_case(name):
    opt, anns, pre, w, h, seed, draws = annotations(name)
    return (opt,) + reference_case(opt, anns, pre, w, h, seed, draws, CASES[name][5])


def random_case(seed, **over):
    """A freshly seeded pair of frames for the live comparison: random categories, symmetry keys, edge kinds, options,
    and unedited draws."""
    rng = np.random.default_rng(seed)
    cat = ("chair", "bottle", "camera", "cup")[seed % 4]
    kinds = ["pose", "pose", "pose", "edge", "twin", "corner_neg", "out4", "out5", "negy", "flat"]
    syms = ["True", "False", None] if cat != "camera" else [None]
    opt = make_opt(dict(c=cat, mug=False, num_symmetry=int(rng.choice([4, 6, 12])), flip=0.5, aug_rot=0.5, rotate=20.0,
                        not_rand_crop=bool(rng.random() < 0.5), scale=0.4, shift=0.05, center_3D=bool(rng.random() < 0.5),
                        use_absolute_scale=bool(rng.random() < 0.5), hps_uncertainty=True, obj_scale_uncertainty=True,
                        tracking_label_mode=int(rng.integers(2)), hm_heat_random=bool(rng.random() < 0.5),
                        hm_hp_heat_random=bool(rng.random() < 0.5), same_aug_pre=bool(rng.random() < 0.3),
                        hm_disturb=float(rng.choice([0.05, 0.5])), hm_hp_disturb=float(rng.choice([0.02, 0.5])),
                        pre_hm=bool(rng.random() < 0.8), pre_hm_hp=bool(rng.random() < 0.8)), **over)
    S = num_symmetry(opt)
    n = int(rng.integers(2, 8))
    specs = [(syms[int(rng.integers(len(syms)))], kinds[int(rng.integers(len(kinds)))]) for _ in range(n)]
    w, h = (640, 480) if rng.random() < 0.5 else (480, 640)
    pre_spec = [(k, None if rng.random() < 0.8 else "obj_%d" % rng.integers(n), bool(rng.random() < 0.3)) for k in range(n)]
    pre_spec += [(int(rng.integers(n)), "obj_%d" % (n + i), False) for i in range(int(rng.integers(0, 3)))]
    pre_spec[-1] = pre_spec[-1][:2] + (False,)  # the last previous object's 'mug' decides the whole current frame
    for sub in range(100):
        r2 = np.random.default_rng([seed, sub])
        anns = name_objects(PC.synth_annotations(r2, specs, w, h))
        pre = previous_frame(r2, anns, pre_spec)
        draws = draw_track_noise(r2, len(pre["objects"]))
        try:
            recs = pack_track_annotations(anns, pre, np.eye(2, 3), np.eye(2, 3), w, h, False, 0.0, opt, draws)
        except ValueError:
            continue
        if _clean(recs, S):
            return opt, anns, pre, w, h, seed * 1000 + sub, draws
    raise RuntimeError("no clean draw for random case %d" % seed)
