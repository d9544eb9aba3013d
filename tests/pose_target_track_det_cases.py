"""Seeded cases of the tracking task's targets with the detector in the loop (data_generation_mode 1), shared by
tools/make_pose_target_track_det_goldens.py and the tests: tests/pose_target_track_cases.py's two-frame annotations, a
synthetic detector answer in the device layout (cp_postprocess / cp_pnp_from_post rows, built around the previous
frame's annotations so that each case's matching events occur), and, where the reference tree is present, a runner of
its unmodified ObjectPoseDataset.__getitem__ with data_generation_mode_ratio = 1.0 whose ``detector`` is a stub that
returns the boxes of those rows.  The golden file stores the records, the rows and the reference's outputs."""
import copy
import json
import os
import sys
import tempfile
import types

import numpy as np

from centerpose_amd import hip
from centerpose_amd.lib.utils.image import get_affine_transform
from centerpose_amd.pose_targets import num_symmetry
from centerpose_amd.pose_targets_track import draw_track_noise, pack_track_annotations
from tests import pose_target_cases as PC
from tests import pose_target_track_cases as TC
from tests import pose_targets_track_det_ref as DR

POST, PNP = hip.POST_STRIDE, hip.PNP_STRIDE
PF = hip.POST_FIELDS

# detector slots, in order.  o = index of a previous object:
#   ("gt", o, d)        a box on object o's annotation, every vertex moved by d pixels (+ 0.3 px jitter)
#   ("gt", o, d, kw)    kw: far="kps" / "pnp"  vertex 3 of kps (read under render_hmhp_mode 0 / 1) or of the reprojection
#                       (2 / 3, where it also enters the norms) at 3 x width: a detector point outside the input;
#                       std=v  every kps_heatmap_std (0.3: radius_detector 0); score=v; height=v
#   ("at", x, y)        a box of 40 px around the normalised point (x, y): a far match for whatever is nearest
#   ("fail",)           PnP status 0        ("behind",)  status 2 (t_z < 0)
#   ("reject",)         solved, but the reprojected centroid is outside the image: pnp_shell's reject
#   ("out3",)           solved, centroid inside, 3 vertices outside: rejected under the 3-point rule only
# per case, besides the slots:
#   twins=[(a, b)]      previous object b gets a's projected_cuboid: every box is exactly as far from the one as the other
#   centre_out=[o]      previous object o's annotated centre is moved out of the image: nine points of -10000 in
#                       instances_2d, while its corners keep it in the per-object loop
CASES = {
    # name: dict(seed, opt overrides, wh, current specs, previous [(current index, name or None, mug)], det slots, ...)
    "plain_hp2": dict(seed=31, over=dict(c="camera", flip=0.0, render_hm_mode=1, render_hmhp_mode=2, tracking_label_mode=1),
                      wh=(640, 480), specs=[(None, "pose")] * 4, pre=[(0, None, False), (1, None, False), (2, None, False),
                                                                      (3, None, False)],
                      det=[("gt", 1, 3.0), ("fail",), ("gt", 0, 2.0), ("gt", 1, 9.0), ("reject",), ("gt", 3, 4.0, dict(score=0.0))]),
    "no_boxes": dict(seed=32, over=dict(c="camera", flip=0.0, render_hm_mode=0, render_hmhp_mode=0, tracking_label_mode=0),
                     wh=(640, 480), specs=[(None, "pose")] * 3, pre=[(0, None, False), (1, None, False), (2, None, False)],
                     det=[("fail",), ("behind",), ("reject",)]),
    "empty": dict(seed=33, over=dict(c="camera", flip=0.0, render_hm_mode=0, render_hmhp_mode=1, tracking_label_mode=1),
                  wh=(640, 480), specs=[(None, "pose")] * 2, pre=[(0, None, False), (1, None, False)], det=[]),
    "twins_hp0": dict(seed=34, over=dict(c="camera", flip=0.0, render_hm_mode=1, render_hmhp_mode=0, tracking_label_mode=1),
                      wh=(640, 480), specs=[(None, "pose")] * 4, pre=[(0, None, False), (1, None, False), (1, "obj_9", False),
                                                                      (3, None, False)], twins=[(1, 2)],
                      det=[("gt", 2, 2.0), ("gt", 0, 3.0, dict(std=0.3)), ("gt", 3, 2.0, dict(far="kps"))]),
    "far_single": dict(seed=35, over=dict(c="camera", flip=0.0, render_hm_mode=0, render_hmhp_mode=1, tracking_label_mode=1),
                       wh=(640, 480), specs=[(None, "pose")], pre=[(0, None, False)], centre_out=[0], det=[("at", 0.4, 0.5)]),
    "far_multi": dict(seed=36, over=dict(c="camera", flip=0.0, render_hm_mode=0, render_hmhp_mode=3, tracking_label_mode=0),
                      wh=(640, 480), specs=[(None, "pose"), (None, "pose")], pre=[(0, None, False), (1, None, False)],
                      centre_out=[0, 1], det=[("at", 0.4, 0.5), ("at", 0.6, 0.4)]),
    "invisible_mix": dict(seed=37, over=dict(c="camera", flip=0.0, render_hm_mode=1, render_hmhp_mode=3, tracking_label_mode=1),
                          wh=(640, 480), specs=[(None, "pose"), (None, "pose"), (None, "pose")],
                          pre=[(0, None, False), (1, None, False), (2, None, False)], centre_out=[1],
                          det=[("gt", 2, 3.0), ("gt", 0, 2.0, dict(far="pnp"))]),
    "flipped_l0": dict(seed=38, over=dict(c="camera", flip=1.0, render_hm_mode=1, render_hmhp_mode=2, tracking_label_mode=0),
                       wh=(640, 480), specs=[(None, "pose")] * 3, pre=[(0, None, False), (1, None, False), (2, None, False)],
                       det=[("gt", 0, 2.0), ("gt", 2, 3.0), ("out3",)]),
    "chair_s4": dict(seed=39, over=dict(c="chair", flip=0.0, render_hm_mode=1, render_hmhp_mode=2, tracking_label_mode=1),
                     wh=(640, 480), specs=[("True", "pose"), ("False", "pose"), ("True", "pose")],
                     pre=[(0, None, False), (1, None, False), (2, None, False)],
                     det=[("gt", 0, 2.0), ("out3",), ("gt", 1, 3.0), ("gt", 2, 2.0)]),
    "rect": dict(seed=40, over=dict(c="camera", flip=1.0, input_w=320, input_h=256, render_hm_mode=0, render_hmhp_mode=0,
                                    tracking_label_mode=1, same_aug_pre=True),
                 wh=(480, 640), specs=[(None, "pose")] * 3, pre=[(0, None, False), (1, None, False), (2, None, False)],
                 det=[("gt", 1, 2.0), ("gt", 0, 3.0, dict(std=0.3)), ("gt", 2, 4.0)]),
}
# cases that are also run in the noise-simulation mode (stored as "<name>@0"): the batch that mixes the modes is
# (plain_hp2@0, plain_hp2, plain_hp2@0), one option set
MODE0 = ("plain_hp2",)


def make_opt(over=None, **kw):
    o = dict(render_hm_mode=0, render_hmhp_mode=0, data_generation_mode_ratio=1.0)
    o.update(over or {})
    o.update(kw)
    return TC.make_opt(o)


def _set(row, name, values):
    off, w = PF[name]
    row[off:off + w] = values


def _box_rows(rng, verts, width, height, status=1, far=None, std=None, score=None, height_v=None):
    """(post row, pnp row) of a detection whose reprojected vertices are ``verts`` [8, 2] in pixels."""
    post, pnp = np.zeros(POST), np.zeros(PNP)
    v = np.array(verts, np.float64)
    kps = v + rng.uniform(-1.0, 1.0, (8, 2))
    if far == "pnp":
        v[3, 0] = 3.0 * width
    elif far == "kps":
        kps[3, 0] = 3.0 * width
    post[0] = rng.uniform(0.35, 0.95) if score is None else score
    _set(post, "obj_scale", rng.uniform(0.5, 1.5, 3))
    _set(post, "ct", v.mean(0) + rng.uniform(-2, 2, 2))
    _set(post, "kps", kps.reshape(-1))
    _set(post, "kps_heatmap_std", np.full(16, std) if std is not None else rng.uniform(2.5, 6.0, 16))
    _set(post, "kps_heatmap_height", np.full(8, height_v) if height_v is not None else rng.uniform(0.2, 1.0, 8))
    _set(post, "kps_displacement_mean", kps.reshape(-1))
    _set(post, "kps_heatmap_mean", kps.reshape(-1))
    pnp[0] = status
    pnp[8:24] = v.reshape(-1)
    q = rng.normal(size=4)
    pnp[24:28] = pnp[31:35] = q / np.linalg.norm(q)
    pnp[4:7] = pnp[28:31] = rng.uniform(-0.3, 0.3, 3) + [0, 0, 1.5]
    return post, pnp


def synth_detections(rng, recs, slots, K):
    """post [K, 120], count, pnp [K, 40] for one image's packed records and its slot list (len(slots) <= K)."""
    img, pobj = recs["pt_image"], recs["ptk_pre_objects"]
    npre = int(recs["ptk_image"][hip.PTK_IMG["num_pre"]])
    width, height = int(img[hip.PT_IMG["width"]]), int(img[hip.PT_IMG["height"]])
    wh = np.array([width, height], np.float64)
    # the annotations where the matching sees them: flipped and swapped, in pixels (an invisible centre: the raw cuboid)
    inst = DR.instances_2d(img, pobj, npre)
    post, pnp = np.zeros((K, POST)), np.full((K, PNP), 0.0)
    pnp[:, 0] = -1
    box = np.array([[-1, -1], [1, -1], [-1, 1], [1, 1], [-0.8, -0.8], [0.8, -0.8], [-0.8, 0.8], [0.8, 0.8]]) * 40.0
    for k, s in enumerate(slots):
        kw = dict(s[3]) if len(s) > 3 and isinstance(s[3], dict) else {}
        if "height" in kw:
            kw["height_v"] = kw.pop("height")
        if s[0] == "gt":
            g = inst[s[1], 1:, :].astype(np.float64) * wh
            assert g.min() > -5000, "slot %d: object %d has no visible centre" % (k, s[1])
            post[k], pnp[k] = _box_rows(rng, g + s[2] + rng.uniform(-0.3, 0.3, (8, 2)), width, height, **kw)
        elif s[0] == "at":
            post[k], pnp[k] = _box_rows(rng, np.array([s[1], s[2]]) * wh + box, width, height, **kw)
        elif s[0] in ("fail", "behind"):
            post[k], pnp[k] = _box_rows(rng, np.array([0.5, 0.5]) * wh + box, width, height, status=0 if s[0] == "fail" else 2)
        elif s[0] == "reject":
            post[k], pnp[k] = _box_rows(rng, np.array([1.2, 0.5]) * wh + box, width, height)
        elif s[0] == "out3":
            v = np.array([0.5, 0.5]) * wh + box
            v[:3, 0] -= 0.6 * width
            post[k], pnp[k] = _box_rows(rng, v, width, height)
        else:
            raise ValueError(s)
    return post, len(slots), pnp


def boxes_of(recs, post, count, pnp, opt):
    img = recs["pt_image"]
    return DR.boxes_from_records(post, count, pnp, int(img[hip.PT_IMG["width"]]), int(img[hip.PT_IMG["height"]]), opt.c)


def no_near_tie(recs, boxes, rel=1e-9):
    """The condition the cases are built under: for every box the two smallest norms differ by more than ``rel``
    relative or are exactly equal (twin annotations), so no argmin hangs on the order of a float64 sum; the same for
    the nearest of several boxes of one object, and no norm lies near the 1000 threshold."""
    npre = int(recs["ptk_image"][hip.PTK_IMG["num_pre"]])
    if not boxes or not npre:
        return True
    nl = DR.norms(DR.instances_2d(recs["pt_image"], recs["ptk_pre_objects"], npre), boxes)
    ok = bool(np.all(np.abs(nl - 1000.0) > 1.0))
    for row in nl:
        a = np.sort(row)
        ok = ok and (len(a) < 2 or a[0] == a[1] or (a[1] - a[0]) > rel * a[1])
    md = np.argmin(nl, axis=1)
    for o in range(npre):
        a = np.sort(nl[md == o, o])
        ok = ok and (len(a) < 2 or (a[1] - a[0]) > rel * a[1])
    return ok


def annotations(name):
    """(opt, anns, anns_pre, width, height, seed, draws) of case ``name`` (pose_target_track_cases.annotations' scheme)."""
    c = CASES[name]
    opt = make_opt(c["over"])
    S = num_symmetry(opt)
    w, h = c["wh"]
    for sub in range(100):
        rng = np.random.default_rng([c["seed"], sub])
        anns = TC.name_objects(PC.synth_annotations(rng, c["specs"], w, h))
        pre = TC.previous_frame(rng, anns, c["pre"])
        for a, b in c.get("twins", ()):
            pre["objects"][b]["projected_cuboid"] = copy.deepcopy(pre["objects"][a]["projected_cuboid"])
        for o in c.get("centre_out", ()):
            pre["objects"][o]["projected_cuboid"][0] = [w + 30.0, h / 2.0]
        pre["camera_data"]["intrinsics"] = {"fx": 1.1 * max(w, h), "fy": 1.1 * max(w, h), "cx": w / 2.0, "cy": h / 2.0}
        draws = draw_track_noise(rng, len(pre["objects"]))
        recs = pack_track_annotations(anns, pre, np.eye(2, 3), np.eye(2, 3), w, h, False, 0.0, opt, draws)
        if TC._clean(recs, S):
            return opt, anns, pre, w, h, c["seed"] * 1000 + sub, draws
    raise RuntimeError("no clean draw for case %s" % name)


def synth_pack(opt, anns, pre, w, h, draws, mode, flipped, rng, aug=True, max_pre_objs=None):
    """Records of one sample without the reference: affines as the dataset builds them from an augmentation centre and
    extent, the generation record with them."""
    c = np.array([w / 2.0, h / 2.0], np.float32) + (rng.uniform(-20, 20, 2).astype(np.float32) if aug else 0)
    s0 = float(max(w, h))
    aug_s, aug_s_pre = (float(rng.uniform(0.8, 1.2)), float(rng.uniform(0.8, 1.2))) if aug else (1.0, 1.0)
    if flipped:
        c[0] = w - c[0] - 1
    R = int(opt.output_res)
    t_out = get_affine_transform(c, s0 * aug_s, 0, [R, R])
    t_in_pre = get_affine_transform(c, s0 * aug_s_pre, 0, [opt.input_w, opt.input_h])
    gen = dict(mode=mode, c=c, s=s0 * aug_s_pre, aug_s=aug_s_pre, intrinsics=pre["camera_data"]["intrinsics"])
    return pack_track_annotations(anns, pre, t_out, t_in_pre, w, h, flipped, 0.0, opt, draws, generation=gen,
                                  max_pre_objs=max_pre_objs)


# ---- the reference's own __getitem__ with a stub detector ----

class _Detector:
    """ds.detector: run() returns the prescribed boxes, fresh copies per call (the reference scales box[0] / box[3] in
    place, :677-678), and records the meta it was handed."""

    def __init__(self, make_boxes):
        self.make_boxes, self.meta = make_boxes, None

    def run(self, img, filename=None, meta_inp=None, preprocessed_flag=False):
        self.meta = meta_inp
        return {"boxes": self.make_boxes()}


def run_reference(opt, anns, anns_pre, width, height, seed, draws, make_boxes):
    """pose_target_track_cases.run_reference with ds.detector (and detector_cup / detector_mug) set to the stub; returns
    (ret, captured): the affines and flags as there, plus c / s / aug_s of the previous frame as the reference resolves
    them (:438-449, :478-489, :681-690) and data_generation_mode."""
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
        TC._Shims(draws).install(mod)
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
            ds.detector = ds.detector_cup = ds.detector_mug = _Detector(make_boxes)
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
                                                        "height", "data_generation_mode", "frame_dist")})
                    same = bool(opt.same_aug_pre and loc.get("frame_dist") != 0)
                    cap["c"], cap["s"] = (loc["c"], loc["s"]) if same else (loc["c_pre"], loc["s_pre"])
                    cap["aug_s"] = loc["aug_s"] if same else loc["aug_s_pre"]

            np.random.seed(seed % (2 ** 32))
            sys.setprofile(prof)
            try:
                ret = ds[0]
            finally:
                sys.setprofile(None)
            cap["meta"] = ds.detector.meta
    finally:
        for name in set(sys.modules) - before:
            del sys.modules[name]
        sys.path[:] = path
    return ret, cap


def pack(opt, anns, anns_pre, cap, draws, mode=1):
    gen = dict(mode=mode, c=cap["c"], s=cap["s"], aug_s=cap["aug_s"], intrinsics=anns_pre["camera_data"]["intrinsics"])
    return pack_track_annotations(anns, anns_pre, cap["trans_output_rot"], cap["trans_input_pre"], cap["width"],
                                  cap["height"], cap["flipped"], cap["rot"], opt, draws, generation=gen)


def reference_case(opt, anns, anns_pre, width, height, seed, draws, slots, K=16, mode=1):
    """(records, (post, count, pnp), reference ret) of one pair of frames in mode 1.  The detector's rows depend on the
    annotations, the image size and the flip only, and opt.flip is 0 or 1 in every case, so they are built before the
    run from a packing with placeholder affines."""
    flipped = opt.flip >= 1.0
    pre0 = pack_track_annotations(anns, anns_pre, np.eye(2, 3), np.eye(2, 3), width, height, flipped, 0.0, opt, draws)
    rows = synth_detections(np.random.default_rng([seed, 7]), pre0, slots, K)
    if mode == 0:  # the same sample in the noise-simulation mode: the detector is never asked
        opt = copy.copy(opt)
        opt.data_generation_mode_ratio = 0
    ret, cap = run_reference(opt, anns, anns_pre, width, height, seed, draws, lambda: boxes_of(pre0, *rows, opt))
    assert cap["data_generation_mode"] == mode and bool(cap["flipped"]) == flipped
    return pack(opt, anns, anns_pre, cap, draws, mode), rows, ret


def golden_case(name, mode=1):
    opt, anns, pre, w, h, seed, draws = annotations(name)
    return (opt,) + reference_case(opt, anns, pre, w, h, seed, draws, CASES[name]["det"], mode=mode)


def random_slots(rng, recs, n):
    """A random detector answer for packed records: boxes on visible objects (some twice), far boxes, failures."""
    npre = int(recs["ptk_image"][hip.PTK_IMG["num_pre"]])
    inst = DR.instances_2d(recs["pt_image"], recs["ptk_pre_objects"], npre)
    vis = [o for o in range(npre) if inst[o].min() > -5000]
    slots = []
    for _ in range(n):
        u = rng.random()
        if vis and u < 0.6:
            kw = {}
            if rng.random() < 0.2:
                kw["far"] = ("kps", "pnp")[int(rng.integers(2))]
            if rng.random() < 0.2:
                kw["std"] = 0.3
            if rng.random() < 0.15:
                kw["score"] = 0.0
            slots.append(("gt", int(vis[rng.integers(len(vis))]), float(rng.uniform(-12, 12)), kw))
        elif u < 0.75:
            slots.append(("at", float(rng.uniform(0.2, 0.8)), float(rng.uniform(0.2, 0.8))))
        else:
            slots.append((("fail",), ("behind",), ("reject",), ("out3",))[int(rng.integers(4))])
    return slots


def random_case(seed, **over):
    """A freshly seeded pair of frames and detector answer for the live comparison."""
    rng = np.random.default_rng([seed, 99])
    o = dict(flip=float(rng.integers(2)), render_hm_mode=int(rng.integers(2)), render_hmhp_mode=int(rng.integers(4)))
    o.update(over)
    opt, anns, pre, w, h, s, draws = TC.random_case(seed, data_generation_mode_ratio=1.0, **o)
    pre = copy.deepcopy(pre)
    pre["camera_data"]["intrinsics"] = {"fx": 1.1 * max(w, h), "fy": 1.1 * max(w, h), "cx": w / 2.0, "cy": h / 2.0}
    return opt, anns, pre, w, h, s, draws


def random_image(rng, opt, mode=1, n_slots=None, K=16, max_pre_objs=None):
    """(records, (post, count, pnp)) of one synthetic sample with dataset-style affines and a random detector answer."""
    S = num_symmetry(opt)
    kinds = ["pose", "pose", "pose", "pose", "edge", "twin", "out5", "corner_neg"]
    syms = ["True", "False", None] if S >= 4 else [None]
    while True:
        w, h = (640, 480) if rng.random() < 0.5 else (480, 640)
        n = int(rng.integers(1, 8))
        specs = [(syms[int(rng.integers(len(syms)))], kinds[int(rng.integers(len(kinds)))]) for _ in range(n)]
        anns = TC.name_objects(PC.synth_annotations(rng, specs, w, h))
        pre = TC.previous_frame(rng, anns, [(k, None, False) for k in range(n)])
        if rng.random() < 0.3:
            pre["objects"][int(rng.integers(n))]["projected_cuboid"][0] = [w + 30.0, h / 2.0]
        pre["camera_data"]["intrinsics"] = {"fx": 1.1 * max(w, h), "fy": 1.1 * max(w, h), "cx": w / 2.0, "cy": h / 2.0}
        draws = draw_track_noise(rng, n)
        try:
            recs = synth_pack(opt, anns, pre, w, h, draws, mode, bool(rng.random() < 0.5), rng, max_pre_objs=max_pre_objs)
        except ValueError:
            continue
        slots = random_slots(rng, recs, int(rng.integers(0, 9)) if n_slots is None else n_slots)
        rows = synth_detections(rng, recs, slots, K)
        if no_near_tie(recs, boxes_of(recs, *rows, opt)):
            return recs, rows
