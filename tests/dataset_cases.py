"""Cases of the lib.datasets tests (test helper, not a test module), shared with tools/make_dataset_goldens.py.

Each case is one synthetic image (tests/pose_target_cases.py's annotations) with its options and seed.  ``reference_run``
drives the reference's unmodified ``__getitem__`` through ``pose_target_cases.run_reference`` (imported, not edited) and
captures what that helper does not return: ``trans_input`` (the matrix its cv2 stub's warpAffine receives), the colour
draws (a recording proxy around ``_data_rng`` and ``random.shuffle``) and the three generators' states afterwards.  The
helper pins ``split = 'train'`` and its cv2 stub has no ``cvtColor``; a trace function sets the split of a 'val' case on
the instance when ``__getitem__`` is entered, and the stub is wrapped (``PC._cv2_stub`` is looked up when called).
``dataset_run`` drives the new dataset on a temporary tree with the same annotations, seeds and a black PNG of the same
size.  The golden file stores ``reference_run``'s captures, so the comparison also runs where the reference is absent.
"""
import hashlib
import json
import os
import random
import sys
import tempfile

import numpy as np

from centerpose_amd import hip
from tests import pose_target_cases as PC
from tests import pose_target_track_cases as PTC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_ref.npz")

# name: (seed, category, split, option overrides)
CASES = {
    "chair_flip0": (31, "chair", "train", dict(flip=0.0, aug_rot=0.0, not_rand_crop=True, no_color_aug=True)),
    "chair_flip1_color": (32, "chair", "train", dict(flip=1.0, aug_rot=0.0, not_rand_crop=False, no_color_aug=False)),
    "chair_half_a": (33, "chair", "train", dict(flip=0.5, aug_rot=0.5, not_rand_crop=False, no_color_aug=False)),
    "chair_half_b": (34, "chair", "train", dict(flip=0.5, aug_rot=0.5, not_rand_crop=True, no_color_aug=False)),
    "bottle_s12": (35, "bottle", "train", dict(num_symmetry=12, flip=0.5, aug_rot=0.5, not_rand_crop=False, no_color_aug=True)),
    "bottle_s12_color": (36, "bottle", "train", dict(num_symmetry=12, flip=0.5, aug_rot=0.0, not_rand_crop=True, no_color_aug=False)),
    "camera_rot": (37, "camera", "train", dict(flip=0.5, aug_rot=0.5, not_rand_crop=True, no_color_aug=True)),
    "camera_crop_color": (38, "camera", "train", dict(flip=0.0, aug_rot=0.5, not_rand_crop=False, no_color_aug=False)),
    "camera_flip1": (39, "camera", "train", dict(flip=1.0, aug_rot=0.0, not_rand_crop=False, no_color_aug=True)),
    "chair_val": (40, "chair", "val", dict(flip=0.5, aug_rot=0.5, not_rand_crop=False, no_color_aug=False)),
    "camera_val": (41, "camera", "val", dict(flip=1.0, aug_rot=0.0, not_rand_crop=True, no_color_aug=True)),
}
TRACK_CASES = {
    # name: (pose_target_track_cases seed, same_aug_pre, option overrides)
    "track_own_aug": (51, False, dict(no_color_aug=True)),
    "track_same_aug": (52, True, dict(no_color_aug=False)),
    "track_own_aug_color": (53, False, dict(no_color_aug=False, flip=1.0)),
}


def case(name):
    seed, cat, split, over = CASES[name]
    opt, anns, w, h, run_seed = PC.random_case(seed, cat, n_obj=3, **over)
    opt.tracking_task, opt.data_generation_mode_ratio = False, 0
    return opt, anns, w, h, run_seed, split


def track_case(name):
    seed, same, over = TRACK_CASES[name]
    opt, anns, pre, w, h, run_seed, draws = PTC.random_case(seed, same_aug_pre=same, **over)
    return opt, anns, pre, w, h, run_seed, draws


def state_digest(state):
    """A generator's state as a short string: equal digests, equal states."""
    h = hashlib.sha256()
    for part in state:
        if isinstance(part, np.ndarray):
            h.update(np.ascontiguousarray(part).tobytes())
        elif isinstance(part, tuple):
            h.update(repr(part).encode())
        else:
            h.update(repr(part).encode())
    return h.hexdigest()


def states(data_rng):
    return {"np": state_digest(np.random.get_state()), "py": state_digest(random.getstate()),
            "data_rng": state_digest(data_rng.get_state())}


class _RecordingRng(object):
    """_data_rng with its uniform / normal draws recorded in call order."""

    def __init__(self, rng):
        self.rng, self.uniforms, self.normals = rng, [], []

    def uniform(self, *a, **k):
        v = self.rng.uniform(*a, **k)
        self.uniforms.append(v)
        return v

    def normal(self, *a, **k):
        v = self.rng.normal(*a, **k)
        self.normals.append(v)
        return v

    def get_state(self):
        return self.rng.get_state()


class _Capture(object):
    """What the wrapped stub and the trace function record of one reference run."""

    def __init__(self, split):
        self.split, self.ds, self.trans, self.rngs, self.orders = split, None, [], [], []

    def stub(self, make):
        cap = self

        def wrapped(sizes):
            cv2 = make(sizes)
            inner = cv2.warpAffine

            def warpAffine(img, M, dsize, flags=None):
                ds = sys._getframe(1).f_locals["self"]  # _get_input's frame
                cap.ds = ds
                cap.trans.append(np.array(M, np.float64))
                rec = _RecordingRng(ds._data_rng.rng if isinstance(ds._data_rng, _RecordingRng) else ds._data_rng)
                ds._data_rng = rec  # color_aug, if it runs, draws through it
                cap.rngs.append(rec)
                return inner(img, M, dsize, flags)

            cv2.warpAffine, cv2.COLOR_BGR2GRAY = warpAffine, 6
            cv2.cvtColor = lambda image, code: image.mean(axis=2)  # grayscale(): only its shape and dtype matter here
            return cv2

        return wrapped

    def trace(self, frame, event, arg):
        if event == "call" and frame.f_code.co_name == "__getitem__" and frame.f_code.co_filename.endswith("dataset_combined.py"):
            frame.f_locals["self"].split = self.split
        return None

    def colors(self):
        """One colour dict (draw_color_aug's format) or None per _get_input call."""
        out, orders = [], list(self.orders)
        for rec in self.rngs:
            if not rec.uniforms:
                out.append(None)
                continue
            names = orders.pop(0)
            out.append({"order": hip.TI_ORDERS.index("".join(n[0] for n in names)), "alphas": [1. + u for u in rec.uniforms],
                        "light": np.asarray(rec.normals[0], np.float64)})
        return out


def _run(cap, seed, call):
    orig_stub, orig_shuffle = PC._cv2_stub, random.shuffle

    def shuffle(x, *a):
        orig_shuffle(x, *a)
        if x and callable(x[0]):
            cap.orders.append([f.__name__ for f in x])

    PC._cv2_stub, random.shuffle = cap.stub(orig_stub), shuffle
    random.seed(seed)
    outer = sys.gettrace()
    sys.settrace(cap.trace)
    try:
        return call()
    finally:
        sys.settrace(outer)
        PC._cv2_stub, random.shuffle = orig_stub, orig_shuffle


def reference_run(name):
    """The reference's captures of a single-frame case: {trans_input, trans_output_rot, rot, flipped, width, height,
    color (dict or None), states}."""
    opt, anns, w, h, seed, split = case(name)
    cap = _Capture(split)
    ret, loc = _run(cap, seed, lambda: PC.run_reference(opt, anns, w, h, seed))
    assert ret is not None and len(cap.trans) == 1
    return {"trans_input": cap.trans[0], "trans_output_rot": np.array(loc["trans_output_rot"], np.float64), "rot": float(loc["rot"]),
            "flipped": bool(loc["flipped"]), "width": int(loc["width"]), "height": int(loc["height"]), "color": cap.colors()[0],
            "states": states(cap.ds._data_rng)}


def reference_track_run(name):
    """The reference's captures of a two-frame case.  Its noise draws read the packed slots (pose_target_track_cases'
    shims), so the generators' states afterwards are those at the point where the noise draws begin."""
    opt, anns, pre, w, h, seed, draws = track_case(name)
    cap = _Capture("train")
    ret, loc = _run(cap, seed, lambda: PTC.run_reference(opt, anns, pre, w, h, seed, draws))
    assert ret is not None and len(cap.trans) == 2
    colors = cap.colors()
    return {"trans_input": cap.trans[0], "trans_input_pre": np.array(loc["trans_input_pre"], np.float64),
            "trans_output_rot": np.array(loc["trans_output_rot"], np.float64), "rot": float(loc["rot"]),
            "flipped": bool(loc["flipped"]), "width": int(loc["width"]), "height": int(loc["height"]), "color": colors[0],
            "color_pre": colors[1], "states": states(cap.ds._data_rng)}


# ---- the new dataset on the same inputs ----

class same_cv2(object):
    """Both sides get the same stand-in for cv2.getAffineTransform.  The reference runs on pose_target_cases' stub (a
    3x3 solve per output row); the mirror's lib.utils.image solves the 6x6 system, which agrees with it to the last bits
    only without a rotation.  Neither is OpenCV's own arithmetic, so for the comparison the mirror's solver is the
    stub's, as it would be cv2's on both sides where cv2 is installed."""

    def __enter__(self):
        from centerpose_amd.lib.utils import image

        self.image, self.inner = image, image._affine_from_3pts
        image._affine_from_3pts = PC._cv2_stub({}).getAffineTransform

    def __exit__(self, *exc):
        self.image._affine_from_3pts = self.inner


def write_tree(root, opt, split, frames, tracking=False):
    """``frames``: [(frame id, annotations, (w, h))] of one video 'v0' under the split's directory, black PNGs."""
    from PIL import Image

    video = os.path.join(root, "outf_all" if tracking else "outf", "%s_%s" % (opt.c, split), "v0")
    os.makedirs(video)
    for fid, anns, (w, h) in frames:
        Image.fromarray(np.zeros((h, w, 3), np.uint8), "RGB").save(os.path.join(video, "%s.png" % fid))
        with open(os.path.join(video, "%s.json" % fid), "w") as fh:
            json.dump(anns, fh)
    return video


def dataset_run(name):
    """(sample, states after the call) of the new dataset's __getitem__ on a single-frame case."""
    from centerpose_amd.lib.datasets.dataset_combined import ObjectPoseDataset

    opt, anns, w, h, seed, split = case(name)
    with tempfile.TemporaryDirectory() as tmp:
        write_tree(tmp, opt, split, [("0", anns, (w, h))])
        opt.data_dir = tmp
        ds = ObjectPoseDataset(opt, split)
        assert len(ds) == 1
        np.random.seed(seed % (2 ** 32))
        random.seed(seed)
        with same_cv2():
            sample = ds[0]
    return sample, states(ds._data_rng)


def dataset_track_run(name):
    """(sample, states where the noise draws begin, the dataset's own draw_track_noise output) on a two-frame case.  As
    in the reference's run, the sample list holds the current frame only and the video's group the previous frame
    only."""
    from centerpose_amd.lib.datasets import dataset_combined as DC

    opt, anns, pre, w, h, seed, _ = track_case(name)
    seen = {}
    inner = DC.draw_track_noise

    def draw(rng, n):
        seen["states"] = states(ds._data_rng)
        seen["draws"] = inner(rng, n)
        return seen["draws"]

    with tempfile.TemporaryDirectory() as tmp:
        write_tree(tmp, opt, "train", [("0", anns, (w, h)), ("1", pre, (w, h))], tracking=True)
        opt.data_dir = tmp
        ds = DC.ObjectPoseDataset(opt, "train")
        assert len(ds) == 2
        cur = [s for s in ds.images if s[2] == "0"]
        ds.videos = {"v0": [s for s in ds.images if s[2] == "1"]}
        ds.images = cur
        np.random.seed(seed % (2 ** 32))
        random.seed(seed)
        DC.draw_track_noise = draw
        try:
            with same_cv2():
                sample = ds[0]
        finally:
            DC.draw_track_noise = inner
    return sample, seen["states"], seen["draws"]


# ---- the golden file ----

_ARRAYS = ("trans_input", "trans_input_pre", "trans_output_rot")


def to_golden(out, name, cap):
    for k in _ARRAYS:
        if k in cap:
            out["%s/%s" % (name, k)] = cap[k]
    out[name + "/scalars"] = np.array([cap["rot"], cap["flipped"], cap["width"], cap["height"]], np.float64)
    for key in ("color", "color_pre"):
        if key in cap:
            c = cap[key]
            out["%s/%s" % (name, key)] = np.zeros(0) if c is None else np.concatenate([[c["order"]], c["alphas"], c["light"]])
    out[name + "/states"] = np.array([cap["states"][k] for k in ("np", "py", "data_rng")])


def from_golden(z, name):
    cap = {k: z["%s/%s" % (name, k)] for k in _ARRAYS if "%s/%s" % (name, k) in z.files}
    rot, flipped, width, height = z[name + "/scalars"]
    cap.update(rot=float(rot), flipped=bool(flipped), width=int(width), height=int(height))
    for key in ("color", "color_pre"):
        if "%s/%s" % (name, key) in z.files:
            v = z["%s/%s" % (name, key)]
            cap[key] = None if v.size == 0 else {"order": int(v[0]), "alphas": [float(a) for a in v[1:4]], "light": v[4:7]}
    cap["states"] = dict(zip(("np", "py", "data_rng"), (str(s) for s in z[name + "/states"])))
    return cap
