"""Seeded cases of the training input images shared by tools/make_train_input_goldens.py and the tests: random 8-bit
frames of three sizes, transforms from the mirror's get_affine_transform, colour draws, and, where the reference tree is
present, runners of its own color_aug and ObjectPoseDataset._get_input with cv2 stubbed (warpAffine as
oracle.cv_emul.warp_affine_u8, cvtColor as the BGR2GRAY formula for float images)."""
import os
import random
import sys
import types
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np

from centerpose_amd import hip
from centerpose_amd.lib.utils.image import get_affine_transform
from centerpose_amd.train_inputs import draw_color_aug, pack_input
from oracle import cv_emul
from tests import train_inputs_ref as R

REF = os.environ.get("CENTERPOSE_REFERENCE", "/root/reference")
SIZES = {"a": (40, 56), "b": (37, 53), "c": (64, 48)}  # (height, width) of the source frames
GOLDEN_CASES = ("geometry36/4", "border48/1", "orders36/3", "mixed48/2")  # batch / image; written at side 36


def frame(size, seed):
    h, w = SIZES[size]
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def transform(kind, size, side, flipped):
    """The forward 2x3 input affine of a named geometry, built as the dataset builds trans_input (:325-345)."""
    h, w = SIZES[size]
    c = np.array([w / 2., h / 2.], dtype=np.float32)
    s, rot = max(h, w) * 1.0, 0
    if kind == "scale06":
        s *= 0.6
    elif kind == "scale14":
        s *= 1.4
    elif kind == "rot+30":
        rot = 30
    elif kind == "rot-30":
        rot = -30
    elif kind == "corner":  # centred near a corner: over a third of the output reads the zero border
        c = np.array([2., 3.], dtype=np.float32)
    elif kind == "rot20":
        rot = 20
    elif kind == "singular":  # rank 1: cv::invertAffineTransform gives the zero matrix
        return np.array([[1., 2., 3.], [2., 4., 5.]])
    else:
        assert kind == "identity", kind
    if flipped:
        c[0] = w - c[0] - 1
    return np.asarray(get_affine_transform(c, s, rot, [side, side]), np.float64)


# image specs: (frame size, geometry, flipped, colour = None or (order code, alphas as run))
A = (0.6, 1.0, 1.4)
BATCHES = {
    # name: (side, [image specs])
    "geometry36": (36, [("a", "identity", 0, None), ("b", "scale06", 0, None), ("c", "scale14", 0, None),
                        ("a", "rot+30", 0, None), ("b", "rot-30", 0, None)]),
    "border48": (48, [("c", "corner", 0, None), ("a", "rot20", 1, None), ("b", "singular", 0, None),
                      ("c", "identity", 1, None), ("b", "corner", 1, None)]),
    "orders36": (36, [("a", "identity", 0, (0, (A[0], A[1], A[2]))), ("b", "rot+30", 0, (1, (A[2], A[0], A[1]))),
                      ("c", "scale14", 1, (2, (A[1], A[2], A[0]))), ("a", "rot20", 1, (3, (A[2], A[2], A[0]))),
                      ("b", "scale06", 0, (4, (A[0], A[0], A[2])))]),
    "mixed48": (48, [("c", "scale06", 0, (5, (A[1], A[0], A[2]))), ("a", "rot-30", 0, None),
                     ("grey", "scale06", 0, (3, (A[0], A[2], A[2]))), ("b", "corner", 1, (2, (A[2], A[1], A[0]))),
                     ("c", "singular", 0, (4, (A[0], A[1], A[1])))]),
    # beyond the issue's list: an odd side, so that a plane is not 16-byte aligned (the scalar-store path)
    "odd35": (35, [("a", "rot+30", 1, (1, (A[0], A[2], A[1]))), ("b", "identity", 0, None), ("c", "corner", 0, (0, A)),
                   ("b", "singular", 1, None), ("a", "scale14", 0, (5, (A[2], A[0], A[0])))]),
}


def batch(name, side=None):
    """(frames, records [N, TI_STRIDE] without offsets, side) of a named batch; `side` overrides the batch's own."""
    own, specs = BATCHES[name]
    side = own if side is None else side
    seed0 = sorted(BATCHES).index(name) * 100
    frames, recs = [], []
    for n, (size, kind, flipped, col) in enumerate(specs):
        if size == "grey":  # a constant-grey frame and a view without border: gs == gs_mean everywhere
            size, f = "a", np.full(SIZES["a"] + (3,), 128, np.uint8)
        else:
            f = frame(size, seed0 + n)
        h, w = SIZES[size]
        color = None
        if col is not None:
            light = np.random.RandomState(seed0 + 50 + n).normal(scale=0.1, size=(3,))
            color = {"order": col[0], "alphas": list(col[1]), "light": light}
        frames.append(f)
        recs.append(pack_input(transform(kind, size, side, flipped), h, w, flipped, color)["ti_image"])
    return frames, np.stack(recs), side


def border_share(frames, recs, side, n):
    """The share of output pixels of image n with at least one tap outside the frame."""
    ones = np.full(frames[n].shape, 255, np.uint8)
    return float((R.warp_u8(ones, recs[n], side)[..., 0] < 255).mean())


# ---- the host build of train_inputs_common.h ----

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_HOST = []


def host_lib():
    if not _HOST:
        import ctypes
        import subprocess
        out = os.path.join(REPO, "tests", "_build", "libcp_train_inputs_host.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        src = os.path.join(REPO, "tests", "native", "train_inputs_host.cpp")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        L = ctypes.CDLL(out)
        L.ti_host_image.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
        L.ti_host_image.restype = None
        L.ti_host_order_op.argtypes = [ctypes.c_int, ctypes.c_int]
        _HOST.append(L)
    return _HOST[0]


def host_batch(frames, recs, side, gs_means=None):
    """(out [N, 3, side, side] float32, gs_means [N]) of the host build; `gs_means` feeds it given means."""
    from centerpose_amd.train_inputs import MEAN, STD, pack_frames
    L = host_lib()
    buf, recs = pack_frames(frames, recs)
    buf = buf.numpy()
    out = np.zeros((len(frames), 3, side, side), np.float32)
    means = np.zeros(len(frames), np.float32) if gs_means is None else np.array(gs_means, np.float32)
    for n in range(len(frames)):
        rec = np.ascontiguousarray(recs[n])
        L.ti_host_image(buf.ctypes.data, rec.ctypes.data, MEAN.ctypes.data, STD.ctypes.data, side, side,
                        int(gs_means is not None), means[n:].ctypes.data, out[n].ctypes.data)
    return out, means


# ---- the reference's own color_aug / _get_input ----

def reference_available():
    return os.path.isfile(os.path.join(REF, "src", "lib", "utils", "image.py"))


def _cv2_stub():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR, cv2.COLOR_BGR2GRAY = 1, 6
    cv2.warpAffine = lambda img, M, dsize, flags=None: cv_emul.warp_affine_u8(np.ascontiguousarray(img), M, dsize)
    cv2.cvtColor = lambda img, code: R.grey(img)
    return cv2


@contextmanager
def reference_modules():
    """Imports the reference's lib.utils.image and lib.datasets.dataset_combined with cv2, albumentations and the
    detector factory stubbed; they, the reference's modules and its path entry are removed afterwards."""
    before, path = set(sys.modules), list(sys.path)
    try:
        sys.modules["cv2"] = _cv2_stub()
        sys.modules["albumentations"] = types.ModuleType("albumentations")
        df = types.ModuleType("lib.detectors.detector_factory")
        df.detector_factory = {}
        sys.modules["lib.detectors.detector_factory"] = df
        sys.path.insert(0, os.path.join(REF, "src"))
        import lib.utils.image as image  # noqa: E402
        from lib.datasets.dataset_combined import ObjectPoseDataset  # noqa: E402
        yield image, ObjectPoseDataset
    finally:
        for name in set(sys.modules) - before:
            del sys.modules[name]
        sys.path[:] = path


def reference_get_input(ObjectPoseDataset, frame_, trans_input, flipped, side, color_seed):
    """The reference's _get_input (unmodified) on a frame: returns (its [3, side, side] float32 output, the record of the
    same draws).  color_seed None: opt.no_color_aug."""
    ds = ObjectPoseDataset.__new__(ObjectPoseDataset)
    ds.opt = SimpleNamespace(input_res=side, no_color_aug=color_seed is None)
    ds.split = "train"
    ds._eig_val = np.array([0.2141788, 0.01817699, 0.00341571], dtype=np.float32)
    ds._eig_vec = np.array([[-0.58752847, -0.69563484, 0.41340352], [-0.5832747, 0.00994535, -0.81221408],
                            [-0.56089297, 0.71832671, 0.41158938]], dtype=np.float32)
    color = None
    if color_seed is not None:
        color = draw_color_aug(np.random.RandomState(color_seed), random.Random(color_seed))
        ds._data_rng = np.random.RandomState(color_seed)
        random.seed(color_seed)
    img = frame_[:, ::-1, :] if flipped else frame_  # :337
    out = ds._get_input(img, trans_input)
    rec = pack_input(trans_input, frame_.shape[0], frame_.shape[1], flipped, color)["ti_image"]
    return np.ascontiguousarray(out), rec
