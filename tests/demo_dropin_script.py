"""Run in a fresh interpreter by tests/test_demo_dropin.py: a demo-style caller of this repo's package as a drop-in ``lib``
(INTEGRATION.md level 0: put centerpose_amd/ ahead of the application's own directory on sys.path) -- `lib.opts`,
`lib.detectors.detector_factory`, `Detector(opt).run(image_path, meta_inp=meta)` and the nine timing keys of its result.

usage: python demo_dropin_script.py <image> <checkpoint>
Only what cannot exist on a GPU-less machine is substituted: cv2 (if absent: imread through PIL, no windows) and the two
device stages of ``process`` / PnP (the oracle's CPU forward, decode and PnP stand in for libcenterpose_hip.so)."""
import os
import sys
import types

import numpy as np
import torch

image, ckpt = sys.argv[1], sys.argv[2]
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "centerpose_amd"))   # `lib` now resolves to centerpose_amd/lib

try:
    import cv2  # noqa: F401
except ImportError:
    from PIL import Image

    cv2 = types.ModuleType("cv2")
    cv2.imread = lambda p: np.asarray(Image.open(p).convert("RGB"))[:, :, ::-1].copy()
    cv2.imshow = lambda *a, **k: None
    cv2.waitKey = lambda *a, **k: -1
    cv2.VideoCapture = None
    sys.modules["cv2"] = cv2

import lib  # noqa: E402  (this repo's package)

assert os.path.realpath(os.path.dirname(lib.__file__)).startswith(os.path.realpath(REPO)), lib.__file__
from lib.opts import opts  # noqa: E402

# ---- the options a demo run sets (a chair, PnP on, the demo's camera) ----
opt = opts().parser.parse_args(["--demo", image, "--arch", "dla_34", "--load_model", ckpt, "--gpus", "-1", "--c", "chair"])
opt.nms = True
opt.obj_scale = True
meta = {"camera_matrix": np.array([[663.0287679036459, 0, 300.2775065104167], [0, 663.0287679036459, 395.00066121419275],
                                   [0, 0, 1]])}
opt.cam_intrinsic = meta["camera_matrix"]
opt.use_pnp = True
opt = opts().parse(opt)
opt = opts().init(opt)

# ---- CPU stand-ins for the device stages (this box has no GPU) ----
from lib.detectors import base_detector as bd  # noqa: E402
from lib.detectors.object_pose import ObjectPoseDetector  # noqa: E402
from lib.utils.pnp import cuboid_pnp_solver as cps  # noqa: E402
from oracle import backbone as ob  # noqa: E402
from oracle import decode as odec  # noqa: E402
from tests.test_tracking_loop import _oracle_pnp_rows  # noqa: E402

sd = torch.load(ckpt, map_location="cpu")["state_dict"]


def process(self, images, pre_images=None, pre_hms=None, pre_hm_hp=None, pre_inds=None, return_time=False):
    import time

    z = ob.dlaseg_forward(sd, images.float(), self.opt.heads, arch="dla")
    z = {k: v for k, v in z.items()}
    z["hm"], z["hm_hp"] = torch.sigmoid(z["hm"]), torch.sigmoid(z["hm_hp"])
    n = {k: v.numpy() for k, v in z.items()}
    dets = odec.object_pose_decode(n["hm"], n["hps"], wh=n["wh"], obj_scale=n["scale"], reg=n["reg"], hm_hp=n["hm_hp"],
                                   hp_offset=n["hp_offset"], K=self.opt.K, rep_mode=self.opt.rep_mode)
    return (z, dets, time.time()) if return_time else (z, dets)


ObjectPoseDetector.process = process
cps.solve_pnp_batch = _oracle_pnp_rows
bd.solve_pnp_batch = _oracle_pnp_rows

# ---- what a demo does per image: one run() on the file's path, then the timing line ----
from lib.detectors.detector_factory import detector_factory  # noqa: E402

TIME_STATS = ["tot", "load", "pre", "net", "dec", "post", "merge", "pnp", "track"]
detector = detector_factory[opt.task](opt)
ret = detector.run(image, meta_inp=meta)
assert {"results", "boxes", "output"} <= set(ret), sorted(ret)
print("Frame 0|" + "".join("%s %.3fs |" % (k, ret[k]) for k in TIME_STATS))
print("DEMO_DROPIN_OK")
