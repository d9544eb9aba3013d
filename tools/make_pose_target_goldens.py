"""Writes tests/golden/pose_targets_ref.npz: the reference's own ObjectPoseDataset.__getitem__ on the synthetic cases of
tests/pose_target_cases.py.

Runs only where the reference project exists ($CENTERPOSE_REFERENCE, as the other make_*_goldens.py).  The dataset
module is imported unmodified with cv2 (imread: a zero image of the annotation's size, getAffineTransform: the 3-point
solve, warpAffine: zeros), albumentations and lib.detectors.detector_factory stubbed; the instance is made with
__new__ and the attributes __getitem__ reads, np.random is seeded per case, and trans_output_rot / rot / flipped are
read from its frame.  Every case's annotation draw keeps each truncated value of the variant projection at least 1e-6
from an integer (pose_target_cases.annotations re-draws otherwise), so a last-bit difference in the 4x4 products
cannot move a keypoint.

  python tools/make_pose_target_goldens.py

Contents, per case <c> (B = 1, arrays without the batch axis):
  <c>/pt_image [32], <c>/pt_objects [10, 64]   the pack_annotations records of the reference's draw
  <c>/<key>                                    every non-map key of the reference's ret
  <c>/<map>_idx int32, <c>/<map>_val float32   hm / hm_hp as their non-zero (flat index, value) pairs
"""
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "pose_targets_ref.npz")

from centerpose_amd.pose_targets import target_keys  # noqa: E402
from tests import pose_target_cases as PC  # noqa: E402

MAPS = ("hm", "hm_hp")


def main():
    if not PC.reference_available():
        raise SystemExit("the reference tree is not present ($CENTERPOSE_REFERENCE)")
    out = {}
    for name in PC.CASES:
        opt, anns, w, h, seed = PC.annotations(name)
        recs, ret = PC.reference_case(opt, anns, w, h, seed)
        out[name + "/pt_image"] = recs["pt_image"]
        out[name + "/pt_objects"] = recs["pt_objects"]
        for k in target_keys(opt):
            v = ret[k]
            if k in MAPS:
                flat = v.reshape(-1)
                nz = np.flatnonzero(flat)
                out[name + "/%s_idx" % k] = nz.astype(np.int32)
                out[name + "/%s_val" % k] = flat[nz]
            else:
                out[name + "/" + k] = v
        print("%-14s S=%-2d R=%-3d objects=%d kept=%d rot=%.2f flipped=%d" % (
            name, ret["ind"].shape[0], opt.output_res, int(recs["pt_image"][10]), int(ret["reg_mask"].sum()),
            float(recs["pt_image"][9]), int(recs["pt_image"][8])))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
