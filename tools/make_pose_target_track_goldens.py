"""Writes tests/golden/pose_targets_track_ref.npz: the reference's own ObjectPoseDataset.__getitem__ with
opt.tracking_task on, on the synthetic two-frame cases of tests/pose_target_track_cases.py.

Runs only where the reference project exists ($CENTERPOSE_REFERENCE, as the other make_*_goldens.py).  The dataset
module is imported unmodified with the stubs of tools/make_pose_target_goldens.py and a one-video ds.videos; inside it,
np.random.random / randn / uniform / choice and stats.truncnorm(...).rvs are replaced by shims that return, for the
calling line, idx_obj and j, the slot of the packed draws (pose_target_track_cases._Shims), so the reference consumes
exactly the numbers the records carry; every other draw (frame choice, augmentation, flip) comes from the seeded
generator.

  python tools/make_pose_target_track_goldens.py

Contents, per case <c> (B = 1, arrays without the batch axis):
  <c>/pt_image, <c>/pt_objects, <c>/ptk_image, <c>/ptk_pre_objects, <c>/ptk_cur_objects   the packed records
  <c>/<key>                                    every non-map key of the reference's ret
  <c>/<map>_idx int32, <c>/<map>_val float32   hm / hm_hp / pre_hm / pre_hm_hp as non-zero (flat index, value) pairs
"""
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "pose_targets_track_ref.npz")

from centerpose_amd.pose_targets_track import track_target_keys  # noqa: E402
from tests import pose_target_cases as PC  # noqa: E402
from tests import pose_target_track_cases as TC  # noqa: E402

MAPS = ("hm", "hm_hp", "pre_hm", "pre_hm_hp")


def main():
    if not PC.reference_available():
        raise SystemExit("the reference tree is not present ($CENTERPOSE_REFERENCE)")
    out = {}
    for name in TC.CASES:
        opt, recs, ret = TC.golden_case(name)
        for k, v in recs.items():
            out[name + "/" + k] = v
        for k in track_target_keys(opt):
            v = ret[k]
            if k in MAPS:
                flat = v.reshape(-1)
                nz = np.flatnonzero(flat)
                out[name + "/%s_idx" % k] = nz.astype(np.int32)
                out[name + "/%s_val" % k] = flat[nz]
            else:
                out[name + "/" + k] = v
        print("%-14s S=%-2d R=%-3d objects=%d previous=%d kept=%d tracked=%d rot=%.2f flipped=%d" % (
            name, ret["ind"].shape[0], opt.output_res, int(recs["pt_image"][10]), int(recs["ptk_image"][6]),
            int(ret["reg_mask"].sum()), int(ret["tracking_mask"].sum()), float(recs["pt_image"][9]),
            int(recs["pt_image"][8])))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
