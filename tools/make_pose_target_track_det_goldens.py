"""Writes tests/golden/pose_targets_track_det_ref.npz: the reference's own ObjectPoseDataset.__getitem__ with
opt.tracking_task on and data_generation_mode_ratio = 1.0 (every sample takes the previous frame from the detector), on
the cases of tests/pose_target_track_det_cases.py.

Runs only where the reference project exists ($CENTERPOSE_REFERENCE, as the other make_*_goldens.py).  The dataset
module is imported unmodified with the stubs and the draw shims of tools/make_pose_target_track_goldens.py; its
``detector`` is a stub whose run() returns the boxes that the stored cp_postprocess / cp_pnp_from_post rows amount to.

  python tools/make_pose_target_track_det_goldens.py

Contents, per case <c> (B = 1, arrays without the batch axis):
  <c>/pt_image ... <c>/ptk_cur_objects, <c>/ptk_gen, <c>/ptk_det_meta   the packed records
  <c>/det_post [K, 120], <c>/det_count, <c>/det_pnp [K, 40]             the detector's rows
  <c>@0/...                                    the cases of DC.MODE0 once more in the noise-simulation mode (ptk_gen mode 0)
  <c>/<key>                                    every non-map key of the reference's ret
  <c>/<map>_idx int32, <c>/<map>_val float32   hm / hm_hp / pre_hm / pre_hm_hp as non-zero (flat index, value) pairs
"""
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "pose_targets_track_det_ref.npz")

from centerpose_amd.pose_targets_track import track_target_keys  # noqa: E402
from tests import pose_target_cases as PC  # noqa: E402
from tests import pose_target_track_det_cases as DC  # noqa: E402

MAPS = ("hm", "hm_hp", "pre_hm", "pre_hm_hp")


def main():
    if not PC.reference_available():
        raise SystemExit("the reference tree is not present ($CENTERPOSE_REFERENCE)")
    out = {}
    for name, mode in [(n, 1) for n in DC.CASES] + [(n, 0) for n in DC.MODE0]:
        opt, recs, (post, count, pnp), ret = DC.golden_case(name, mode)
        name = name if mode else name + "@0"
        for k, v in recs.items():
            out[name + "/" + k] = v
        out[name + "/det_post"], out[name + "/det_count"], out[name + "/det_pnp"] = post, np.int32(count), pnp
        for k in track_target_keys(opt):
            v = ret[k]
            if k in MAPS:
                flat = v.reshape(-1)
                nz = np.flatnonzero(flat)
                out[name + "/%s_idx" % k] = nz.astype(np.int32)
                out[name + "/%s_val" % k] = flat[nz]
            else:
                out[name + "/" + k] = v
        print("%-14s S=%-2d previous=%d slots=%d pre_hm>0=%d pre_hm_hp>0=%d tracked=%d flipped=%d" % (
            name, ret["ind"].shape[0], int(recs["ptk_image"][6]), count, int((ret["pre_hm"] > 0).sum()),
            int((ret["pre_hm_hp"] > 0).sum()), int(ret["tracking_mask"].sum()), int(recs["pt_image"][8])))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
