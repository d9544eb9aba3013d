"""Writes tests/golden/dataset_ref.npz: what the reference's own ObjectPoseDataset.__getitem__ draws on the cases of
tests/dataset_cases.py, so that lib.datasets is compared with it where the reference project is absent.

Runs only where the reference project exists ($CENTERPOSE_REFERENCE, as the other make_*_goldens.py).  The dataset
module is imported unmodified through tests/pose_target_cases.run_reference (and pose_target_track_cases.run_reference
for the two-frame cases) with the captures tests/dataset_cases.py adds around them.

  python tools/make_dataset_goldens.py

Contents, per case <c>:
  <c>/trans_input [2, 3], <c>/trans_output_rot [2, 3]   the affines of the reference's draw (two-frame cases:
                                                        <c>/trans_input_pre as well)
  <c>/scalars [4]                                       rot, flipped, width, height
  <c>/color [7] or [0]                                  order code, the three alphas, the three lighting normals; empty
                                                        when color_aug did not run (<c>/color_pre: the previous frame's)
  <c>/states [3]                                        SHA-256 of the states of np.random, random and _data_rng after the
                                                        call (two-frame cases: where the noise draws begin)
"""
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from tests import dataset_cases as DC  # noqa: E402
from tests import pose_target_cases as PC  # noqa: E402


def main():
    if not PC.reference_available():
        raise SystemExit("the reference tree is not present ($CENTERPOSE_REFERENCE)")
    out = {}
    for name in DC.CASES:
        cap = DC.reference_run(name)
        DC.to_golden(out, name, cap)
        print("%-20s rot=%7.2f flipped=%d color=%s %dx%d" % (name, cap["rot"], cap["flipped"], cap["color"] is not None,
                                                             cap["width"], cap["height"]))
    for name in DC.TRACK_CASES:
        cap = DC.reference_track_run(name)
        DC.to_golden(out, name, cap)
        same = np.array_equal(cap["trans_input"], cap["trans_input_pre"])
        print("%-20s rot=%7.2f flipped=%d color=%s same affine=%s" % (name, cap["rot"], cap["flipped"], cap["color"] is not None,
                                                                     same))
    np.savez_compressed(DC.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (DC.GOLDEN, os.path.getsize(DC.GOLDEN)))


if __name__ == "__main__":
    main()
