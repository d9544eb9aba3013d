"""Writes tests/golden/train_inputs_ref.npz: the reference's own ObjectPoseDataset._get_input output for four of the
cases of tests/train_input_cases.py at side 36, with the frame and the packed record of the same draws, so that the
tests read nothing but the file.  cv2 is stubbed as tests/train_input_cases.py states.  Needs the reference tree
($CENTERPOSE_REFERENCE).

  python tools/make_train_input_goldens.py
"""
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from centerpose_amd import hip  # noqa: E402
from tests import train_input_cases as TC  # noqa: E402

SIDE = 36


def main():
    if not TC.reference_available():
        raise SystemExit("the reference tree is not present at %s" % TC.REF)
    I = hip.TI_IMG
    data = {}
    with TC.reference_modules() as (_, ObjectPoseDataset):
        for i, key in enumerate(TC.GOLDEN_CASES):
            name, n = key.split("/")
            frames, recs, _ = TC.batch(name, SIDE)
            f, r = frames[int(n)], recs[int(n)]
            trans = r[I["trans"]:I["trans"] + 6].reshape(2, 3)
            out, rec = TC.reference_get_input(ObjectPoseDataset, f, trans, bool(r[I["flipped"]]), SIDE,
                                              1000 + i if r[I["color"]] else None)
            assert out.dtype == np.float32 and out.shape == (3, SIDE, SIDE)
            data[key + "/frame"], data[key + "/ti_image"], data[key + "/out"] = f, rec, out
    path = os.path.join(REPO, "tests", "golden", "train_inputs_ref.npz")
    np.savez_compressed(path, **data)
    print("wrote %s: %d bytes, cases %s" % (path, os.path.getsize(path), ", ".join(TC.GOLDEN_CASES)))


if __name__ == "__main__":
    main()
