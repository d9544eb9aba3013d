"""ORACLE tooling (build container only): the REFERENCE's ``ObjectPoseDetector.run`` on the 5-frame stub video of
oracle/tools/track_golden.py with ``meta['pre_dets']`` on the frames its evaluator gives them
(tools/objectron_eval/eval_video_official.py:327-456) -> tests/golden/track_run_seeded.json.

Three runs, the flag sets of the reference's tracking benchmark (shell_eval_video_CenterPoseTrack.py) on top of
``TRACK_ARGV``: ``--gt_pre_hm_hmhp_first`` (seeds and ground-truth maps on frame 0), ``--gt_pre_hm_hmhp`` (every frame) and
``--gt_pre_hm_hmhp_first --empty_pre_hm`` (seeds on frame 0, zero maps throughout).  What is real and what is
substituted when the reference runs is listed in oracle/tools/track_golden.py, whose ``reference_detector`` and
``summarise`` are used as they are; the seeds are tests/track_seed_cases.py.  Only recorded results are written.

    python tools/make_track_seed_goldens.py
"""
import contextlib
import io
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle.tools import track_golden as tg  # noqa: E402
from tests import track_seed_cases as sc  # noqa: E402


def main():
    out = {}
    for mode, extra in sc.MODES.items():
        argv = tg.TRACK_ARGV + extra
        det, gat = tg.reference_detector(argv)
        with contextlib.redirect_stdout(io.StringIO()):
            frames = sc.run_video(det, gat, mode)
        out[mode] = {"argv": argv, "frames": frames}
        print(mode, "tracks per frame", [len(x["tracks"]) for x in frames], "boxes", [x["n_boxes"] for x in frames],
              "ids", [[t["tracking_id"] for t in x["tracks"]] for x in frames],
              "pre_hm_hp pixels", [x["pre_hm_hp_nonzero"] for x in frames])
    with open(os.path.join(tg.GOLD, "track_run_seeded.json"), "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
