"""Times the device targets of the tracking task (cp_pose_targets_track via TrackPoseTargets) against the host path at
B = 32, 512 x 512 input (output 128 x 128), 8 joints, S = 1 and 4, and writes the table to
profiles/pose_targets_track_bench.txt (or --out).

  device     GPU events around each TrackPoseTargets call (the staging copies of the records + the four kernels), the
             median of --iters calls after a warm-up, three record sets rotated and the last three outputs kept alive,
             so that consecutive calls write distinct buffers
  no pre     the same call with pre_hm and pre_hm_hp off: the records, both objects kernels and the current frame's
             maps, i.e. everything but the previous-frame map writer; "pre maps" is the difference of the two medians
  current    cp_pose_targets alone (PoseTargets) on the same current-frame records
  floor      the previous-frame maps' bytes (B x 9 x 512 x 512 x 4 = 302 MB) at 6.29 TB/s, the HBM copy rate the README
             measures
  host       the numpy restatement tests/pose_targets_track_ref.py, one thread, per batch
  H2D        a pinned host-to-device copy of the same tensors (what a host-built batch pays after it is built)

  python tools/pose_targets_track_bench.py [--iters 30] [--out profiles/pose_targets_track_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from centerpose_amd.pose_targets import PoseTargets, num_symmetry  # noqa: E402
from centerpose_amd.pose_targets_track import TrackPoseTargets  # noqa: E402
from tests import pose_target_cases as PC  # noqa: E402
from tests import pose_target_track_cases as TC  # noqa: E402
from tests.test_pose_targets_track_cpu import random_records, restate  # noqa: E402
from tools.pose_targets_bench import COPY_RATE, NROT, median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pose_targets_track_bench.txt"))
    ap.add_argument("--sizes", default="1,4", help="the S values to time (a profiler run takes one)")
    args = ap.parse_args()
    B, inp, Rr = 32, 512, 128
    rows = []
    for S in (int(v) for v in args.sizes.split(",")):
        cat = {1: "camera", 4: "chair"}.get(S, "bottle")
        over = dict(c=cat, num_symmetry=S, input_res=inp, input_w=inp, input_h=inp, output_res=Rr)
        opt = TC.make_opt(over)
        assert num_symmetry(opt) == S
        rng = np.random.default_rng(S)
        sets = [random_records(rng, B, opt) for _ in range(NROT)]
        keep = []

        def timed(target, records):
            def call(i):
                keep.append(target(records[i % NROT]))
                del keep[:-NROT]

            return median_ms(call, args.iters)

        nopre_ms = timed(TrackPoseTargets(TC.make_opt(over, pre_hm=False, pre_hm_hp=False)), sets)
        cur_ms = timed(PoseTargets(PC.make_opt(dict(c=cat, num_symmetry=S, output_res=Rr))), sets)
        dev_ms = timed(TrackPoseTargets(opt), sets)
        out = keep[-1]
        nbytes = sum(t.numel() * t.element_size() for t in out.values())
        pre_bytes = sum(out[k].numel() * 4 for k in ("pre_hm", "pre_hm_hp"))
        t0 = time.perf_counter()
        ref = restate(sets[0], opt)
        host_ms = (time.perf_counter() - t0) * 1e3
        pinned = [{k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in out.items()} for _ in range(NROT)]
        dst = {k: torch.empty_like(v) for k, v in out.items()}

        def h2d(i):
            for k, v in pinned[i % NROT].items():
                dst[k].copy_(v, non_blocking=True)

        h2d_ms = median_ms(h2d, max(10, args.iters // 2))
        kept = sum(q["kept"] for im in ref["pre"] for q in im)
        rows.append((S, nbytes, pre_bytes, dev_ms, nopre_ms, cur_ms, pre_bytes / COPY_RATE * 1e6, host_ms, h2d_ms, kept,
                     int(ref["tracking_mask"].sum())))
        print(rows[-1], flush=True)
    lines = ["TrackPoseTargets (cp_pose_targets_track) at B = %d, %dx%d input, %dx%d output, 8 joints, 10 + 10 object "
             "slots, every output on; %d record sets rotated; median of %d calls" % (B, inp, inp, Rr, Rr, NROT, args.iters),
             "device = GPU events around the call; no pre = pre_hm / pre_hm_hp off; pre maps = device - no pre; current = "
             "cp_pose_targets alone; floor = the previous-frame maps' bytes at 6.29 TB/s; host = numpy restatement per "
             "batch, one thread; H2D = pinned copy of the same tensors",
             "   S |  output MB  pre-map MB |  device ms  no pre ms  pre maps us  floor us  current ms |   host ms |"
             "    H2D ms | previous kept  tracked"]
    for S, nb, pb, d, npre, cur, floor, h, c, kept, tracked in rows:
        lines.append("  %2d |  %9.1f  %10.1f |  %9.4f  %9.4f  %11.1f  %8.1f  %10.4f | %9.1f | %9.3f | %13d  %7d"
                     % (S, nb / 1e6, pb / 1e6, d, npre, (d - npre) * 1e3, floor, cur, h, c, kept, tracked))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
