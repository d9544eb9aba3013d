"""Times the device ObjectPose targets (cp_pose_targets via PoseTargets) against the host path at B = 32, 8 joints,
128 x 128, S = 1, 4 and 12, and writes the table to profiles/pose_targets_bench.txt (or --out).

  device     GPU events around each PoseTargets call (the staging copy of the records + both kernels), the median of
             --iters calls after a warm-up, three record sets rotated and the last three outputs kept alive, so that
             consecutive calls write distinct buffers
  GB/s       the bytes of the returned tensors over the device time; the floor is those bytes at 6.29 TB/s, the HBM
             copy rate the README measures
  host       the numpy restatement tests/pose_targets_ref.py, one thread, per batch (the reference's own per-image
             drawing and stacking are in the issue's table; the restatement is of the same order)
  H2D        a pinned host-to-device copy of the same tensors (what a host-built batch pays after it is built)

  python tools/pose_targets_bench.py [--iters 30] [--out profiles/pose_targets_bench.txt]
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
from tests import pose_target_cases as PC  # noqa: E402
from tests import pose_targets_ref as R  # noqa: E402
from tests.test_pose_targets_cpu import random_records  # noqa: E402

COPY_RATE = 6.29e12  # bytes/s
NROT = 3


def median_ms(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for _ in range(3):
        fn(0)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(i)
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pose_targets_bench.txt"))
    ap.add_argument("--sizes", default="1,4,12", help="the S values to time (a profiler run takes one)")
    args = ap.parse_args()
    B, Rr = 32, 128
    rows = []
    for S in (int(v) for v in args.sizes.split(",")):
        cat = {1: "camera", 4: "chair"}.get(S, "bottle")
        opt = PC.make_opt(dict(c=cat, num_symmetry=S, output_res=Rr))
        assert num_symmetry(opt) == S
        pt = PoseTargets(opt)
        rng = np.random.default_rng(S)
        sets = [random_records(rng, B, S, Rr, cat) for _ in range(NROT)]
        recs = [{"pt_image": torch.from_numpy(i), "pt_objects": torch.from_numpy(o)} for i, o in sets]
        keep = []

        def call(i):
            keep.append(pt(recs[i % NROT]))
            del keep[:-NROT]

        dev_ms = median_ms(call, args.iters)
        out = keep[-1]
        nbytes = sum(t.numel() * t.element_size() for t in out.values())
        t0 = time.perf_counter()
        R.batch_targets(sets[0][0], sets[0][1], S, Rr)
        host_ms = (time.perf_counter() - t0) * 1e3
        pinned = [{k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in out.items()} for _ in range(NROT)]
        dst = {k: torch.empty_like(v) for k, v in out.items()}

        def h2d(i):
            for k, v in pinned[i % NROT].items():
                dst[k].copy_(v, non_blocking=True)

        h2d_ms = median_ms(h2d, max(10, args.iters // 2))
        rows.append((S, nbytes, dev_ms, nbytes / dev_ms / 1e6, nbytes / COPY_RATE * 1e6, host_ms, h2d_ms,
                     int(sum(int(o["reg_mask"].sum()) for o in keep[-1:]))))
        print(rows[-1], flush=True)
    lines = ["PoseTargets (cp_pose_targets) at B = %d, 8 joints, %dx%d, hm_hp + hp_offset + scale + wh + reg on, "
             "%d record sets rotated; median of %d calls" % (B, Rr, Rr, NROT, args.iters),
             "device = GPU events around the call (record staging + objects kernel + maps kernel); floor = output bytes "
             "at 6.29 TB/s; host = numpy restatement per batch, one thread; H2D = pinned copy of the same tensors",
             "   S |   output MB |  device ms     GB/s   floor us |   host ms |    H2D ms | objects kept"]
    for S, nb, d, gbs, floor, h, c, kept in rows:
        lines.append("  %2d |  %10.1f |  %9.4f  %7.0f  %9.1f | %9.1f | %9.3f | %d" % (S, nb / 1e6, d, gbs, floor, h, c,
                                                                                  kept))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
