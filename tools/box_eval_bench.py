"""One cp_box_eval launch over N matched pairs at num_symmetry rotations (default 4096 x 100, the reference's
eval_num_symmetry), after one warm-up launch: run it under `rocprofv3 --kernel-trace --stats` for box_eval_kernel's
device time.

  rocprofv3 --kernel-trace --stats -d build/prof -o box -- python tools/box_eval_bench.py [N] [num_symmetry]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from centerpose_amd import hip  # noqa: E402
from tools.make_box_eval_goldens import box, gl_projection, mo2c, object_pose, project, rot  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    nsym = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    rng = np.random.RandomState(1)
    P = gl_projection()
    pr, gt, p2, M = [], [], [], []
    for _ in range(n):
        R, t, s = object_pose(rng)
        gt.append(box(R, t, s))
        M.append(mo2c(R, t))
        pr.append(box(R @ rot([0, 1, 0], rng.uniform(-np.pi, np.pi)), t + rng.randn(3) * 0.03,
                      s * rng.uniform(0.9, 1.1, 3)))
        p2.append(project(P, gt[-1]) + rng.randn(9, 2) * 0.004)
    args = (np.array(pr), np.array(gt), np.array(p2), np.array(M), np.repeat(P[None], n, 0), np.zeros(n, np.int32))
    hip.box_eval(*args, nsym)  # warm-up (module load)
    torch.cuda.synchronize()
    t0 = time.time()
    out = hip.box_eval(*args, nsym)
    t1 = time.time()
    print("box_eval: %d pairs x %d rotations, %.2f ms wall (upload + launch + read-back), mean IoU %.4f, flags %d"
          % (n, nsym, (t1 - t0) * 1e3, out[:, 0].mean(), int((out[:, 8] != 0).sum())))


if __name__ == "__main__":
    main()
