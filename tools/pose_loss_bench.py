"""Times the device ObjectPoseLoss (cp_pose_loss_forward / _backward) against the torch restatement (tests/pose_loss_ref.py,
float32) on the same GPU, at B = 16 and 32, S = 1, 4 and 12, 8 joints, 128 x 128, every head on.

Rates are over the algorithmic bytes: forward = read the logits and every ground-truth slice once, write the sigmoid and
the clamped maps; backward = read the sigmoid and the chosen slice, write the heat-map gradients, zero-fill the dense
regression gradients.  The ground truth at B = 32, S = 12 (226 MB) fits in the 256 MiB Infinity Cache, so three distinct
batches are rotated and the rate reported is the HBM rate of that rotation.

  python tools/pose_loss_bench.py [--iters 20] [--quick]       (--quick: B = 32, S = 12 only, a few iterations)
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from centerpose_amd import hip  # noqa: E402
from centerpose_amd.pose_loss import loss_config  # noqa: E402
from tests import pose_loss_cases as PC  # noqa: E402
from tests import pose_loss_ref as R  # noqa: E402

PEAK = 6.0e12  # bytes/s, streaming ceiling (MI355X_MICROARCH.md)
NROT = 3


def timed(fn, iters):
    fn(0)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for i in range(iters):
        fn(i)
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    opt = PC.make_opt({})
    terms, flags, weights = loss_config(opt, "train")
    res, J = 128, 8
    shapes = [(32, 12)] if a.quick else [(16, 1), (16, 4), (16, 12), (32, 1), (32, 4), (32, 12)]
    iters = 3 if a.quick else a.iters
    print("ObjectPoseLoss, %d joints, %dx%d, all heads; %d distinct batches rotated; times per call (ms)" % (J, res, res, NROT))
    print("%4s %3s | %9s %9s %7s | %9s %9s %7s | %11s %9s" % ("B", "S", "fwd", "GB/s", "%peak", "bwd", "GB/s", "%peak",
                                                             "torch f+b", "speedup"))
    for B, S in shapes:
        rng = np.random.default_rng(B * 100 + S)
        batches = [{k: torch.from_numpy(v).to(dev) for k, v in PC.make_batch(rng, B, S, res, J).items()}
                   for _ in range(NROT)]
        outputs = PC.make_outputs(rng, opt, B, res, J)
        heads = [{k: torch.from_numpy(v).to(dev) for k, v in outputs[0].items()}]
        hm_px = B * (1 + J) * res * res
        fwd_bytes = 4 * (hm_px * 3 + hm_px * S)
        reg_ch = 2 * J + 2 + 2 + 3 + 2
        bwd_bytes = 4 * (hm_px * 3 + B * reg_ch * res * res)
        state = {}

        def fwd(i):
            state["r"] = hip.pose_loss_forward(heads, batches[i % NROT], terms, flags, weights)

        tf = timed(fwd, iters)
        dl = torch.ones(1, device=dev)

        def bwd(i):
            hip.pose_loss_backward(state["r"][5], dl)

        tb = timed(bwd, iters)

        def ref(i):
            o = [{k: v.detach().requires_grad_() for k, v in heads[0].items()}]
            R.object_pose_loss(opt, o, batches[i % NROT], "train")["loss"].backward()

        tr = timed(ref, max(2, iters // 4))
        print("%4d %3d | %9.4f %9.0f %6.1f%% | %9.4f %9.0f %6.1f%% | %11.3f %8.1fx" % (
            B, S, tf, fwd_bytes / tf / 1e6, 100 * fwd_bytes / (tf * 1e-3) / PEAK,
            tb, bwd_bytes / tb / 1e6, 100 * bwd_bytes / (tb * 1e-3) / PEAK, tr, tr / (tf + tb)))
        del batches, heads, state
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
