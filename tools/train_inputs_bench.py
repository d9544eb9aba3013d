"""Times the device training inputs (cp_train_inputs via TrainInputs) against the host path at B = 32, 480 x 640 frames
-> 512 x 512, with and without colour augmentation, and writes the table to profiles/train_inputs_bench.txt (or --out).

  device     GPU events around each call on frames that are already on the device (the staging copy of the records + the
             grey kernel with colour + the apply kernel), the median of --iters calls after a warm-up, three frame /
             record sets rotated and the last three outputs kept alive, so that consecutive calls touch distinct buffers
  floor      the call's least traffic, the frames read once + 12 bytes written per output pixel, at 6.29 TB/s, the
             measured HBM copy rate of the MI355X (8 TB/s is the specification)
  host       the numpy restatement tests/train_inputs_ref.py (float32 mode) of the same batch, one thread
  H2D        a pinned host-to-device copy of the float32 result, which the device path no longer needs, against the copy
             of the 8-bit frames, which it does need

  python tools/train_inputs_bench.py [--iters 30] [--out profiles/train_inputs_bench.txt]
"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from centerpose_amd.lib.utils.image import get_affine_transform  # noqa: E402
from centerpose_amd.train_inputs import TrainInputs, draw_color_aug, pack_input  # noqa: E402
from tests import train_inputs_ref as R  # noqa: E402

COPY_RATE = 6.29e12  # bytes/s
NROT = 3


def median_ms(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(i)
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def make_set(seed, B, H, W, side, color):
    """B random frames and the records of the dataset's own augmentation draws (random centre, scale 0.6 - 1.4,
    rotation within 15 degrees for a quarter of the images, flip for half)."""
    rng, py = np.random.RandomState(seed), random.Random(seed)
    frames = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    recs = []
    for _ in range(B):
        c = np.array([rng.randint(W // 4, 3 * W // 4), rng.randint(H // 4, 3 * H // 4)], dtype=np.float32)
        s = max(H, W) * rng.choice(np.arange(0.6, 1.4, 0.1))
        rot = float(np.clip(rng.randn() * 15, -30, 30)) if rng.random_sample() < 0.25 else 0
        flipped = rng.random_sample() < 0.5
        if flipped:
            c[0] = W - c[0] - 1
        col = draw_color_aug(rng, py) if color else None
        recs.append(pack_input(get_affine_transform(c, s, rot, [side, side]), H, W, flipped, col)["ti_image"])
    return frames, np.stack(recs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_inputs_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_inputs_bench: no HIP device (there is no CPU timing of a device call)")
    B, H, W, side = args.batch, 480, 640, 512
    dev = torch.device("cuda:0")
    ti = TrainInputs(argparse.Namespace(new_data_augmentation=False, input_res=side))
    rows = []
    for color in (False, True):
        sets = [make_set(10 * s + color, B, H, W, side, color) for s in range(NROT)]
        dframes = [torch.from_numpy(f).to(dev) for f, _ in sets]
        keep = []

        def call(i):
            keep.append(ti(dframes[i % NROT], sets[i % NROT][1]))
            del keep[:-NROT]

        dev_ms = median_ms(call, args.iters)
        out = keep[-1]
        in_bytes, out_bytes = B * H * W * 3, out.numel() * 4
        t0 = time.perf_counter()
        ref = R.batch(list(sets[(args.iters - 1) % NROT][0]), sets[(args.iters - 1) % NROT][1], side, "f32")
        host_ms = (time.perf_counter() - t0) * 1e3
        diff = float(np.abs(out.cpu().numpy() - ref).max())  # the timed output is the restatement's (0 without colour)
        pin_out = [torch.empty(out.shape, dtype=torch.float32, pin_memory=True) for _ in range(NROT)]
        pin_in = [torch.from_numpy(f).pin_memory() for f, _ in sets]
        dst_out, dst_in = torch.empty_like(out), torch.empty_like(dframes[0])
        h2d_out = median_ms(lambda i: dst_out.copy_(pin_out[i % NROT], non_blocking=True), max(10, args.iters // 2))
        h2d_in = median_ms(lambda i: dst_in.copy_(pin_in[i % NROT], non_blocking=True), max(10, args.iters // 2))
        rows.append((color, in_bytes, out_bytes, dev_ms, (in_bytes + out_bytes) / COPY_RATE * 1e3, host_ms, h2d_out, h2d_in,
                     diff))
        print(rows[-1], flush=True)
    lines = ["TrainInputs (cp_train_inputs) at B = %d, %dx%d frames -> %dx%d, %d frame / record sets rotated; median of %d "
             "calls" % (B, H, W, side, side, NROT, args.iters),
             "device = GPU events around the call, frames already on the device (record staging + grey kernel with colour + "
             "apply kernel); floor = (frames read once + 12 bytes per output pixel) at 6.29 TB/s, the measured HBM copy rate; "
             "host = numpy restatement of the batch, one thread; H2D = pinned copies; max diff = the timed output against "
             "the float32 restatement",
             " colour |  frames MB  output MB |  device ms   floor ms |    host ms | H2D f32 out ms  H2D u8 frames ms | max diff"]
    for color, ib, ob, d, floor, h, ho, hi, diff in rows:
        lines.append("  %5s |  %9.1f  %9.1f |  %9.4f  %9.4f | %10.1f | %14.3f  %16.3f | %.3g"
                     % ("yes" if color else "no", ib / 1e6, ob / 1e6, d, floor, h, ho, hi, diff))
    lines.append("colour / no colour device time: %.2f" % (rows[1][3] / rows[0][3]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
