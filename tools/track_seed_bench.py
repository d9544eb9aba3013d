"""Times the CenterPoseTrack loop of ``BatchedTracking`` with and without seeding from annotations: B = 16 concurrent
videos, 512 x 512 input, the stub network of oracle/tools/track_golden.py (its five seeded head frames, cycled, already on
the device -- so a step is render of the previous maps + decode + post-process + PnP + tracker, and what seeding adds is
not hidden behind a backbone), seeds of tests/track_seed_cases.py (six per video, five of them accepted).

Configurations, alternated inside every round in one process:
  device / unseeded        ``device_tracker=True`` without seeds or flags: the loop as it was before seeding existed
  device / gt_first        --gt_pre_hm_hmhp_first: seeds + ground-truth maps on frame 0 (inside the warm-up), nothing after
  device / gt_every        --gt_pre_hm_hmhp: every frame packs 16 seed lists on the host, copies them and launches cp_track_seed
  host   / gt_first        the same two modes on the reference-shaped Python tracker (``device_tracker=False``)
  host   / gt_every
Frames/s = B * frames / wall clock, the host clock around a final synchronise, after --warmup frames; ``meta['id']`` counts
up, so only frame 0 is "the first".  The median of the rounds is reported; for device / gt_every the host time spent in
``hip.pack_seeds`` and in ``DeviceTracker.seed`` (staging, copy, launch: enqueue only) is given per step as well.

  python tools/track_seed_bench.py [--frames 120] [--rounds 3] [--out profiles/track_seed_bench.txt]
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from centerpose_amd import hip  # noqa: E402
from centerpose_amd.lib.detectors import base_detector as bd  # noqa: E402
from centerpose_amd.lib.detectors.batch_tracking import BatchedTracking  # noqa: E402
from centerpose_amd.lib.detectors.object_pose import ObjectPoseDetector  # noqa: E402
from centerpose_amd.lib.opts import opts  # noqa: E402
from centerpose_amd.lib.utils.image import get_affine_transform  # noqa: E402
from oracle.tools import track_golden as tg  # noqa: E402
from tests import track_seed_cases as sc  # noqa: E402

B = 16
CONFIGS = [("device", "unseeded"), ("device", "gt_first"), ("device", "gt_every"), ("host", "gt_first"), ("host", "gt_every")]


class Engine(object):
    """The stub network for B videos: the video's head frames, sigmoid applied, resident on the device."""

    def __init__(self, heads, device):
        self.frames, self.calls = [], 0
        for h in heads:
            self.frames.append({k: (torch.sigmoid(v) if k in ("hm", "hm_hp") else v).repeat(B, 1, 1, 1).contiguous().to(device)
                                for k, v in h.items()})

    def forward(self, images, pre_images=None, pre_hms=None, pre_hm_hp=None, sigmoid_hm=True):
        out = dict(self.frames[self.calls % len(self.frames)])   # (the decode thresholds hm in place: hand it a copy)
        out["hm"], out["hm_hp"] = out["hm"].clone(), out["hm_hp"].clone()
        self.calls += 1
        return out


def make_detector(mode, engine):
    stub = tg.StubNetwork([])
    bd.create_model = lambda *a, **k: stub
    bd.load_model = lambda m, *a, **k: m
    argv = [a if a != "-1" else "0" for a in tg.TRACK_ARGV] + (sc.MODES[mode] if mode in sc.MODES else [])
    with contextlib.redirect_stdout(io.StringIO()):
        o = opts().parser.parse_args(argv)
        o = opts().init(opts().parse(tg.demo_flags(o)))
        det = ObjectPoseDetector(o)
    stub._engine = lambda: engine
    return det


def run(det, engine, tracker, mode, images, meta, labels, frames, warmup):
    """-> (frames/s, host ms per step in pack_seeds, host ms per step in DeviceTracker.seed)"""
    bt = BatchedTracking(det, B, device_tracker=(tracker == "device"))
    engine.calls = 0
    spent = {"pack": 0.0, "seed": 0.0}
    real_pack, real_seed = hip.pack_seeds, hip.DeviceTracker.seed

    def timed(name, fn):
        def wrapper(*a, **k):
            t = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                spent[name] += time.perf_counter() - t
        return wrapper

    hip.pack_seeds, hip.DeviceTracker.seed = timed("pack", real_pack), timed("seed", real_seed)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            for f in range(warmup + frames):
                if f == warmup:
                    torch.cuda.synchronize()
                    spent["pack"] = spent["seed"] = 0.0
                    t0 = time.perf_counter()
                metas = []
                for b in range(B):
                    m = dict(meta, id=f)
                    if mode == "gt_every" or (mode == "gt_first" and f == 0):
                        m["pre_dets"] = labels[max(f - 1, 0) % len(labels)][b]   # the evaluator hands the same dicts on
                    metas.append(m)
                bt.step(images, metas, read=(tracker == "host"))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    finally:
        hip.pack_seeds, hip.DeviceTracker.seed = real_pack, real_seed
    if tracker == "device":
        bt.dev.check()
        assert all(len(a) >= 2 for a in bt.dev.read())
    return B * frames / dt, spent["pack"] / frames * 1e3, spent["seed"] / frames * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120, help="timed frames per configuration and round")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_seed_bench.txt"))
    args = ap.parse_args()
    device = torch.device("cuda:0")
    engine = Engine(tg.video_heads(), device)
    img, meta = tg.frame_inputs(get_affine_transform)[0]
    images = torch.from_numpy(img)[None].repeat(B, 1, 1, 1).to(device)
    labels = [[sc.annotations(f) for _ in range(B)] for f in range(tg.N_FRAMES)]
    dets = {mode: make_detector(mode, engine) for mode in ("unseeded", "gt_first", "gt_every")}
    res = {c: [] for c in CONFIGS}
    for r in range(args.rounds):
        for tracker, mode in (CONFIGS if r % 2 == 0 else CONFIGS[::-1]):
            res[(tracker, mode)].append(run(dets[mode], engine, tracker, mode, images, meta, labels, args.frames, args.warmup))
    lines = ["BatchedTracking, B = %d videos, 512 x 512, stub network, %s" % (B, torch.cuda.get_device_name(0)),
             "%d rounds x %d timed frames per configuration (after %d warm-up frames, frame 0 among them), alternated; "
             "median of the rounds" % (args.rounds, args.frames, args.warmup), "",
             "%-8s %-10s %12s %12s %18s %18s" % ("tracker", "mode", "frames/s", "ms/step", "pack_seeds ms/step", "seed() ms/step")]
    for c in CONFIGS:
        fps = statistics.median(x[0] for x in res[c])
        pack, seed = statistics.median(x[1] for x in res[c]), statistics.median(x[2] for x in res[c])
        lines.append("%-8s %-10s %12.1f %12.3f %18.3f %18.3f" % (c[0], c[1], fps, B / fps * 1e3, pack, seed))
    lines += ["", "rounds (frames/s): " + "; ".join("%s/%s %s" % (c[0], c[1], " ".join("%.0f" % x[0] for x in res[c]))
                                                     for c in CONFIGS)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
