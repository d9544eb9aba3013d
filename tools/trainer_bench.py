"""Times one training iteration through lib.trains' trainer against the bare hand-written loop of INTEGRATION.md
("Training inputs": TrainInputs -> PoseTargets -> PoseNet -> ObjectPoseLoss -> optim.Adam) on the same pre-collated
batches: dla_34, B = 16, 512 x 512, head_conv 256 by default.

Each route owns a network and an optimizer from the same seeded state.  The batches are read once from a synthetic
data_dir (centerpose_amd.synth.write_dataset) and kept in memory, so neither route pays for decoding.  A window is
--steps iterations between two host clock readings, closed by the route's own end: the trainer's read-back of its meter,
a torch.cuda.synchronize() for the bare loop.  After a warm-up of each route the routes alternate round by round; every
round is reported, then the medians and their ratio.  The trainer adds one small accumulate per iteration (a stack of
the ten statistics and a float64 add) and nothing else, so the ratio is expected around 1.0.

  python tools/trainer_bench.py [--rounds 5] [--steps 20] [--warmup 3] [--batch 16] [--res 512] [--out profiles/trainer_bench.txt]
"""
import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from centerpose_amd import synth  # noqa: E402
from centerpose_amd.lib.datasets.dataset_combined import ObjectPoseDataset  # noqa: E402
from centerpose_amd.lib.datasets.dataset_factory import collate_fn_filtered  # noqa: E402
from centerpose_amd.lib.opts import opts  # noqa: E402
from centerpose_amd.lib.trains.train_factory import train_factory  # noqa: E402
from centerpose_amd.optim import Adam  # noqa: E402
from centerpose_amd.pose_loss import ObjectPoseLoss  # noqa: E402
from centerpose_amd.pose_net import PoseNet  # noqa: E402
from centerpose_amd.pose_targets import PoseTargets  # noqa: E402
from centerpose_amd.train_inputs import TrainInputs  # noqa: E402


def bare_loop(opt, net, optimizer, batches, parts):
    """The hand-written loop; not code under test."""
    inputs, targets, crit = parts
    for batch in batches:
        images = inputs(batch["frame"], batch["ti_image"])
        gt = targets(batch)
        out = net(images)
        loss, stats, _ = crit(out, gt, "train")
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--head_conv", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    o = opts()
    opt = o.parse(o.parser.parse_args(["--c", "chair", "--arch", "dla_34", "--input_res", str(a.res), "--head_conv", str(a.head_conv),
                                       "--batch_size", str(a.batch), "--num_workers", "0", "--debug", "0", "--obj_scale"]))
    scratch = tempfile.mkdtemp(prefix="centerpose_bench_")
    try:
        synth.write_dataset(scratch, a.batch, "chair", splits=("train",), size=(640, 480))
        opt.data_dir = scratch
        opt = o.update_dataset_info_and_set_heads(opt, ObjectPoseDataset)
        opt.device = dev
        np.random.seed(opt.seed)
        random.seed(opt.seed)
        loader = torch.utils.data.DataLoader(ObjectPoseDataset(opt, "train"), batch_size=a.batch, shuffle=False, num_workers=0,
                                             collate_fn=collate_fn_filtered)
        one = next(iter(loader))
    finally:
        shutil.rmtree(scratch, ignore_errors=True)

    def batches(n):  # the trainer adds its tensors to the dict it is given
        return [dict(one) for _ in range(n)]

    sd = synth.make_state_dict("dla_34", opt.heads, head_conv=a.head_conv)
    nets = {}
    for route in ("trainer", "bare"):
        net = PoseNet(opt.heads, a.head_conv, opt)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).train()
        nets[route] = (net, Adam(net.parameters(), opt.lr, max_grad_norm=100.))
    trainer = train_factory["object_pose"](opt, *nets["trainer"])
    trainer.set_device(opt.gpus, opt.chunk_sizes, dev)
    parts = (TrainInputs(opt), PoseTargets(opt), ObjectPoseLoss(opt))

    def run(route, n):
        t0 = time.perf_counter()
        if route == "trainer":
            opt.num_iters = n
            trainer.run_epoch("train", 1, batches(n))
        else:
            bare_loop(opt, *nets["bare"], batches(n), parts)
        return (time.perf_counter() - t0) * 1e3 / n

    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    emit(dict(what="trainer_bench", device=torch.cuda.get_device_name(0), torch=torch.__version__, arch="dla_34", batch=a.batch,
              res=a.res, head_conv=a.head_conv, rounds=a.rounds, steps=a.steps, warmup=a.warmup))
    for route in nets:
        run(route, a.warmup)
    times = {route: [] for route in nets}
    for r in range(a.rounds):
        for route in nets:
            ms = run(route, a.steps)
            times[route].append(ms)
            emit(dict(route=route, round=r, ms_per_iteration=round(ms, 3)))
    med = {route: statistics.median(v) for route, v in times.items()}
    for route in nets:
        emit(dict(route=route, summary="median of %d rounds" % a.rounds, ms_per_iteration=round(med[route], 3),
                  min_ms=round(min(times[route]), 3), max_ms=round(max(times[route]), 3)))
    emit(dict(summary="trainer / bare", ratio=round(med["trainer"] / med["bare"], 4)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
