"""Trains a CenterPose network with lib.datasets and lib.trains: the project's training entry point.

  python tools/train.py --c chair --arch dla_34 --batch_size 16 --num_epochs 140 --lr_step 90,120 [lib.opts flags]
  python tools/train.py --synthetic 64 --input_res 128 --num_epochs 3 --batch_size 4 --print_iter 1

It parses lib.opts (with ``--debug`` defaulting to 0 here: the flag's value 1 forces batch size 1), creates the model,
builds ``centerpose_amd.optim.Adam(model.parameters(), opt.lr, max_grad_norm=100.)`` (the clip of the reference's step
folded into the update), loads ``--load_model`` (``--resume`` continues its optimizer and epoch), and runs the epoch loop
of the reference's main: ``<c>_last.pth`` after every epoch, a validation pass at batch size 1 every ``--val_intervals``
epochs that keeps ``<c>_best.pth`` by ``--metric``, ``<c>_<epoch>.pth`` and a tenfold drop of the learning rate at each
``--lr_step`` epoch (lr = opt.lr * 0.1 ** (number of milestones reached)).

Flags of its own:
  --data_dir DIR            where ``outf/<c>_<split>`` (``outf_all`` for --tracking_task) lies; default lib.opts' data_dir
  --out_dir DIR             where the checkpoints, opt.txt and log.txt go; default lib.opts' save_dir
  --synthetic N             write an N-frame synthetic set (centerpose_amd.synth.write_dataset: PNG frames and projected
                            cuboids, two videos) into a temporary data_dir, train on it, remove it
  --synthetic_size WxH      its frame size (default 160x120)
  --backward_precision P    f32 (default) or f16x3: the four set_backward_precision switches (conv, deconv, heads, DCN)
  --deterministic           hip.set_deterministic(True): bit-reproducible steps
  --no_shuffle              keep the training loader in dataset order
  --track_detector PATH     the dlav1_34 checkpoint of the detector that --data_generation_mode_ratio > 0 runs on the
                            previous frame (TrackPoseTargets(opt, detector=...))
"""
import os
import random
import shutil
import sys
import tempfile

import numpy as np
import torch
import torch.utils.data

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from centerpose_amd import conv, deconv, hip, pose_heads, synth  # noqa: E402
from centerpose_amd.lib.datasets.dataset_combined import ObjectPoseDataset  # noqa: E402
from centerpose_amd.lib.datasets.dataset_factory import collate_fn_filtered  # noqa: E402
from centerpose_amd.lib.logger import Logger  # noqa: E402
from centerpose_amd.lib.models.model import create_model, load_model, save_model  # noqa: E402
from centerpose_amd.lib.models.networks.DCNv2 import dcn_v2  # noqa: E402
from centerpose_amd.lib.opts import opts  # noqa: E402
from centerpose_amd.lib.trains.train_factory import train_factory  # noqa: E402
from centerpose_amd.optim import Adam  # noqa: E402


def parse(argv=None):
    o = opts()
    p = o.parser
    p.set_defaults(debug=0)
    p.add_argument("--data_dir", default=None)
    p.add_argument("--out_dir", default=None)
    p.add_argument("--synthetic", type=int, default=0)
    p.add_argument("--synthetic_size", default="160x120")
    p.add_argument("--backward_precision", default="f32", choices=["f32", "f16x3"])
    p.add_argument("--deterministic", action="store_true")
    p.add_argument("--no_shuffle", action="store_true")
    p.add_argument("--track_detector", default="")
    args = p.parse_args(argv)
    data_dir, out_dir = args.data_dir, args.out_dir
    opt = o.parse(args)
    if data_dir:
        opt.data_dir = data_dir
    if out_dir:
        opt.save_dir, opt.debug_dir = out_dir, os.path.join(out_dir, "debug")
    return o, opt


def track_detector(opt, path):
    """The detector of dataset_combined.py:144-154: dlav1_34 without pre_img, on the flags' defaults."""
    o = opts()
    d = o.parser.parse_args([])
    d.c, d.debug, d.pre_img, d.arch, d.use_pnp, d.rep_mode, d.obj_scale = opt.c, 0, False, "dlav1_34", True, 1, True
    d = o.init(o.parse(d))
    model = load_model(create_model(d.arch, d.heads, d.head_conv, d), path)
    return model.to(opt.device), d


def main(argv=None):
    o, opt = parse(argv)
    torch.manual_seed(opt.seed)
    np.random.seed(opt.seed)
    random.seed(opt.seed)
    if opt.deterministic:
        hip.set_deterministic(True)
    scratch = None
    if opt.synthetic > 0:
        scratch = tempfile.mkdtemp(prefix="centerpose_synth_")
        w, h = (int(v) for v in opt.synthetic_size.lower().split("x"))
        synth.write_dataset(scratch, opt.synthetic, opt.c, tracking=opt.tracking_task, size=(w, h), seed=opt.seed)
        opt.data_dir = scratch
    try:
        run(o, opt)
    finally:
        if scratch is not None:
            shutil.rmtree(scratch, ignore_errors=True)


def run(o, opt):
    opt = o.update_dataset_info_and_set_heads(opt, ObjectPoseDataset)
    print(opt)
    logger = Logger(opt)
    opt.device = torch.device("cuda" if opt.gpus[0] >= 0 else "cpu")

    print("Creating model...")
    model = create_model(opt.arch, opt.heads, opt.head_conv, opt=opt)
    optimizer = Adam(model.parameters(), opt.lr, max_grad_norm=100.)
    start_epoch = 0
    if opt.load_model != "":
        model, optimizer, start_epoch = load_model(model, opt.load_model, optimizer, opt.resume, opt.lr, opt.lr_step)
    detector = None
    if opt.track_detector:
        detector, _ = track_detector(opt, opt.track_detector)
    trainer = train_factory[opt.task](opt, model, optimizer, detector=detector)
    trainer.set_device(opt.gpus, opt.chunk_sizes, opt.device)
    if opt.backward_precision != "f32":
        net = trainer.model_with_loss.model
        for m in (conv, deconv, pose_heads, dcn_v2):
            m.set_backward_precision(net, opt.backward_precision)

    print("Setting up data...")
    val_dataset = ObjectPoseDataset(opt, "val")
    if opt.tracking_task:  # every fifteenth frame, as the reference validates the videos
        val_dataset = torch.utils.data.Subset(val_dataset, range(0, len(val_dataset), 15))
    val_loader = torch.utils.data.DataLoader(val_dataset, batch_size=1, shuffle=False, num_workers=0, pin_memory=True,
                                             collate_fn=collate_fn_filtered)
    train_loader = torch.utils.data.DataLoader(ObjectPoseDataset(opt, "train"), batch_size=opt.batch_size,
                                               shuffle=not opt.no_shuffle, num_workers=opt.num_workers, pin_memory=True,
                                               drop_last=True, collate_fn=collate_fn_filtered)
    if opt.test:
        trainer.val(0, val_loader)

    def path(mark):
        return os.path.join(opt.save_dir, "{}_{}.pth".format(opt.c, mark))

    print("Starting training...")
    best = 1e10
    for epoch in range(start_epoch + 1, opt.num_epochs + 1):
        log, _, _ = trainer.train(epoch, train_loader)
        logger.write("epoch: {} | ".format(epoch))
        for k, v in log.items():
            logger.scalar_summary("train_{}".format(k), v, epoch)
            logger.write("train_{} {:8f} | ".format(k, v))
        save_model(path("last"), epoch, model, optimizer)
        if opt.val_intervals > 0 and epoch % opt.val_intervals == 0 and len(val_dataset) > 0:
            if opt.save_all:
                save_model(path(epoch), epoch, model, optimizer)
            log_val, _, _ = trainer.val(epoch, val_loader)
            for k, v in log_val.items():
                logger.scalar_summary("val_{}".format(k), v, epoch)
                logger.write("val_{} {:8f} | ".format(k, v))
            if log_val[opt.metric] < best:
                best = log_val[opt.metric]
                save_model(path("best"), epoch, model)
        logger.write("\n\n")
        if epoch in opt.lr_step:
            save_model(path(epoch), epoch, model, optimizer)
            lr = opt.lr * (0.1 ** (opt.lr_step.index(epoch) + 1))
            print("Drop LR to", lr)
            for group in optimizer.param_groups:
                group["lr"] = lr
    logger.close()


if __name__ == "__main__":
    main()
