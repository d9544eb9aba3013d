"""Training input images on the device: ``batch['input']`` (and ``batch['pre_img']`` of the tracking task) as
ObjectPoseDataset._get_input builds them (datasets/dataset_combined.py:278-288, called at :348 and :456), for a whole
batch, computed by cp_train_inputs from the decoded 8-bit frames.

The host keeps image decoding and every random draw.  A dataset returns, per image, the decoded frame and the small
fixed-size record of ``pack_input`` (the default collate stacks it); the training step warps, flips, jitters and
normalises on the device:

    color = None if opt.no_color_aug else draw_color_aug(self._data_rng)          # per image, in the dataset
    ret['frame'] = frame_as_decoded                                               # uint8 HWC BGR, not flipped
    ret.update(pack_input(trans_input, height, width, flipped, color))
    batch['input'] = TrainInputs(opt)(batch['frame'], batch['ti_image'])          # per batch, on the device

``draw_color_aug`` consumes ``random`` and ``data_rng`` exactly as ``color_aug`` (utils/image.py:269-277) does, so a
dataset that swaps one call for the other keeps its random stream.
"""
import random

import numpy as np
import torch

from . import hip

# ObjectPoseDataset's tables (dataset_combined.py:60-63, :130-137), float32 as there
MEAN = np.array([0.40789654, 0.44719302, 0.47026115], dtype=np.float32)
STD = np.array([0.28863828, 0.27408164, 0.27809835], dtype=np.float32)
EIG_VAL = np.array([0.2141788, 0.01817699, 0.00341571], dtype=np.float32)
EIG_VEC = np.array([[-0.58752847, -0.69563484, 0.41340352],
                    [-0.5832747, 0.00994535, -0.81221408],
                    [-0.56089297, 0.71832671, 0.41158938]], dtype=np.float32)
FRAME_ALIGN = 256  # bytes between the starts of packed frames are a multiple of this


def draw_color_aug(data_rng, py_random=random):
    """The draws of one ``color_aug`` call, in its order: ``random.shuffle`` of the three functions (:270-271), one
    ``data_rng.uniform(-0.4, 0.4)`` per function in the shuffled order (:255, :260, :265), then
    ``data_rng.normal(scale=0.1, size=(3,))`` (:244).  Returns {'order': code 0..5 (hip.TI_ORDERS), 'alphas': the three
    ``1 + uniform`` values as run, 'light': the three normal draws}."""
    ops = ["b", "c", "s"]  # brightness_, contrast_, saturation_
    py_random.shuffle(ops)
    alphas = [1. + data_rng.uniform(low=-0.4, high=0.4) for _ in ops]
    light = data_rng.normal(scale=0.1, size=(3,))
    return {"order": hip.TI_ORDERS.index("".join(ops)), "alphas": alphas, "light": light}


def pack_input(trans_input, height, width, flipped, color=None, eig_val=EIG_VAL, eig_vec=EIG_VEC):
    """The per-image record of cp_train_inputs (layout in include/centerpose_hip.h), on the host in numpy:
    {'ti_image': float64 [hip.TI_STRIDE]}.  ``trans_input`` is the forward 2x3 input affine (c[0] already mirrored when
    flipped, :339), ``height`` / ``width`` the decoded frame's size, ``color`` the dict of ``draw_color_aug`` or None
    (opt.no_color_aug, or a split other than train).  The frame's byte offset is filled in by ``TrainInputs``."""
    I = hip.TI_IMG
    rec = np.zeros(hip.TI_STRIDE, np.float64)
    rec[I["height"]], rec[I["width"]] = height, width
    rec[I["trans"]:I["trans"] + 6] = np.asarray(trans_input, np.float64).reshape(6)
    rec[I["flipped"]] = float(bool(flipped))
    if color is not None:
        rec[I["color"]], rec[I["order"]] = 1.0, int(color["order"])
        rec[I["alpha"]:I["alpha"] + 3] = np.asarray(color["alphas"], np.float64)
        # lighting_ (:243-245): a float32 table times float64 draws, float64
        rec[I["shift"]:I["shift"] + 3] = np.dot(eig_vec, eig_val * np.asarray(color["light"], np.float64))
    return {"ti_image": rec}


def pack_frames(frames, records, pin=False):
    """Packs a list of uint8 HWC frames (arrays or host tensors) of differing sizes into one host uint8 buffer (pinned
    with ``pin``), each frame starting at a multiple of FRAME_ALIGN, and returns (buffer, records with the offsets
    written).  The records' height / width must be the frames'."""
    I = hip.TI_IMG
    records = np.array(records, dtype=np.float64, order="C", copy=True)
    if records.ndim != 2 or records.shape[1] != hip.TI_STRIDE or records.shape[0] != len(frames):
        raise ValueError("TrainInputs: records must be [%d, %d], one per frame" % (len(frames), hip.TI_STRIDE))
    views, off = [], 0
    for n, f in enumerate(frames):
        t = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("TrainInputs: frame %d must be uint8 [H, W, 3]" % n)
        if (records[n, I["height"]], records[n, I["width"]]) != (t.shape[0], t.shape[1]):
            raise ValueError("TrainInputs: frame %d is %dx%d, its record says %gx%g"
                             % (n, t.shape[0], t.shape[1], records[n, I["height"]], records[n, I["width"]]))
        records[n, I["offset"]] = off
        views.append((off, t))
        off += (t.numel() + FRAME_ALIGN - 1) // FRAME_ALIGN * FRAME_ALIGN
    buf = torch.empty(off, dtype=torch.uint8, pin_memory=pin)
    for o, t in views:
        buf[o:o + t.numel()].copy_(t.reshape(-1))
    return buf, records


def split_tracking(out):
    """The two halves of a 2B-frame call (current frames first, previous frames second) as the tracking task's
    {'input', 'pre_img'} (:348, :456)."""
    B = out.shape[0] // 2
    return {"input": out[:B], "pre_img": out[B:]}


class TrainInputs:
    """Builds the batch's network inputs on the device from decoded frames and collated ``pack_input`` records.  Refuses
    opt.new_data_augmentation at construction: its albumentations blur / down-scale / noise draws (:307-319) are not
    built."""

    def __init__(self, opt, split="train"):
        if getattr(opt, "new_data_augmentation", False):
            raise NotImplementedError("TrainInputs on the device: opt.new_data_augmentation (albumentations MotionBlur / "
                                      "Downscale / GaussNoise on the decoded frame) is not built")
        self.opt, self.split = opt, split
        self.res = int(opt.input_res)
        self.mean = np.asarray(getattr(opt, "mean", MEAN), np.float32).reshape(3)
        self.std = np.asarray(getattr(opt, "std", STD), np.float32).reshape(3)

    def __call__(self, frames, records, device=None, out=None, return_means=False):
        """``frames``: one uint8 [N, H, W, 3] tensor (host or device), or a list of N uint8 HWC arrays / tensors of
        differing sizes, which are packed into one pinned staging buffer and copied once.  ``records``: [N,
        hip.TI_STRIDE] (tensor or array on the host).  Returns float32 [N, 3, input_res, input_res] on ``device``
        (default: the frames' device, else the current HIP device), written on the current stream."""
        I = hip.TI_IMG
        rec = records.cpu().numpy() if torch.is_tensor(records) else np.asarray(records)
        if torch.is_tensor(frames):
            if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError("TrainInputs: frames must be uint8 [N, H, W, 3]")
            rec = np.array(rec, dtype=np.float64, order="C", copy=True)
            N, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
            if rec.shape != (N, hip.TI_STRIDE) or (rec[:, I["height"]] != H).any() or (rec[:, I["width"]] != W).any():
                raise ValueError("TrainInputs: records must be [%d, %d] with height %d and width %d"
                                 % (N, hip.TI_STRIDE, H, W))
            rec[:, I["offset"]] = np.arange(N, dtype=np.float64) * (3 * H * W)
            if device is None and frames.is_cuda:
                device = frames.device
            host = frames.contiguous()
        else:
            host, rec = pack_frames(frames, rec, pin=True)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        buf = host.to(dev, non_blocking=True)
        if out is None:
            out = torch.empty(rec.shape[0], 3, self.res, self.res, dtype=torch.float32, device=dev)
        return hip.train_inputs(buf, rec, self.mean, self.std, out, return_means=return_means)
