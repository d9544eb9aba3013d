"""Numpy restatement of the training input image (ObjectPoseDataset._get_input, datasets/dataset_combined.py:278-288, with
color_aug, utils/image.py:239-277), from a decoded frame and its cp_train_inputs record: oracle.cv_emul.warp_affine_u8
on the (flipped) frame, then / 255, colour, normalise.

mode 'f32'  mirrors numpy's own evaluation of the reference's statements: the same in-place operations on a float32
            image with Python-float alphas, so every rounding falls where the reference's falls (numpy >= 2 promotion:
            a Python float beside a float32 array or scalar is rounded to float32).
mode 'f64'  every step after the 8-bit warp in float64: the yardstick of the colour images' error bound.
"""
import numpy as np

from centerpose_amd import hip
from centerpose_amd.train_inputs import MEAN, STD
from oracle import cv_emul

I = hip.TI_IMG
OPS = {"b": "brightness", "c": "contrast", "s": "saturation"}


def grey(img):
    """cv2.cvtColor(img, COLOR_BGR2GRAY) of a float image, in the image's dtype."""
    t = img.dtype.type
    return (t(0.114) * img[..., 0] + t(0.587) * img[..., 1]) + t(0.299) * img[..., 2]


def warp_u8(frame, rec, side):
    """The 8-bit warped image [side, side, 3] of the record's transform; the reference warps the flipped view."""
    src = frame[:, ::-1, :] if rec[I["flipped"]] else frame
    return cv_emul.warp_affine_u8(np.ascontiguousarray(src), rec[I["trans"]:I["trans"] + 6].reshape(2, 3), (side, side))


def _blend(alpha, image1, image2):  # blend_ (utils/image.py:248-251), statement for statement
    image1 *= alpha
    image2 *= (1 - alpha)
    image1 += image2


def color(inp, rec, gs_mean=None):
    """color_aug on `inp` [H,W,3] (float32 or float64) in place with the record's draws; returns the gs_mean used.
    `gs_mean` overrides the image's own mean (the device reduces it in another order)."""
    order = hip.TI_ORDERS[int(rec[I["order"]])]
    gs = grey(inp)
    m = gs.mean() if gs_mean is None else inp.dtype.type(gs_mean)
    for i, op in enumerate(order):
        alpha = float(rec[I["alpha"] + i])
        if op == "b":
            inp *= alpha
        elif op == "c":
            _blend(alpha, inp, m)  # a scalar: `image2 *=` rebinds the local name only
        else:
            _blend(alpha, inp, gs[:, :, None])
    inp += rec[I["shift"]:I["shift"] + 3]  # lighting_: a float64 array into the image
    return m


def image(frame, rec, side, mode="f32", mean=MEAN, std=STD, gs_mean=None):
    """[3, side, side] of one frame and record: float32 in mode 'f32', float64 in mode 'f64'."""
    dt = np.float32 if mode == "f32" else np.float64
    inp = warp_u8(frame, rec, side).astype(dt) / 255.
    assert inp.dtype == dt
    if rec[I["color"]]:
        color(inp, rec, gs_mean)
    inp = (inp - np.asarray(mean, np.float32).astype(dt)) / np.asarray(std, np.float32).astype(dt)
    assert inp.dtype == dt
    return inp.transpose(2, 0, 1)


def batch(frames, recs, side, mode="f32", gs_means=None):
    return np.stack([image(f, r, side, mode, gs_mean=None if gs_means is None else gs_means[n])
                     for n, (f, r) in enumerate(zip(frames, recs))])
