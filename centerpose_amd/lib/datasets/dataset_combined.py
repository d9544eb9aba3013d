"""ObjectPoseDataset with the reference's constructor contract (datasets/dataset_combined.py:107-231) and a
``__getitem__`` that keeps what depends on the host and leaves the rest to the device.

The reference's ``__getitem__`` decodes the image, draws the augmentation, warps the image and draws every dense target
map in numpy.  Here the sample is the decoded frame plus a few small float64 records, and the training step expands them
on the device (lib.trains.base_trainer: TrainInputs, PoseTargets / TrackPoseTargets):

    frame        uint8 HWC BGR as decoded, NOT flipped (the record carries the flip)
    ti_image     pack_input(trans_input, height, width, flipped, colour draws)
    pt_image     pack_annotations(anns, trans_output_rot, width, height, flipped, rot, opt)
    pt_objects

and with opt.tracking_task

    frame_pre, ti_image_pre                         the previous frame and its own input record
    ptk_image, ptk_pre_objects, ptk_cur_objects     pack_track_annotations(...) with draw_track_noise's numbers
    ptk_gen, ptk_det_meta                           only with opt.data_generation_mode_ratio > 0 (generation=)

Every host-side random draw is made in the reference's order and from the reference's three generators (np.random,
random, self._data_rng): _get_aug_param (:240-265), the flip draw (:335), draw_color_aug where _get_input calls
color_aug (:285), and for the tracking task the previous-frame choice (:424), its own augmentation (:445) and colour
draws (:456), the generation mode (:465) and then the noise as one draw_track_noise block.  On 'val' the single-frame
task draws nothing (c_ori, s_ori, no colour).  The dataset never constructs a detector: the reference's in-dataset
detector (:141-172) is the trainer's TrackPoseTargets(opt, detector=...).
"""
import glob
import json
import os

import numpy as np
import torch.utils.data as data

from centerpose_amd.pose_targets import pack_annotations
from centerpose_amd.pose_targets_track import draw_generation_mode, draw_track_noise, pack_track_annotations
from centerpose_amd.train_inputs import draw_color_aug, pack_input

from ..utils.image import get_affine_transform

_IMAGE_EXTENSIONS = ("png", "jpg")


def read_image(path):
    """The decoded frame as uint8 HWC BGR, or None when it cannot be read (cv2.imread's answer).  cv2 when it can be
    imported, else PIL converted to BGR: the same bytes for PNG, which is lossless; a JPEG decoder of PIL's need not
    agree with cv2's to the bit."""
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        return cv2.imread(path)
    try:
        from PIL import Image

        with Image.open(path) as im:
            rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
    except Exception:
        return None
    return np.ascontiguousarray(rgb[:, :, ::-1])


def find_samples(root, extensions=_IMAGE_EXTENSIONS):
    """[(img_path, video_id, frame_id, json_path)] under ``root``, discovered as the reference does (:177-205): a
    depth-first walk in os.listdir order that descends while a directory has sub-directories and, in a leaf, globs
    ``*.<ext>`` per extension and keeps an image that has a .json beside it.  On one file tree the order is the
    reference's."""
    found = []

    def leaf(path):
        for ext in extensions:
            for img in glob.glob(path + "/*.{}".format(ext)):
                ann = img.replace(ext, "json")
                if os.path.exists(img) and os.path.exists(ann):
                    found.append((img, os.path.split(os.path.split(img)[0])[1], os.path.splitext(os.path.basename(img))[0], ann))

    def walk(path):
        if not os.path.isdir(path):
            return
        below = [os.path.join(path, o) for o in os.listdir(path) if os.path.isdir(os.path.join(path, o))]
        for sub in below:
            walk(sub)
        if not below:
            leaf(path)

    walk(root)
    return found


class ObjectPoseDataset(data.Dataset):
    num_classes = 1
    num_joints = 8
    default_resolution = [512, 512]
    mean = np.array([0.40789654, 0.44719302, 0.47026115], dtype=np.float32).reshape(1, 1, 3)
    std = np.array([0.28863828, 0.27408164, 0.27809835], dtype=np.float32).reshape(1, 1, 3)
    flip_idx = [[1, 5], [3, 7], [2, 6], [4, 8]]  # the keypoints a horizontal flip swaps

    def __init__(self, opt, split):
        super().__init__()
        if getattr(opt, "new_data_augmentation", False):
            raise NotImplementedError("ObjectPoseDataset: opt.new_data_augmentation (albumentations MotionBlur / Downscale / "
                                      "GaussNoise on the decoded frame) is not built")
        self.data_dir = os.path.join(opt.data_dir, "outf_all" if opt.tracking_task else "outf")
        self.img_dir = os.path.join(self.data_dir, "{}_{}".format(opt.c, split))
        if split == "val" and not os.path.isdir(self.img_dir):  # the test split stands in for validation
            self.img_dir = os.path.join(self.data_dir, "{}_test".format(opt.c))
        self.max_objs = 10
        self._data_rng = np.random.RandomState(123)
        self.split = split
        self.opt = opt
        print("==> initializing objectron {}_{} data.".format(opt.c, split))
        print(self.img_dir)
        self.images = find_samples(self.img_dir)
        self.num_samples = len(self.images)
        print("Loaded {} {} samples".format(split, self.num_samples))
        self.videos = {}  # video_id -> its samples, in discovery order
        for sample in self.images:
            self.videos.setdefault(sample[1], []).append(sample)

    def __len__(self):
        return self.num_samples

    @staticmethod
    def _get_border(border, size):
        i = 1
        while size - border // i <= border // i:
            i *= 2
        return border // i

    def _get_aug_param(self, c_ori, s, width, height, disturb=False):
        """(c, aug_s, rot) with the draws of :240-265 in their order: the crop's scale choice and two randint centres, or
        (not_rand_crop, or the previous frame's disturbance) three randn; then the rotation's uniform, and a second one
        when it falls below opt.aug_rot."""
        opt = self.opt
        c = c_ori.copy()
        if (not opt.not_rand_crop) and not disturb:
            aug_s = np.random.choice(np.arange(0.6, 1.4, 0.1))
            w_border, h_border = self._get_border(128, width), self._get_border(128, height)
            c[0] = np.random.randint(low=w_border, high=width - w_border)
            c[1] = np.random.randint(low=h_border, high=height - h_border)
        else:
            sf, cf = opt.scale, opt.shift
            c[0] += s * np.clip(np.random.randn() * cf, -2 * cf, 2 * cf)
            c[1] += s * np.clip(np.random.randn() * cf, -2 * cf, 2 * cf)
            aug_s = np.clip(np.random.randn() * sf + 1, 1 - sf, 1 + sf)
        rot = 2 * (np.random.rand() - 0.5) * opt.rotate if np.random.random() < opt.aug_rot else 0
        return c, aug_s, rot

    def _color(self):
        """The colour draws at the place _get_input makes them (:284-285), or None."""
        if self.split == "train" and not self.opt.no_color_aug:
            return draw_color_aug(self._data_rng)
        return None

    def __getitem__(self, index):
        opt = self.opt
        path_img, video_id, frame_id, path_json = self.images[index]
        with open(path_json) as f:
            anns = json.load(f)
        frame = read_image(path_img)
        if frame is None or frame.ndim != 3:
            return None
        height, width = frame.shape[0], frame.shape[1]
        c_ori = np.array([width / 2., height / 2.], dtype=np.float32)
        s_ori = max(height, width) * 1.0
        rot, aug_s, flipped = 0, 1.0, False
        if self.split == "train":
            c, aug_s, rot = self._get_aug_param(c_ori, s_ori, width, height, disturb=False)
            s = s_ori * aug_s
            if np.random.random() < opt.flip:
                flipped = True
                c[0] = width - c[0] - 1
        else:
            c, s = c_ori, s_ori
        trans_input = get_affine_transform(c, s, rot, [opt.input_res, opt.input_res])
        color = self._color()
        trans_output_rot = get_affine_transform(c, s, rot, [opt.output_res, opt.output_res])
        ret = {"frame": np.ascontiguousarray(frame)}
        ret.update(pack_input(trans_input, height, width, flipped, color))
        if not opt.tracking_task:
            ret.update(pack_annotations(anns, trans_output_rot, width, height, flipped, rot, opt, self.max_objs))
            return ret

        # the previous frame (:410-456): a nearby frame of the video in training, the exact predecessor (or the frame
        # itself) otherwise
        group = self.videos[video_id]
        if "train" in self.split:
            near = [g for g in group if abs(int(g[2]) - int(frame_id)) < opt.max_frame_dist]
        else:
            near = [g for g in group if int(g[2]) - int(frame_id) == -1] or [g for g in group if int(g[2]) == int(frame_id)]
        path_img_pre, _, frame_id_pre, path_json_pre = near[np.random.choice(len(near))]
        frame_dist = abs(int(frame_id) - int(frame_id_pre))
        frame_pre = read_image(path_img_pre)
        with open(path_json_pre) as f:
            anns_pre = json.load(f)
        same = bool(opt.same_aug_pre and frame_dist != 0)
        if same:
            trans_input_pre, c_pre, s_pre, aug_s_pre = trans_input, c, s, aug_s
        else:  # its own disturbance, the current frame's rotation
            c_pre, aug_s_pre, _ = self._get_aug_param(c_ori, s_ori, width, height, disturb=True)
            s_pre = s_ori * aug_s_pre
            trans_input_pre = get_affine_transform(c_pre, s_pre, rot, [opt.input_w, opt.input_h])
        if frame_pre is None or frame_pre.ndim != 3:
            return None
        color_pre = self._color()
        mode = draw_generation_mode(None, opt.data_generation_mode_ratio)
        draws = draw_track_noise(None, len(anns_pre["objects"]))
        generation = None
        if opt.data_generation_mode_ratio > 0:
            generation = dict(mode=mode, c=c_pre, s=s_pre, aug_s=aug_s_pre,
                              intrinsics=anns_pre["camera_data"]["intrinsics"])
        ret["frame_pre"] = np.ascontiguousarray(frame_pre)
        ret["ti_image_pre"] = pack_input(trans_input_pre, frame_pre.shape[0], frame_pre.shape[1], flipped, color_pre)["ti_image"]
        ret.update(pack_track_annotations(anns, anns_pre, trans_output_rot, trans_input_pre, width, height, flipped, rot, opt,
                                          draws, self.max_objs, generation=generation))
        return ret
