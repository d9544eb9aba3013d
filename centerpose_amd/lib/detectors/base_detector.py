"""``BaseDetector`` with the reference's public surface (detectors/base_detector.py:31-776):
``run(image_or_path_or_tensor, filename=None, meta_inp={}, preprocessed_flag=False)`` returns the same
dict ({'results','boxes','output','tot','load','pre','net','dec','post','merge','pnp','track'}), with the
network, decode and PnP stages executed by libcenterpose_hip.so.  ``run_batch`` is the added batched
entry point (the reference processes one image per call, base_detector.py:134,431).

CenterPoseTrack (``opt.tracking_task``) and the Kalman baseline (``opt.refined_Kalman``) run the reference's
per-frame loop (:445-464 previous-frame inputs rendered from the tracks, :501-544 Gaussian fusion of the two keypoint
estimates, :660-665 ``tracker.step``); the previous-frame heat-maps are drawn on the device (cp_render_gaussians).

With ``opt.debug`` >= 1 ``run`` builds a ``Debugger`` (utils/debugger.py) as the reference does (:393) and hands it to
``show_results`` / ``save_results``: ``--debug 4`` writes ``<demo_save>/<name>/<file>_out_img_pred.png`` beside the JSON,
drawn by the library's own rasteriser (cp_draw_primitives).  ``run_batch(..., draw=frames)`` draws a batch's detections into
device frames without a read-back (cp_draw_detections).

Not mirrored: the heat-map views of ``debug()`` (debug 2 / 3: gen_colormap, add_blend_img, add_arrow),
cv2's anti-aliasing and font, and the GMM sampling of rep_mode 2.
"""
import copy
import json
import math
import os
import time

import numpy as np
import torch

from ..models.model import create_model, load_model
from ..utils.image import (get_affine_transform, affine_transform, warp_affine_bilinear, gaussian_radius,
                           draw_gaussian_records)
from ..utils.tracker import Tracker, Tracker_baseline
from ..utils.pnp.cuboid_pnp_shell import pnp_shell, finish_detection
from ..utils.pnp.cuboid_pnp_solver import solve_pnp_batch


def _imread_bgr(path):
    """cv2.imread stand-in: HxWx3 uint8 in BGR order (the reference's mean/std are BGR-ordered, opts.py:436-437)."""
    try:
        import cv2  # noqa: F401

        return cv2.imread(path)
    except ImportError:
        from PIL import Image

        return np.asarray(Image.open(path).convert('RGB'))[:, :, ::-1].copy()


def _resize(image, new_w, new_h):
    if image.shape[1] == new_w and image.shape[0] == new_h:
        return image
    try:
        import cv2

        return cv2.resize(image, (new_w, new_h))
    except ImportError:
        from PIL import Image

        return np.asarray(Image.fromarray(image).resize((new_w, new_h), Image.BILINEAR))


def _build_tracker(opt):
    """Which track keeper the flags select (base_detector.py:53-57: ``refined_Kalman`` wins when both are set)."""
    if opt.refined_Kalman:
        return Tracker_baseline(opt)
    if opt.tracking_task:
        return Tracker(opt)
    return None


class BaseDetector(object):
    """Public attributes as the reference constructor leaves them (base_detector.py:31-57): ``model`` (built, loaded,
    moved, eval), ``mean`` / ``std`` ([1,1,3] float32), ``max_per_image``, ``num_classes``, ``scales``, ``opt`` (with
    ``opt.device`` filled in), ``pause``, ``pre_images`` and -- for the tracking configurations -- ``tracker``."""

    def __init__(self, opt):
        opt.device = torch.device('cuda' if opt.gpus[0] >= 0 else 'cpu')
        self.opt = opt
        print('Creating model...')
        net = load_model(create_model(opt.arch, opt.heads, opt.head_conv, opt), opt.load_model)
        self.model = net.to(opt.device)
        self.model.eval()
        self.mean, self.std = (np.array(v, dtype=np.float32).reshape(1, 1, 3) for v in (opt.mean, opt.std))
        self.num_classes, self.scales = opt.num_classes, opt.test_scales
        self.max_per_image, self.pause, self.pre_images = 100, True, None
        tracker = _build_tracker(opt)
        if tracker is not None:
            self.tracker = tracker

    def process(self, images, pre_images=None, pre_hms=None, pre_inds=None, return_time=False):
        raise NotImplementedError

    def post_process(self, dets, meta, scale=1):
        raise NotImplementedError

    def merge_outputs(self, detections):
        raise NotImplementedError

    def show_results(self, debugger, image, results):
        raise NotImplementedError

    def _trans_bbox(self, bbox, trans, width, height):
        bbox = np.array(copy.deepcopy(bbox), dtype=np.float32)
        bbox[:2] = affine_transform(bbox[:2], trans)
        bbox[2:] = affine_transform(bbox[2:], trans)
        bbox[[0, 2]] = np.clip(bbox[[0, 2]], 0, width - 1)
        bbox[[1, 3]] = np.clip(bbox[[1, 3]], 0, height - 1)
        return bbox

    def _input_geometry(self, height, width, scale):
        """Network input size and the crop (centre c, extent s) of the three test modes (base_detector.py:103-120):
        ``fix_short`` (short side fixed, long side rounded up to 64), ``fix_res`` (the demo's mode: input_h x input_w,
        crop = the scaled frame's centre with the longer ORIGINAL side as extent), else keep the resolution and pad to
        ``opt.pad + 1``.  Returns (inp_h, inp_w, c, s, scaled_h, scaled_w)."""
        o = self.opt
        sh, sw = int(height * scale), int(width * scale)
        f32 = np.float32
        if o.fix_short > 0:
            long_side = lambda a, b: (int(a / b * o.fix_short) + 63) // 64 * 64
            inp_h, inp_w = (o.fix_short, long_side(width, height)) if height < width else (long_side(height, width), o.fix_short)
            return inp_h, inp_w, np.array([width / 2, height / 2], dtype=f32), np.array([width, height], dtype=f32), sh, sw
        if o.fix_res:
            return o.input_h, o.input_w, np.array([sw / 2., sh / 2.], dtype=f32), max(height, width) * 1.0, sh, sw
        inp_h, inp_w = (sh | o.pad) + 1, (sw | o.pad) + 1
        return inp_h, inp_w, np.array([sw // 2, sh // 2], dtype=f32), np.array([inp_w, inp_h], dtype=f32), sh, sw

    def pre_process(self, image, scale, input_meta={}):
        """base_detector.py:91-148: resize by ``scale``, warp the crop into the network input, normalise, CHW; the meta
        dict carries the crop and both affine maps for post-processing."""
        height, width = image.shape[0:2]
        inp_height, inp_width, c, s, new_height, new_width = self._input_geometry(height, width, scale)
        out_height, out_width = inp_height // self.opt.down_ratio, inp_width // self.opt.down_ratio
        trans_input = get_affine_transform(c, s, 0, [inp_width, inp_height])
        trans_output = get_affine_transform(c, s, 0, [out_width, out_height])
        if self.opt.device.type == 'cuda' and image.dtype == np.uint8 and image.ndim == 3:
            # resize (scale != 1) + warp + normalise on the device, in OpenCV's fixed-point arithmetic (cp_resize_u8,
            # cp_preprocess); the 8-bit frame is the only host->device copy
            from centerpose_amd import hip as _hip
            frame = torch.from_numpy(np.ascontiguousarray(image)).to(self.opt.device)
            if (new_width, new_height) != (width, height):
                frame = _hip.resize_u8(frame, new_height, new_width)
            images = _hip.preprocess(frame, trans_input, self.mean, self.std, inp_height, inp_width)
        else:
            resized_image = _resize(image, new_width, new_height)
            inp_image = warp_affine_bilinear(resized_image, trans_input, inp_width, inp_height)
            inp_image = ((inp_image / 255. - self.mean) / self.std).astype(np.float32)
            images = torch.from_numpy(inp_image.transpose(2, 0, 1).reshape(1, 3, inp_height, inp_width))
        meta = {'c': c, 's': s, 'height': height, 'width': width, 'out_height': out_height, 'out_width': out_width,
                'inp_height': inp_height, 'inp_width': inp_width, 'trans_input': trans_input,
                'trans_output': trans_output}
        for k in ('pre_dets', 'camera_matrix', 'id'):
            if k in input_meta:
                meta[k] = input_meta[k]
        return images, meta

    # ------------------------------------------------------------------ CenterPoseTrack: previous-frame inputs
    def _hp_confidence(self, det):
        """Peak value of each vertex Gaussian (base_detector.py:277-305): from the Kalman covariance, from the fused
        std, or the measured heat-map height."""
        lo, hi = self.opt.conf_border[self.opt.c][0], self.opt.conf_border[self.opt.c][1]
        decay = np.exp(np.log(0.15) / (lo - hi))
        if self.opt.kalman == True and 'kf' in det:  # noqa: E712
            P = det['kf'].P
            comb = [np.sqrt(P[4 * i, 4 * i] + P[4 * i + 1, 4 * i + 1]) for i in range(8)]
        elif self.opt.hps_uncertainty:
            f = det['kps_fusion_std']
            comb = [np.sqrt(f[2 * i] + f[2 * i + 1]) for i in range(8)]
        else:
            return np.array(det['kps_heatmap_height'])
        return [np.maximum(1 - decay ** (c - hi), 0) for c in comb]

    def _hp_source(self, det, mode):
        """Which vertex estimate is re-drawn (normalised image coordinates, centre first; :253-268)."""
        o = self.opt
        if mode == 'gt':
            return np.array(det['kps_gt'][1:])
        if o.render_hmhp_mode in (0, 1):
            return np.array(det['kps_ori'][1:])
        if o.kalman == True or o.scale_pool == True:  # noqa: E712
            return np.array(det['kps_pnp_kf'][1:]) if 'kps_pnp_kf' in det else np.array(det['kps_mean_kf'][1:])
        return np.array(det['kps_pnp'][1:]) if 'kps_pnp' in det else np.zeros((8, 2))  # PnP failed: nothing to draw

    def _track_records(self, dets, meta, with_hm, with_hm_hp):
        """The Gaussians ``_get_additional_inputs`` draws (base_detector.py:150-388), as (channel, x, y, radius, k)
        records for pre_hm and pre_hm_hp, plus the output-grid centre indices."""
        o = self.opt
        t_in, t_out = meta['trans_input'], meta['trans_output']
        iw, ih, ow, oh = meta['inp_width'], meta['inp_height'], meta['out_width'], meta['out_height']
        W0, H0 = meta['width'], meta['height']
        hm, hp, inds = [], [], []
        if o.empty_pre_hm:
            return hm, hp, inds
        if o.gt_pre_hm_hmhp == True or (o.gt_pre_hm_hmhp_first == True and meta['id'] == 0):  # noqa: E712
            mode = 'gt'
        else:
            mode = 'pnp' if o.use_pnp else 'kps'
        for det in dets:
            if mode != 'gt' and not det['score'] >= o.pre_thresh:  # (written so that a NaN score draws nothing)
                continue
            box = self._trans_bbox(det['bbox'], t_in, iw, ih)
            box_out = self._trans_bbox(det['bbox'], t_out, ow, oh)
            h, w = box[3] - box[1], box[2] - box[0]
            if not (h > 0 and w > 0):
                continue
            radius = max(0, int(gaussian_radius((math.ceil(h), math.ceil(w)))))
            ct = np.array([(box[0] + box[2]) / 2, (box[1] + box[3]) / 2], dtype=np.float32).astype(np.int32)
            if with_hm:
                k = det['score'] if (mode != 'gt' and o.render_hm_mode == 1) else 1
                if mode == 'gt' or o.render_hm_mode in (0, 1):
                    hm.append((0, int(ct[0]), int(ct[1]), radius, k))
            ct_out = np.array([(box_out[0] + box_out[2]) / 2, (box_out[1] + box_out[3]) / 2], dtype=np.int32)
            inds.append(ct_out[1] * ow + ct_out[0])
            if not with_hm_hp:
                continue
            if mode == 'kps':
                src = np.array(det['kps']).reshape((-1, 2))
            else:
                src = self._hp_source(det, mode)
                src[:, 0] = src[:, 0] * W0
                src[:, 1] = src[:, 1] * H0
            if mode == 'pnp':
                spread = np.array(det['kps_fusion_std'] if o.hps_uncertainty == True  # noqa: E712
                                  else det['kps_heatmap_std']).reshape(-1, 2).astype(np.int32)
                conf = self._hp_confidence(det)
            # COCO-style visibility in an integer table, exactly as the reference builds it (floats truncate)
            pts = np.zeros((8, 3), dtype='int64')
            for idx, q in enumerate(src):
                outside = q[0] >= W0 or q[0] < 0 or q[1] < 0 or q[1] >= H0
                pts[idx] = [q[0], q[1], 1 if outside else 2]
            for j in range(8):
                pts[j, :2] = affine_transform(pts[j, :2], t_in)
                if mode != 'gt':
                    if not (pts[j, 2] > 1 and 0 <= pts[j, 0] < iw and 0 <= pts[j, 1] < ih):
                        continue
                x, y = pts[j, :2].astype(np.int32)
                if mode == 'pnp' and o.render_hmhp_mode in (0, 2):
                    if spread[j, 0] > 0:  # the heat-map estimate is sometimes missing
                        hp.append((j, int(x), int(y), radius, conf[j]))
                elif mode != 'pnp' or o.render_hmhp_mode in (1, 3):
                    hp.append((j, int(x), int(y), radius, 1))
        return hm, hp, inds

    def _get_additional_inputs(self, dets, meta, with_hm=True, with_hm_hp=True):
        """Render the previous frame's tracks as network inputs: pre_hm [1,1,H,W], pre_hm_hp [1,8,H,W], pre_inds."""
        hm, hp, inds = self._track_records(dets, meta, with_hm, with_hm_hp)
        ih, iw = meta['inp_height'], meta['inp_width']
        dev = self.opt.device

        def render(recs, C):
            if dev.type == 'cuda':
                from centerpose_amd import hip as _hip
                return _hip.render_gaussians(np.array(recs, np.float64).reshape(-1, 5), C, ih, iw, dev)[None]
            return torch.from_numpy(draw_gaussian_records(recs, C, ih, iw)[None]).to(dev)

        input_hm = render(hm, 1) if with_hm else None
        input_hm_hp = render(hp, 8) if with_hm_hp else None
        output_inds = torch.from_numpy(np.array(inds, np.int64).reshape(1, -1)).to(dev)
        return input_hm, input_hm_hp, output_inds

    def _fuse_keypoints(self, det):
        """Product of the displacement and heat-map Gaussians per coordinate (base_detector.py:503-536)."""
        mean, std = [], []
        dm, ds = det['kps_displacement_mean'], det['kps_displacement_std']
        hmn, hs = det['kps_heatmap_mean'], det['kps_heatmap_std']
        for i in range(16):
            missing = hmn[i] < 0 or hs[i] < 0
            if self.opt.hps_uncertainty == True:  # noqa: E712
                if missing:
                    s_, m_ = ds[i], dm[i]
                else:
                    s_ = (ds[i] ** -2 + hs[i] ** -2) ** -0.5
                    m_ = s_ ** 2 * (ds[i] ** -2 * dm[i] + hs[i] ** -2 * hmn[i])
            elif missing:
                s_, m_ = 20, dm[i]
            else:
                s_ = hs[i] / np.sqrt(2)
                m_ = s_ ** 2 * (hs[i] ** -2 * dm[i] + hs[i] ** -2 * hmn[i])
            mean.append(m_)
            std.append(s_)
        return mean, std

    # ------------------------------------------------------------------ PnP input assembly
    def _pnp_points(self, det):
        """base_detector.py:549-566"""
        if self.opt.rep_mode in (0, 3, 4):
            return np.array(det['kps']).reshape(-1, 2)
        if self.opt.rep_mode == 1:
            p1 = np.array(det['kps_displacement_mean']).reshape(-1, 2)
            p2 = np.array(det['kps_heatmap_mean']).reshape(-1, 2)
            return np.hstack((p1, p2)).reshape(-1, 2)
        raise NotImplementedError("rep_mode 2 (GMM sampling with np.random, base_detector.py:568-650) is out of scope")

    def _pnp_all(self, results, meta):
        """One batched device solve for every surviving detection, then the reference's per-detection
        packaging / visibility filters (cuboid_pnp_shell.py:26-91)."""
        boxes = []
        if not len(results):
            return boxes
        pts = [self._pnp_points(d) for d in results]
        scales = [np.asarray(d['obj_scale'], np.float64) / d['obj_scale'][1] for d in results]
        raw = solve_pnp_batch(pts, scales, meta['camera_matrix'], device=self.opt.device)
        for det, r in zip(results, raw):
            if int(r[0]) != 1:  # no pose (too few points, behind the camera, degenerate): dropped (cuboid_pnp_shell.py:24)
                continue
            proj = r[8:24].reshape(8, 2).copy()
            if self.opt.show_axes:  # OPENCV_RETURN (base_detector.py:652)
                loc, quat = list(r[4:7]), r[24:28].copy()
            else:
                loc, quat = list(r[28:31]), r[31:35].copy()
            ret = finish_detection(self.opt, meta, det, det['obj_scale'], loc, quat, proj)
            if ret is not None:
                boxes.append(ret)
        return boxes

    def _dict_out(self, meta, boxes):
        """base_detector.py:672-754 (non-tracking branch)"""
        dict_out = {"camera_data": [], "objects": []}
        if 'camera_matrix' in meta:
            dict_out['camera_data'] = np.asarray(meta['camera_matrix']).tolist()
        o = self.opt
        if o.tracking_task or o.refined_Kalman:  # one object per live track (:681-731)
            for t in self.tracker.tracks:
                obj = {'class': o.c, 'ct': t['ct'], 'bbox': np.array(t['bbox']).tolist(), 'confidence': t['score'],
                       'kps_displacement_mean': t['kps_displacement_mean'].tolist(),
                       'kps_heatmap_mean': t['kps_heatmap_mean'].tolist(), 'kps_heatmap_std': t['kps_heatmap_std'].tolist(),
                       'kps_heatmap_height': t['kps_heatmap_height'].tolist(),
                       'obj_scale': (t['obj_scale'] / t['obj_scale'][1]).tolist(), 'tracking_id': t['tracking_id']}
                if o.use_pnp:
                    if 'location' in t:
                        obj['location'] = t['location']
                        obj['quaternion_xyzw'] = t['quaternion_xyzw'].tolist()
                    if 'kps_pnp' in t:
                        obj['kps_pnp'] = t['kps_pnp'].tolist()
                        obj['kps_3d_cam'] = t['kps_3d_cam'].tolist()
                if o.obj_scale_uncertainty:
                    obj['obj_scale_uncertainty'] = t['obj_scale_uncertainty'].tolist()
                if o.kalman:
                    obj['kps_mean_kf'] = t['kps_mean_kf'].tolist()
                    obj['kps_std_kf'] = t['kps_std_kf']
                    if o.use_pnp and 'kps_pnp_kf' in t:
                        obj['kps_pnp_kf'] = t['kps_pnp_kf'].tolist()
                        obj['kps_3d_cam_kf'] = t['kps_3d_cam_kf'].tolist()
                if o.scale_pool == True:  # noqa: E712
                    obj['obj_scale_kf'] = (t['obj_scale_kf'] / t['obj_scale_kf'][1]).tolist()
                    obj['obj_scale_uncertainty_kf'] = t['obj_scale_uncertainty_kf'].tolist()
                if o.hps_uncertainty:
                    obj['kps_displacement_std'] = t['kps_displacement_std'].tolist()
                    obj['kps_fusion_mean'] = t['kps_fusion_mean'].tolist()
                    obj['kps_fusion_std'] = t['kps_fusion_std'].tolist()
                if o.tracking:
                    obj['tracking'] = t['tracking'].tolist()
                if o.tracking_hp:
                    obj['tracking_hp'] = t['tracking_hp'].tolist()
                dict_out['objects'].append(obj)
            return dict_out
        for box in boxes:
            b = box[4]
            obj = {'class': self.opt.c, 'ct': b['ct'], 'bbox': np.array(b['bbox']).tolist(), 'confidence': b['score'],
                   'kps_displacement_mean': b['kps_displacement_mean'].tolist(),
                   'kps_heatmap_mean': b['kps_heatmap_mean'].tolist(), 'kps_heatmap_std': b['kps_heatmap_std'].tolist(),
                   'kps_heatmap_height': b['kps_heatmap_height'].tolist(), 'obj_scale': b['obj_scale'].tolist()}
            if self.opt.use_pnp:
                if 'location' in b:
                    obj['location'] = [float(v) for v in b['location']]
                    obj['quaternion_xyzw'] = np.asarray(b['quaternion_xyzw']).tolist()
                if 'kps_pnp' in b:
                    obj['kps_pnp'] = b['kps_pnp'].tolist()
                    obj['kps_3d_cam'] = b['kps_3d_cam'].tolist()
            dict_out['objects'].append(obj)
        return dict_out

    def _sync(self):
        if self.opt.device.type == 'cuda':
            torch.cuda.synchronize()

    def run(self, image_or_path_or_tensor, filename=None, meta_inp={}, preprocessed_flag=False):
        load_time, pre_time, net_time, dec_time, post_time = 0, 0, 0, 0, 0
        merge_time, track_time, pnp_time, tot_time = 0, 0, 0, 0
        start_time = time.time()
        pre_processed = preprocessed_flag
        if isinstance(image_or_path_or_tensor, np.ndarray):
            image = image_or_path_or_tensor
            if filename is not None:
                image_or_path_or_tensor = filename
        elif type(image_or_path_or_tensor) == type(''):
            image = _imread_bgr(image_or_path_or_tensor)
        else:
            image = image_or_path_or_tensor['image'][0].numpy()
            pre_processed = True
        loaded_time = time.time()
        load_time += (loaded_time - start_time)

        detections = []
        for scale in self.scales:
            scale_start_time = time.time()
            if not pre_processed:
                images, meta = self.pre_process(image, scale, meta_inp)
            else:
                images = torch.from_numpy(np.expand_dims(image, axis=0))
                meta = meta_inp
            images = images.to(self.opt.device)
            pre_hms, pre_hm_hp, pre_inds = None, None, None
            if self.opt.refined_Kalman:
                self.tracker.init_track(meta)
            if self.opt.tracking_task:
                if self.pre_images is None:  # first frame of a video: the frame is its own predecessor
                    print('Initialize tracking!')
                    self.pre_images = images
                    self.tracker.init_track(meta)
                elif self.opt.gt_pre_hm_hmhp or (self.opt.gt_pre_hm_hmhp_first and meta['id'] == 0):
                    self.tracker.init_track(meta)
                if self.opt.pre_hm or self.opt.pre_hm_hp:
                    pre_hms, pre_hm_hp, pre_inds = self._get_additional_inputs(
                        self.tracker.tracks, meta, with_hm=self.opt.pre_hm, with_hm_hp=self.opt.pre_hm_hp)
            self._sync()
            pre_process_time = time.time()
            pre_time += pre_process_time - scale_start_time
            output, dets, forward_time = self.process(images, self.pre_images, pre_hms, pre_hm_hp, pre_inds,
                                                      return_time=True)
            self._sync()
            net_time += forward_time - pre_process_time
            decode_time = time.time()
            dec_time += decode_time - forward_time
            dets = self.post_process(dets, meta, scale)
            post_process_time = time.time()
            post_time += post_process_time - decode_time
            detections.append(dets)

        results = self.merge_outputs(detections)
        merge_outputs_time = time.time()
        merge_time += merge_outputs_time - post_process_time

        if self.opt.tracking_task or self.opt.refined_Kalman:
            for det in results:
                m_, s_ = self._fuse_keypoints(det)
                det['kps_fusion_mean'] = np.array(m_)
                det['kps_fusion_std'] = np.array(s_)

        boxes = []
        if self.opt.use_pnp == True:  # noqa: E712
            boxes = self._pnp_all(results, meta)
        pnp_process_time = time.time()
        pnp_time += pnp_process_time - merge_outputs_time
        if self.opt.tracking_task:
            results, boxes = self.tracker.step(results, boxes)
            self.pre_images = images
        elif self.opt.refined_Kalman:
            results, boxes = self.tracker.step(results, boxes)
        end_time = time.time()
        track_time += end_time - pnp_process_time
        tot_time += end_time - start_time

        dict_out = self._dict_out(meta, boxes)
        if self.opt.debug >= 1:  # (nothing is constructed or drawn at debug 0: the timed path)
            from ..utils.debugger import Debugger
            debugger = Debugger(dataset=self.opt.dataset, ipynb=(self.opt.debug == 3), theme=self.opt.debugger_theme,
                                device=self.opt.device)   # base_detector.py:393
            if self.opt.debug < 4:
                self.show_results(debugger, image, results)
            elif self.opt.debug == 4:
                self.save_results(debugger, image, results, image_or_path_or_tensor, dict_out)
        return {'results': results, 'boxes': boxes, 'output': output, 'tot': tot_time, 'load': load_time,
                'pre': pre_time, 'net': net_time, 'dec': dec_time, 'post': post_time, 'merge': merge_time,
                'pnp': pnp_time, 'track': track_time}

    def run_batch(self, images, metas, draw=None):
        """Batched inference (added): ``images`` [B,3,H,W] already pre-processed (float32, on any device),
        ``metas`` a list of B meta dicts as produced by ``pre_process`` (+ 'camera_matrix').  Returns a list of
        B dicts with the keys of ``run`` ('results', 'boxes'); the network, decode and PnP each run once
        for the whole batch.  ``draw``: device uint8 frames [B,H,W,3] in the original image size; the detections are drawn
        into them in place (cp_draw_detections + cp_draw_primitives) behind the PnP, on its stream, before anything is read
        back.  The returned records do not depend on it."""
        t0 = time.time()
        images = images.to(self.opt.device)
        on_device = self.opt.device.type == 'cuda' and hasattr(self, 'post_process_merge_device')
        if draw is not None and not on_device:
            raise RuntimeError("run_batch: draw= needs the device post-process (a CUDA device)")
        self._skip_host_dets = on_device  # the packed detections stay on the device
        try:
            output, dets = self.process(images, None, None, None, None)
        finally:
            self._skip_host_dets = False
        self._sync()
        t1 = time.time()
        outs = []
        if on_device:
            # coordinate transform + threshold + soft-NMS of the whole batch in one launch (cp_postprocess)
            all_results = self.post_process_merge_device(metas, draw=draw)
        else:
            all_results = []
            for b, meta in enumerate(metas):
                d_b = {k: v[b:b + 1] for k, v in dets.items()}
                results = self.merge_outputs([self.post_process(d_b, meta, 1)])
                all_results.append(results)
        t2 = time.time()
        if self.opt.use_pnp == True:  # noqa: E712
            flat = [(b, k, d) for b, rs in enumerate(all_results) for k, d in enumerate(rs)]
            boxes_per = [[] for _ in metas]
            if flat:
                if on_device and getattr(self, 'pnp_dev', None) is not None:
                    # solved on the device straight from the post-processed records (cp_pnp_from_post): no per-detection
                    # host assembly, one copy of the [B,K,40] result
                    allraw = self.pnp_dev.cpu().numpy()
                    raw = [allraw[b, k] for b, k, _ in flat]
                else:
                    pts = [self._pnp_points(d) for _, _, d in flat]
                    scales = [np.asarray(d['obj_scale'], np.float64) / d['obj_scale'][1] for _, _, d in flat]
                    cams = np.stack([np.asarray(metas[b]['camera_matrix'], np.float64) for b, _, _ in flat])
                    raw = solve_pnp_batch(pts, scales, cams, device=self.opt.device)
                for (b, _, det), r in zip(flat, raw):
                    if int(r[0]) != 1:
                        continue
                    proj = r[8:24].reshape(8, 2).copy()
                    loc, quat = (list(r[4:7]), r[24:28].copy()) if self.opt.show_axes else \
                        (list(r[28:31]), r[31:35].copy())
                    ret = finish_detection(self.opt, metas[b], det, det['obj_scale'], loc, quat, proj)
                    if ret is not None:
                        boxes_per[b].append(ret)
        else:
            boxes_per = [[] for _ in metas]
        t3 = time.time()
        for b in range(len(metas)):
            outs.append({'results': all_results[b], 'boxes': boxes_per[b], 'net+dec': t1 - t0, 'post+merge': t2 - t1,
                         'pnp': t3 - t2})
        return outs

    def _demo_target(self):
        """`<demo_save>/<folder or source name>` (object_pose.py:394-401)."""
        if os.path.isdir(self.opt.demo):
            return os.path.join(self.opt.demo_save, os.path.basename(self.opt.demo))
        return os.path.join(self.opt.demo_save, os.path.splitext(os.path.basename(self.opt.demo))[0])

    def save_results(self, debugger, image, results, image_or_path_or_tensor, dict_out=None):
        """JSON side of object_pose.py:383-414 (ObjectPoseDetector.save_results adds the picture)."""
        target = self._demo_target()
        os.makedirs(target, exist_ok=True)
        if dict_out is not None and isinstance(image_or_path_or_tensor, str):
            name = os.path.splitext(os.path.basename(image_or_path_or_tensor))[0]
            with open(os.path.join(target, name + '.json'), 'w') as fp:
                json.dump(dict_out, fp)

    def reset_tracking(self):
        self.tracker.reset()
        self.pre_images = None
