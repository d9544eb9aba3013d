"""Everything between a frame and its poses except the network: preprocess / resize / render, the decode (whole, tiled, or
as peaks + gathered tables), post-process, PnP, and ``PoseStage``, which runs the last two on a side stream.  The
detection, post-processed and pose record layouts are here too."""
import ctypes
import os
from collections import OrderedDict

import torch

from . import _abi

DET_FIELDS = OrderedDict([  # field -> (offset, width) inside a 118-float detection record (decode.py:347-361)
    ("bboxes", (0, 4)), ("scores", (4, 1)), ("kps", (5, 16)), ("clses", (21, 1)), ("obj_scale", (22, 3)),
    ("obj_scale_uncertainty", (25, 3)), ("tracking", (28, 2)), ("tracking_hp", (30, 16)),
    ("kps_displacement_mean", (46, 16)), ("kps_displacement_std", (62, 16)), ("kps_heatmap_mean", (78, 16)),
    ("kps_heatmap_std", (94, 16)), ("kps_heatmap_height", (110, 8))])
DET_STRIDE = 118


def _decode(tiled, hm, hps, wh, hm_hp, optional, K, rep_mode, fit_gaussian, balance, legacy_bool_mask, apply_sigmoid):
    """decode_raw (cp_decode) and decode_raw_tiled (cp_decode_tiled): one argument list, two entry points."""
    L = _abi.lib()
    name = "decode_tiled" if tiled else "decode"
    for t in (hm, hps, wh, hm_hp):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise RuntimeError("%s: required heads must be contiguous float32 device tensors" % name)
    opt = [_abi._dev_opt(t) for t in optional]
    B, _, H, W = hm.shape
    n = L.cp_decode_tiled_workspace_bytes(B, H, W, int(K)) if tiled else L.cp_decode_workspace_bytes(B, K)
    if tiled and n == 0:
        raise RuntimeError("decode_tiled: unsupported shape B=%d H=%d W=%d K=%d (need 1 <= K <= 128, K <= H*W <= 1048576, "
                           "W %% 4 == 0, W <= 4096)" % (B, H, W, K))
    det = torch.empty(B, K, DET_STRIDE, device=hm.device, dtype=torch.float32)
    ws = _abi._workspace(n, hm.device)
    rc = getattr(L, "cp_" + name)(_abi._stream(), B, H, W, *_abi._ptrs(hm, hps, wh, *opt[:4], hm_hp, *opt[4:]), int(K),
                                  int(rep_mode), int(bool(fit_gaussian)), float(balance), int(bool(legacy_bool_mask)),
                                  int(bool(apply_sigmoid)), _abi._ptr(det), _abi._ptr(ws), n)
    _abi._check(rc, "cp_" + name)
    return det


def decode_raw(hm, hps, wh, hm_hp, hps_uncertainty=None, scale=None, scale_uncertainty=None, reg=None,
               hp_offset=None, tracking=None, tracking_hp=None, K=100, rep_mode=1, fit_gaussian=False,
               balance=2.0, legacy_bool_mask=False, apply_sigmoid=False):
    """Device decode -> det [B,K,118] (device tensor).  hm / hm_hp are modified in place when
    apply_sigmoid is set.  Tensors must be contiguous float32 NCHW on the HIP device."""
    return _decode(False, hm, hps, wh, hm_hp, (hps_uncertainty, scale, scale_uncertainty, reg, hp_offset, tracking, tracking_hp),
                   K, rep_mode, fit_gaussian, balance, legacy_bool_mask, apply_sigmoid)


def decode_raw_tiled(hm, hps, wh, hm_hp, hps_uncertainty=None, scale=None, scale_uncertainty=None, reg=None,
                     hp_offset=None, tracking=None, tracking_hp=None, K=100, rep_mode=1, fit_gaussian=False,
                     balance=2.0, legacy_bool_mask=False, apply_sigmoid=False):
    """``decode_raw`` through cp_decode_tiled: the same records, bit for bit, for output grids of any size up to 1048576
    pixels (W % 4 == 0, W <= 4096, K <= 128).  The workspace grows with H*W and is sized here."""
    return _decode(True, hm, hps, wh, hm_hp, (hps_uncertainty, scale, scale_uncertainty, reg, hp_offset, tracking, tracking_hp),
                   K, rep_mode, fit_gaussian, balance, legacy_bool_mask, apply_sigmoid)


def split_detections(det):
    """[B,K,118] -> dict of the 13 reference keys (views)."""
    return OrderedDict((k, det[..., o:o + w]) for k, (o, w) in DET_FIELDS.items())


# heads the decode reads at the peaks only (every head but the two heat-maps); hp_offset at the joint peaks, the rest at the centres
_MAP_HEADS = ("hm", "hm_hp")


def decode_peaks(hm, hm_hp, K=100, apply_sigmoid=False):
    """The first half of the decode (cp_decode_peaks): NMS + top-K of hm [B,1,H,W] and hm_hp [B,8,H,W] ->
    (pk_score float32 [B,9,K], pk_ind int32 [B,9,K]); index = y * W + x, map 0 = hm, 1..8 = hm_hp.  Any grid decode_raw or
    decode_raw_tiled accepts."""
    L = _abi.lib()
    hm, hm_hp = _abi._dev(hm), _abi._dev(hm_hp)
    B, _, H, W = hm.shape
    n = L.cp_decode_peaks_workspace_bytes(B, H, W, int(K))
    if n == 0:
        raise RuntimeError("cp_decode_peaks: unsupported shape")
    ws = _abi._workspace(n, hm.device)
    pk_score = torch.empty(B, 9, K, device=hm.device, dtype=torch.float32)
    pk_ind = torch.empty(B, 9, K, device=hm.device, dtype=torch.int32)
    _abi._check(L.cp_decode_peaks(_abi._stream(), B, H, W, _abi._ptr(hm), _abi._ptr(hm_hp), int(K), int(bool(apply_sigmoid)),
                                  *_abi._ptrs(pk_score, pk_ind, ws), ws.numel()), "cp_decode_peaks")
    return pk_score, pk_ind


def decode_gathered(hm_hp, pk_score, pk_ind, hps, wh, hps_uncertainty=None, scale=None, scale_uncertainty=None, reg=None,
                    hp_offset=None, tracking=None, tracking_hp=None, rep_mode=1, fit_gaussian=False, balance=2.0,
                    legacy_bool_mask=False):
    """The second half of the decode on COMPACT tables (cp_decode_gathered): each regression head holds its values at the
    peaks only -- [B,C,K] at the centre peaks pk_ind[:, 0], hp_offset [B,8,2,K] at the joint peaks pk_ind[:, 1:] -- and
    hm_hp is the dense (sigmoided) map.  -> det [B,K,118], bit-identical to decode_raw on maps holding the same values."""
    L = _abi.lib()
    hm_hp = _abi._dev(hm_hp)
    B, _, H, W = hm_hp.shape
    K = pk_ind.shape[2]
    opt = [_abi._dev_opt(t) for t in (hps, wh, hps_uncertainty, scale, scale_uncertainty, reg, hp_offset, tracking, tracking_hp)]
    want = (16, 2, 16, 3, 3, 2, None, 2, 16)
    for t, c in zip(opt, want):
        if t is not None and tuple(t.shape) != ((B, 8, 2, K) if c is None else (B, c, K)):
            raise ValueError("decode_gathered: a table has shape %s" % (tuple(t.shape),))
    det = torch.empty(B, K, DET_STRIDE, device=hm_hp.device, dtype=torch.float32)
    pk_score, pk_ind = pk_score.contiguous(), pk_ind.contiguous()
    if pk_score.dtype != torch.float32 or pk_ind.dtype != torch.int32:
        raise ValueError("decode_gathered: pk_score float32 and pk_ind int32 expected")
    _abi._check(L.cp_decode_gathered(_abi._stream(), B, H, W, *_abi._ptrs(hm_hp, *opt, pk_score, pk_ind),
                                     int(K), int(rep_mode), int(bool(fit_gaussian)), float(balance), int(bool(legacy_bool_mask)),
                                     _abi._ptr(det)), "cp_decode_gathered")
    return det


def preprocess(image_u8_hwc, trans_input, mean, std, out_h, out_w):
    """Device warp + normalise of one BGR uint8 frame [H,W,3] -> float32 [1,3,out_h,out_w]
    (BaseDetector.pre_process, base_detector.py:127-134).  ``trans_input`` is the 2x3 source->input affine."""
    import numpy as np

    L = _abi.lib()
    if not (image_u8_hwc.is_cuda and image_u8_hwc.dtype == torch.uint8 and image_u8_hwc.is_contiguous()):
        raise RuntimeError("preprocess: image must be a contiguous uint8 device tensor [H,W,3]")
    H, W = int(image_u8_hwc.shape[0]), int(image_u8_hwc.shape[1])
    fwd = np.asarray(trans_input, np.float64).reshape(-1)
    out = torch.empty(1, 3, out_h, out_w, device=image_u8_hwc.device, dtype=torch.float32)
    rc = L.cp_preprocess(_abi._stream(), _abi._ptr(image_u8_hwc), H, W, (ctypes.c_double * 6)(*fwd.tolist()),
                         _abi._float3(mean), _abi._float3(std), _abi._ptr(out), out_h, out_w)
    _abi._check(rc, "cp_preprocess")
    return out


def preprocess_batch(images_u8_bhwc, trans_input, mean, std, out_h, out_w, out=None):
    """`preprocess` for B frames of one size sharing the transform: uint8 [B,H,W,3] -> float32 [B,3,out_h,out_w], one launch."""
    import numpy as np

    L = _abi.lib()
    t = images_u8_bhwc
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 4 and t.shape[3] == 3):
        raise RuntimeError("preprocess_batch: images must be a contiguous uint8 device tensor [B,H,W,3]")
    B, H, W = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    fwd = np.asarray(trans_input, np.float64).reshape(-1)
    if out is None:
        out = torch.empty(B, 3, out_h, out_w, device=t.device, dtype=torch.float32)
    rc = L.cp_preprocess_batch(_abi._stream(), _abi._ptr(t), B, H, W, (ctypes.c_double * 6)(*fwd.tolist()),
                               _abi._float3(mean), _abi._float3(std), _abi._ptr(out), out_h, out_w)
    _abi._check(rc, "cp_preprocess_batch")
    return out


def resize_u8(image_u8_hwc, out_h, out_w):
    """cv2.resize(img, (out_w, out_h)) (INTER_LINEAR, OpenCV's fixed-point form) of a uint8 [H,W,C] device frame."""
    L = _abi.lib()
    if not (image_u8_hwc.is_cuda and image_u8_hwc.dtype == torch.uint8 and image_u8_hwc.is_contiguous()
            and image_u8_hwc.dim() == 3):
        raise RuntimeError("resize_u8: image must be a contiguous uint8 device tensor [H,W,C]")
    H, W, C = (int(v) for v in image_u8_hwc.shape)
    out = torch.empty(out_h, out_w, C, device=image_u8_hwc.device, dtype=torch.uint8)
    _abi._check(L.cp_resize_u8(_abi._stream(), _abi._ptr(image_u8_hwc), H, W, C, _abi._ptr(out), out_h, out_w), "cp_resize_u8")
    return out


def render_gaussians(records, C, H, W, device, out=None):
    """Draw (channel, x, y, radius, k) Gaussians into a float32 [C,H,W] device map with max() merging
    (draw_umich_gaussian, utils/image.py:135-150): the pre_hm / pre_hm_hp render of CenterPoseTrack."""
    L = _abi.lib()
    rec = torch.as_tensor(records, dtype=torch.float64).reshape(-1, 5).contiguous().to(device)
    if out is None:
        out = torch.empty(C, H, W, dtype=torch.float32, device=device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (C, H, W)):
        raise RuntimeError("render_gaussians: out must be a contiguous float32 device tensor [C,H,W]")
    _abi._check(L.cp_render_gaussians(_abi._stream(), _abi._ptr(rec) if rec.numel() else None, int(rec.shape[0]), _abi._ptr(out),
                                      C, H, W, 1), "cp_render_gaussians")
    return out


POST_STRIDE = 120
POST_FIELDS = OrderedDict([  # field -> (offset, width) inside a post-processed record (post_process.py:21-58)
    ("score", (0, 1)), ("cls", (1, 1)), ("obj_scale", (2, 3)), ("obj_scale_uncertainty", (5, 3)),
    ("kps_displacement_std", (8, 16)), ("bbox", (24, 4)), ("ct", (28, 2)), ("kps", (30, 16)), ("tracking", (46, 2)),
    ("tracking_hp", (48, 16)), ("kps_displacement_mean", (64, 16)), ("kps_heatmap_mean", (80, 16)),
    ("kps_heatmap_std", (96, 16)), ("kps_heatmap_height", (112, 8))])


def postprocess(det, meta, vis_thresh, nms=True, div_scale=1.0, out=None, cnt=None, ws=None):
    """Device post-process + Gaussian soft-NMS of a whole batch (object_pose.py:167-197).
    det [B,K,118] float32 device; meta [B,8] float64 (inverse affine 6, ratio, pad) -> (records [B,K,120] float64
    device, counts [B] int32 device); image b keeps records[b, :counts[b]] in the reference's final order.
    ``out`` / ``cnt`` / ``ws``: caller-owned result and workspace tensors (PoseStage rotates its own)."""
    L = _abi.lib()
    if not (det.is_cuda and det.dtype == torch.float32 and det.is_contiguous() and det.dim() == 3
            and det.shape[2] == DET_STRIDE):
        raise RuntimeError("postprocess: det must be a contiguous float32 device tensor [B,K,118]")
    B, K = int(det.shape[0]), int(det.shape[1])
    meta = torch.as_tensor(meta, dtype=torch.float64).reshape(B, 8).contiguous().to(det.device)
    if out is None:
        out = torch.empty(B, K, POST_STRIDE, dtype=torch.float64, device=det.device)
    if cnt is None:
        cnt = torch.empty(B, dtype=torch.int32, device=det.device)
    n = L.cp_postprocess_workspace_bytes(B, K)
    ws = _abi._workspace(n, det.device, given=ws)
    if tuple(out.shape) != (B, K, POST_STRIDE) or out.dtype != torch.float64 or cnt.numel() != B or ws.numel() < n:
        raise RuntimeError("postprocess: out / cnt / ws do not fit this batch")
    rc = L.cp_postprocess(_abi._stream(), _abi._ptr(det), B, K, _abi._ptr(meta), float(vis_thresh), int(bool(nms)),
                          float(div_scale), *_abi._ptrs(out, cnt, ws), n)
    _abi._check(rc, "cp_postprocess")
    return out, cnt


PNP_STRIDE = 40


def pnp_solve(pts, scale, cam):
    """Batched cuboid PnP.  pts [N,npts,2] float32 (npts 8 or 16), scale [N,3] float32, cam [N,4] float64
    (fx, fy, cx, cy); all on the HIP device.  Returns out [N,40] float64 (layout: centerpose_hip.h)."""
    L = _abi.lib()
    _abi._on_device(pts, scale, cam, what="pnp_solve")
    pts = pts.contiguous().float()
    scale = scale.contiguous().float()
    cam = cam.contiguous().double()
    N, npts = pts.shape[0], pts.shape[1]
    out = torch.zeros(N, PNP_STRIDE, device=pts.device, dtype=torch.float64)
    if N == 0:
        return out
    ws = _abi._workspace(L.cp_pnp_workspace_bytes(N), pts.device)
    _abi._check(L.cp_pnp_solve(_abi._stream(), *_abi._ptrs(pts, scale, cam), N, npts, _abi._ptr(out), _abi._ptr(ws), ws.numel()),
                "cp_pnp_solve")
    return out


_pnp_ws_cache = {}


def pnp_from_post(post, count, cam, rep_mode=1, out=None, ws=None):
    """PnP of every post-processed slot on the device (cp_pnp_from_post): post [B,K,120] float64 + count [B] int32 from
    ``postprocess``, cam [B,4] float64 (fx, fy, cx, cy).  Returns [B,K,40] float64; rows k >= count[b] carry status -1.
    No host synchronisation.  ``out`` / ``ws``: caller-owned result and workspace (default: a fresh result and one
    cached workspace per (shape, device, stream) -- launches on the same stream are ordered, so they may share it)."""
    L = _abi.lib()
    B, K = int(post.shape[0]), int(post.shape[1])
    if not (post.is_cuda and post.dtype == torch.float64 and post.is_contiguous() and count.is_cuda and cam.is_cuda):
        raise RuntimeError("pnp_from_post: contiguous device tensors expected (no CPU path)")
    cam = cam.contiguous().double().reshape(B, 4)
    if out is None:
        out = torch.empty(B, K, PNP_STRIDE, dtype=torch.float64, device=post.device)
    n = L.cp_pnp_from_post_workspace_bytes(B, K)
    if ws is None:
        key = (B, K, post.device, torch.cuda.current_stream(post.device).cuda_stream)
        ws = _pnp_ws_cache.get(key)
        if ws is None:
            if len(_pnp_ws_cache) >= 16:
                _pnp_ws_cache.clear()
            ws = _pnp_ws_cache[key] = _abi._workspace(n, post.device)
    if tuple(out.shape) != (B, K, PNP_STRIDE) or out.dtype != torch.float64 or ws.numel() < n:
        raise RuntimeError("pnp_from_post: out / ws do not fit this batch")
    _abi._check(L.cp_pnp_from_post(_abi._stream(), _abi._ptr(post), _abi._ptr(count), B, K, int(rep_mode),
                                   *_abi._ptrs(cam, out, ws), n), "cp_pnp_from_post")
    return out


_masked_streams = {}   # (device index, n_cus) -> (handle, torch stream): ONE stream per mask for the life of the process (every
                       # hipExtStreamCreateWithCUMask is a hardware queue of its own; a process that kept creating them would
                       # push its other streams onto shared queues)


def masked_stream(device, n_cus):
    """A HIP stream whose kernels may only run on the first ``n_cus`` compute units (hipExtStreamCreateWithCUMask; bits are spread
    over the XCDs by the runtime), wrapped as a torch stream.  For latency-bound side work that must not take registers away from
    the kernels of the main stream everywhere on the chip: the batched PnP solve holds 286 - 330 vector registers per wavefront
    -- one such wave takes more than half of a SIMD's register file for the ~0.5 ms of its Levenberg-Marquardt walk, and a few
    hundred of them spread over all 1024 SIMDs cost the network kernels they overlap ~0.3 ms per step (profiles/NOTES.md round 6)."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(n_cus))
    if key in _masked_streams:
        return _masked_streams[key][1]
    rt = ctypes.CDLL("libamdhip64.so")
    words = (int(n_cus) + 31) // 32
    mask = (ctypes.c_uint32 * words)()
    for i in range(int(n_cus)):
        mask[i // 32] |= 1 << (i % 32)
    h = ctypes.c_void_p()
    with torch.cuda.device(dev):
        rc = rt.hipExtStreamCreateWithCUMask(ctypes.byref(h), ctypes.c_uint32(words), mask)
    if rc != 0 or not h.value:
        raise RuntimeError("hipExtStreamCreateWithCUMask failed with code %d" % rc)
    st = torch.cuda.ExternalStream(h.value, device=dev)
    _masked_streams[key] = (h, st)
    return st


class PoseStage(object):
    """Post-process + soft-NMS + batched PnP of decoded batches (base_detector.py:547-654 for a whole batch), with the
    PnP -- and, from 8 images per batch, the post-process -- on a side stream.  The solve is at most B*K independent float64 problems of ~1e5 operations each: a few dozen
    wavefronts whose run time is the slowest lane's Levenberg-Marquardt walk (0.5 - 2.5 ms), during which the rest of
    the chip would idle.  ``submit`` therefore queues the solve (and the post-process of a batch of 8 or more, behind a copy of the
    decoded records) on the stage's own stream, so that the solve of batch i runs under the network of batch i+1; ``depth`` sets of result buffers
    rotate, and the caller's stream waits for the solve that last used a set before post-process overwrites it.

    submit() -> (post [B,K,120], count [B], poses [B,K,40], done): the tensors are valid once ``done`` (a
    torch.cuda.Event) has completed -- ``done.synchronize()`` on the host or ``stream.wait_event(done)``.
    Caller-owned inputs (``det``, ``meta``, ``cam``) are read on the side stream as well: the stage tells the caching
    allocator (``record_stream``), so the caller may drop them right after ``submit``."""

    # batches of at least this many images post-process on the side stream too (below: on the caller's, one hop less per frame);
    # $CP_POST_SIDE_FROM overrides (A/B runs)
    SIDE_POST_FROM = int(os.environ.get("CP_POST_SIDE_FROM", "8"))

    def __init__(self, B, K, device, depth=2, cus=None):
        """``cus``: run the solve on a stream restricted to that many compute units (``masked_stream``); None = $CP_PNP_CUS or,
        unset, 32 (B = 64, 1650 mostly ill-posed detections per batch, profiles/r06_pnp_cu_mask_ab.txt: the first layers of the
        next batch, which the solve overlaps, 1.60 -> 1.45 ms, step 18.74 -> 18.63 ms with the longer solve's tail included; 8 / 16
        CUs stretch the solve to 5.4 / 3.4 ms and lose); 0 = an ordinary stream (the solve's waves land on every CU)."""
        L = _abi.lib()
        self.B, self.K, self.depth, self.i = int(B), int(K), int(depth), 0
        if cus is None:
            cus = int(os.environ.get("CP_PNP_CUS", "32"))
        self.cus = int(cus)
        self.side = None
        if self.cus > 0:
            try:
                self.side = masked_stream(device, self.cus)
            except (RuntimeError, OSError, AttributeError):   # runtime without the extension: an ordinary stream does the same work
                self.cus = 0
        if self.side is None:
            self.side = torch.cuda.Stream(device=device)
        n_post, n_pnp = L.cp_postprocess_workspace_bytes(B, K), L.cp_pnp_from_post_workspace_bytes(B, K)
        self.sets = []
        for _ in range(self.depth):
            self.sets.append(dict(
                post=torch.empty(B, K, POST_STRIDE, dtype=torch.float64, device=device),
                cnt=torch.empty(B, dtype=torch.int32, device=device),
                poses=torch.empty(B, K, PNP_STRIDE, dtype=torch.float64, device=device),
                det=torch.empty(B, K, DET_STRIDE, dtype=torch.float32, device=device),
                meta=torch.empty(B, 8, dtype=torch.float64, device=device),
                ws_post=_abi._workspace(n_post, device), ws_pnp=_abi._workspace(n_pnp, device),
                ready=torch.cuda.Event(), done=torch.cuda.Event(enable_timing=True),
                begin=torch.cuda.Event(enable_timing=True)))
        self._timed = []

    def submit(self, det, meta, cam, vis_thresh, nms=True, rep_mode=1):
        s = self.sets[self.i % self.depth]
        first_use = self.i < self.depth
        self.i += 1
        main = torch.cuda.current_stream()
        if not first_use:
            main.wait_event(s["done"])  # the post-process / solve that read this set `depth` batches ago
        B = int(det.shape[0])
        side_post = B >= self.SIDE_POST_FROM
        if side_post:
            # the post-process (one latency-bound launch of ~0.15 ms at B = 64: a serial soft-NMS walk per image) joins the solve on the
            # side stream; the caller's stream only copies the decoded records (3 MB) and the per-image affine into the set, so the
            # caller may overwrite `det` / `meta` with the next batch at once
            s["det"][:B].copy_(det, non_blocking=True)
            s["meta"][:B].copy_(torch.as_tensor(meta, dtype=torch.float64).reshape(B, 8).to(det.device), non_blocking=True)
        else:
            postprocess(det, meta, vis_thresh, nms=nms, out=s["post"], cnt=s["cnt"], ws=s["ws_post"])
        s["ready"].record(main)
        if torch.is_tensor(cam) and cam.is_cuda:
            cam.record_stream(self.side)  # read by the solve after this call returns
        with torch.cuda.stream(self.side):
            self.side.wait_event(s["ready"])
            s["begin"].record(self.side)
            if side_post:
                postprocess(s["det"][:B], s["meta"][:B], vis_thresh, nms=nms, out=s["post"], cnt=s["cnt"], ws=s["ws_post"])
            pnp_from_post(s["post"], s["cnt"], cam, rep_mode=rep_mode, out=s["poses"], ws=s["ws_pnp"])
            s["done"].record(self.side)
        self._timed = [(s["begin"], s["done"])]
        return s["post"], s["cnt"], s["poses"], s["done"]

    def take_solve_ms(self):
        """Milliseconds the most recent assembly + solve took on the side stream (synchronises on it); None before the
        first submit."""
        if not self._timed:
            return None
        b, d = self._timed[-1]
        d.synchronize()
        return b.elapsed_time(d)
