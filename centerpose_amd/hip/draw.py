"""The overlay (cp_draw_*): primitive lists drawn into 8-bit frames on the device, the two list builders that read the
detector's and the tracker's device records, and what a host needs to write such lists itself -- the font's layout,
``text_size`` / ``text_primitives``, ``pack_primitives`` -- plus ``rasterize_host``, the same rule in numpy for frames that are
not on a device.  The rule is stated in csrc/draw_common.h."""
import ctypes

import torch

from . import _abi
from ._structs import (DRAW_COORD_MAX, DRAW_COORD_MIN, DRAW_DISC, DRAW_FILL, DRAW_GLYPH, DRAW_RECT, DRAW_SEGMENT,
                       DRAW_SLOTS, DrawParams)
from .detect import PNP_STRIDE, POST_STRIDE
from .track import TRACK_CAP

# the library's 5 x 7 font (csrc/draw_common.h: draw_glyph_bits; tests/test_draw_cpu.py compares the two), rows top to bottom,
# the most significant of the five bits on the left.  The space has no bitmap: it only advances the pen.
FONT = {
    "0": (0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110),
    "1": (0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110),
    "2": (0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111),
    "3": (0b11111, 0b00010, 0b00100, 0b00010, 0b00001, 0b10001, 0b01110),
    "4": (0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010),
    "5": (0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110),
    "6": (0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110),
    "7": (0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000),
    "8": (0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110),
    "9": (0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100),
    ".": (0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b01100, 0b01100),
    ":": (0b00000, 0b01100, 0b01100, 0b00000, 0b01100, 0b01100, 0b00000),
    "/": (0b00001, 0b00001, 0b00010, 0b00100, 0b01000, 0b10000, 0b10000),
    "-": (0b00000, 0b00000, 0b00000, 0b11111, 0b00000, 0b00000, 0b00000),
    "o": (0b00000, 0b00000, 0b01110, 0b10001, 0b10001, 0b10001, 0b01110),
    "p": (0b00000, 0b00000, 0b11110, 0b10001, 0b11110, 0b10000, 0b10000),
    "I": (0b01110, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110),
    "D": (0b11100, 0b10010, 0b10001, 0b10001, 0b10001, 0b10010, 0b11100),
    "P": (0b11110, 0b10001, 0b10001, 0b11110, 0b10000, 0b10000, 0b10000),
    "r": (0b00000, 0b00000, 0b10110, 0b11001, 0b10000, 0b10000, 0b10000),
    "e": (0b00000, 0b00000, 0b01110, 0b10001, 0b11111, 0b10000, 0b01110),
    "d": (0b00001, 0b00001, 0b01101, 0b10011, 0b10001, 0b10001, 0b01111),
    "F": (0b11111, 0b10000, 0b10000, 0b11110, 0b10000, 0b10000, 0b10000),
    "a": (0b00000, 0b00000, 0b01110, 0b00001, 0b01111, 0b10001, 0b01111),
    "m": (0b00000, 0b00000, 0b11010, 0b10101, 0b10101, 0b10001, 0b10001),
    "G": (0b01110, 0b10001, 0b10000, 0b10111, 0b10001, 0b10001, 0b01111),
    "T": (0b11111, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100),
    "n": (0b00000, 0b00000, 0b10110, 0b11001, 0b10001, 0b10001, 0b10001),
}
REQUIRED_CHARS = "0123456789 .:/-opIDPred"  # the reference's three label formats: 'op<score>', 'ID:<n>', 'Pred:a/b/c'


def glyph_bits(code):
    """The 35 bits of a character code (row r, column c at bit 5 r + 4 - c), 0 for a code that draws nothing."""
    rows = FONT.get(chr(code)) if 0 <= int(code) < 128 else None
    return sum(r << (5 * i) for i, r in enumerate(rows)) if rows else 0


def text_size(txt, scale):
    """(width, height) in pixels of ``txt`` at integer ``scale``: cells of pitch 6 scale, the last one without its gap."""
    n, s = len(txt), int(scale)
    return (6 * s * n - s if n else 0, 7 * s)


def text_primitives(txt, x, y, scale, colour):
    """One glyph primitive per character of ``txt``, the first cell's top-left at (x, y)."""
    s = int(scale)
    return [(DRAW_GLYPH, int(x) + 6 * s * i, int(y), 0, 0, s, int(colour), ord(ch)) for i, ch in enumerate(txt)]


def pack_primitives(prims, P):
    """A list of 8-tuples (one image), or a list of such lists (a batch), as the int32 array [P, 8] / [B, P, 8] that
    ``draw_primitives`` takes: drawing order = list order, the unused slots kind 0."""
    import numpy as np

    def scalar(v):
        return isinstance(v, (int, np.integer))

    batch = len(prims) > 0 and (len(prims[0]) == 0 or not scalar(prims[0][0]))  # (an empty list is one image without primitives)
    lists = prims if batch else [prims]
    out = np.zeros((len(lists), int(P), 8), np.int32)
    for b, lst in enumerate(lists):
        if len(lst) > P:
            raise ValueError("pack_primitives: %d primitives, %d slots" % (len(lst), P))
        if len(lst):
            out[b, :len(lst)] = np.asarray(lst, np.int64).reshape(len(lst), 8).clip(-2 ** 31, 2 ** 31 - 1)
    return out if batch else out[0]


def draw_params(opt=None, width=0, height=0, labels=False, **over):
    """cp_draw_params from a reference ``opt`` (vis_thresh, reg_bbox, show_axes, paper_display, tracking_task, debugger_theme)
    and the frame size; keyword arguments replace single fields."""
    g = (lambda n, d: getattr(opt, n, d)) if opt is not None else (lambda n, d: d)
    f = dict(vis_thresh=float(g("vis_thresh", 0.3)), reg_bbox=int(bool(g("reg_bbox", True))), show_axes=int(bool(g("show_axes", False))),
             paper_display=int(bool(g("paper_display", False))), tracking_task=int(bool(g("tracking_task", False))),
             theme=int(g("debugger_theme", "white") == "white"), labels=int(bool(labels)), width=int(width), height=int(height))
    f.update(over)
    return DrawParams(**f)


def _frames4(frames):
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() in (3, 4) and frames.shape[-1] == 3):
        raise RuntimeError("draw_primitives: frames must be a device uint8 tensor [B, H, W, 3] (or [H, W, 3])")
    f = frames if frames.dim() == 4 else frames[None]
    B, H, W = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
    if f.stride(3) != 1 or f.stride(2) != 3 or (B > 1 and f.stride(0) != H * f.stride(1)) or f.stride(1) < 3 * W:
        raise RuntimeError("draw_primitives: frames must be rows of packed BGR pixels, images H rows apart")
    return f, B, H, W


def workspace_bytes(B, P):
    return _abi.lib().cp_draw_workspace_bytes(int(B), int(P))


def draw_primitives(frames, prims, ws=None):
    """Draw ``prims`` (device int32 [B, P, 8], or [P, 8] for one frame) into ``frames`` (device uint8 [B, H, W, 3], rows may be
    pitched) in place, on the current stream, without synchronising.  ``ws``: a uint8 workspace of ``workspace_bytes(B, P)``."""
    f, B, H, W = _frames4(frames)
    p = prims if prims.dim() == 3 else prims[None]
    if not (p.is_cuda and p.dtype == torch.int32 and p.is_contiguous() and p.dim() == 3 and p.shape[0] == B and p.shape[2] == 8):
        raise RuntimeError("draw_primitives: prims must be a contiguous device int32 tensor [B, P, 8]")
    P = int(p.shape[1])
    L = _abi.lib()
    ws = _abi._workspace(L.cp_draw_workspace_bytes(B, P), f.device, given=ws)
    _abi._check_args(L.cp_draw_primitives(_abi._stream(), _abi._ptr(f), B, H, W, f.stride(1), _abi._ptr(p), P, _abi._ptr(ws),
                                          ws.numel()), "cp_draw_primitives")
    return frames


def draw_detections(post, count, det_pnp, cam, params, out=None):
    """The primitive list of a batch of detections, built on the device (cp_draw_detections): ``post`` [B, K, 120] / ``count``
    [B] of ``postprocess``, ``det_pnp`` [B, K, 40] of ``pnp_from_post`` or None, ``cam`` [B, 4] float64 (fx, fy, cx, cy) or
    None -> int32 [B, K * DRAW_SLOTS, 8]."""
    if not (post.is_cuda and post.dtype == torch.float64 and post.is_contiguous() and post.dim() == 3 and post.shape[2] == POST_STRIDE
            and count.is_cuda and count.dtype == torch.int32):
        raise RuntimeError("draw_detections: post [B,K,120] float64 / count [B] int32 device tensors expected")
    B, K = int(post.shape[0]), int(post.shape[1])
    if det_pnp is not None and not (det_pnp.is_cuda and det_pnp.dtype == torch.float64 and det_pnp.is_contiguous() and
                                    tuple(det_pnp.shape) == (B, K, PNP_STRIDE)):
        raise RuntimeError("draw_detections: det_pnp must be the [B,K,40] float64 output of pnp_from_post")
    cam = _cam(cam, B, post.device)
    out = _out(out, B, K, post.device)
    _abi._check_args(_abi.lib().cp_draw_detections(_abi._stream(), *_abi._ptrs(post, count, det_pnp, cam), B, K, ctypes.byref(params),
                                                   _abi._ptr(out)), "cp_draw_detections")
    return out


def draw_tracks(state, B, cap, cam, params, out=None):
    """The primitive list of the tracks in this frame's ``boxes`` (cp_draw_tracks): ``state`` is ``DeviceTracker.state`` ->
    int32 [B, cap * DRAW_SLOTS, 8]."""
    B, cap = int(B), int(cap)
    if not (state.is_cuda and state.dtype == torch.uint8) or not 1 <= cap <= TRACK_CAP or \
            state.numel() < _abi.lib().cp_track_state_bytes(B, cap):
        raise RuntimeError("draw_tracks: state must be the device buffer of cp_track_state_bytes(B, cap) bytes")
    cam = _cam(cam, B, state.device)
    out = _out(out, B, cap, state.device)
    _abi._check_args(_abi.lib().cp_draw_tracks(_abi._stream(), _abi._ptr(state), B, cap, _abi._ptr(cam), ctypes.byref(params),
                                               _abi._ptr(out)), "cp_draw_tracks")
    return out


def _cam(cam, B, device):
    if cam is None:
        return None
    cam = torch.as_tensor(cam, dtype=torch.float64).reshape(B, 4).contiguous()
    return cam if cam.is_cuda else cam.to(device)


def _out(out, B, K, device):
    if out is None:
        return torch.empty(B, K * DRAW_SLOTS, 8, dtype=torch.int32, device=device)
    if not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (B, K * DRAW_SLOTS, 8)):
        raise RuntimeError("draw: out must be a contiguous device int32 tensor [B, %d, 8]" % (K * DRAW_SLOTS))
    return out


def cam_rows(metas):
    """[B, 4] float64 (fx, fy, cx, cy) from the metas' 'camera_matrix', or None when one has none."""
    import numpy as np

    if not all("camera_matrix" in m for m in metas):
        return None
    Ks = [np.asarray(m["camera_matrix"], np.float64) for m in metas]
    return np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]] for K in Ks])


# ---- the same rule on the host, in numpy: frames that are not on a device (the Debugger on a CPU-only machine) ----
def _seg(X, Y, x0, y0, x1, y1, t):
    import numpy as np

    dx, dy, wx, wy = x1 - x0, y1 - y0, X - x0, Y - y0
    L2, s = dx * dx + dy * dy, wx * dx + wy * dy
    near0 = 4 * (wx * wx + wy * wy) <= t * t
    near1 = 4 * ((X - x1) ** 2 + (Y - y1) ** 2) <= t * t
    cr = wx * dy - wy * dx
    return np.where((L2 == 0) | (s <= 0), near0, np.where(s >= L2, near1, 4 * cr * cr <= t * t * L2))


def rasterize_host(frame, prims):
    """``prims`` (anything ``numpy.asarray`` reads as [P, 8]) into the uint8 array ``frame`` [H, W, 3], in place: the rule of
    csrc/draw_common.h in int64 numpy, primitive by primitive over its clipped bounding box."""
    import numpy as np

    H, W = frame.shape[:2]
    for kind, x0, y0, x1, y1, size, colour, aux in np.asarray(prims, np.int64).reshape(-1, 8).tolist():
        if not all(DRAW_COORD_MIN <= v <= DRAW_COORD_MAX for v in (x0, y0, x1, y1)):
            continue
        if kind in (DRAW_SEGMENT, DRAW_RECT):
            if not 1 <= size <= 16:
                continue
            m = (size + 1) // 2
            box = (min(x0, x1) - m, min(y0, y1) - m, max(x0, x1) + m, max(y0, y1) + m)
        elif kind == DRAW_DISC:
            if not 0 <= size <= 64:
                continue
            box = (x0 - size, y0 - size, x0 + size, y0 + size)
        elif kind == DRAW_FILL:
            box = (min(x0, x1), min(y0, y1), max(x0, x1), max(y0, y1))
        elif kind == DRAW_GLYPH:
            if not 1 <= size <= 8 or glyph_bits(aux) == 0:
                continue
            box = (x0, y0, x0 + 5 * size - 1, y0 + 7 * size - 1)
        else:
            continue
        lx, ly, hx, hy = max(box[0], 0), max(box[1], 0), min(box[2], W - 1), min(box[3], H - 1)
        if lx > hx or ly > hy:
            continue
        Y, X = np.mgrid[ly:hy + 1, lx:hx + 1].astype(np.int64)
        if kind == DRAW_SEGMENT:
            cov = _seg(X, Y, x0, y0, x1, y1, size)
        elif kind == DRAW_DISC:
            cov = (X - x0) ** 2 + (Y - y0) ** 2 <= size * size
        elif kind == DRAW_RECT:
            cov = _seg(X, Y, x0, y0, x1, y0, size) | _seg(X, Y, x1, y0, x1, y1, size) | _seg(X, Y, x1, y1, x0, y1, size) | \
                _seg(X, Y, x0, y1, x0, y0, size)
        elif kind == DRAW_FILL:
            cov = np.ones(X.shape, bool)
        else:
            bits = glyph_bits(aux)
            cov = ((bits >> (5 * ((Y - y0) // size) + 4 - (X - x0) // size)) & 1).astype(bool)
        frame[ly:hy + 1, lx:hx + 1][cov] = (colour & 0xFF, (colour >> 8) & 0xFF, (colour >> 16) & 0xFF)
    return frame
