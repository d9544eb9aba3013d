"""The oracle of the overlay tests: the rasterising rule of centerpose_amd/csrc/draw_common.h restated in int64 numpy.  It
loops over the primitives of an image in order and evaluates each on the whole frame (no bounding boxes, no tiles), so it shares
no structure with the device kernels or with the host build.  It is this project's own rule: comparisons are bit for bit."""
import numpy as np

from centerpose_amd.hip import draw as hd

CMIN, CMAX = -8192, 8191


def _seg(X, Y, x0, y0, x1, y1, t):
    dx, dy, wx, wy = x1 - x0, y1 - y0, X - x0, Y - y0
    L2, s = dx * dx + dy * dy, wx * dx + wy * dy
    cr = wx * dy - wy * dx
    out = 4 * cr * cr <= t * t * L2
    out = np.where(s >= L2, 4 * ((X - x1) ** 2 + (Y - y1) ** 2) <= t * t, out)
    return np.where((s <= 0) | (L2 == 0), 4 * (wx * wx + wy * wy) <= t * t, out)


def covers(p, H, W):
    """bool [H, W]: the pixels the primitive ``p`` (8 ints) covers; all False for a primitive the rule skips."""
    kind, x0, y0, x1, y1, size, _, aux = [int(v) for v in p]
    none = np.zeros((H, W), bool)
    if not all(CMIN <= v <= CMAX for v in (x0, y0, x1, y1)):
        return none
    Y, X = np.mgrid[0:H, 0:W].astype(np.int64)
    if kind == 1:
        return _seg(X, Y, x0, y0, x1, y1, size) if 1 <= size <= 16 else none
    if kind == 2:
        return (X - x0) ** 2 + (Y - y0) ** 2 <= size * size if 0 <= size <= 64 else none
    if kind == 3:
        if not 1 <= size <= 16:
            return none
        c = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
        return np.logical_or.reduce([_seg(X, Y, *c[i], *c[(i + 1) % 4], size) for i in range(4)])
    if kind == 4:
        return (X >= min(x0, x1)) & (X <= max(x0, x1)) & (Y >= min(y0, y1)) & (Y <= max(y0, y1))
    if kind == 5:
        bits = hd.glyph_bits(aux) if 0 <= aux < 256 else 0
        if not 1 <= size <= 8 or bits == 0:
            return none
        gx, gy = X - x0, Y - y0
        inside = (gx >= 0) & (gy >= 0) & (gx < 5 * size) & (gy < 7 * size)
        bit = (bits >> np.clip(5 * (gy // size) + 4 - gx // size, 0, 62)) & 1
        return inside & (bit == 1)
    return none


def draw_image(img, prims):
    """``prims`` [P, 8] into the uint8 array ``img`` [H, W, 3] (a view is fine: only covered pixels are written), in order."""
    H, W = img.shape[:2]
    for p in np.asarray(prims, np.int64).reshape(-1, 8):
        if p[0] == 0:
            continue
        c = int(p[6])
        img[covers(p, H, W)] = (c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF)
    return img


def draw_pitched(buf, B, H, W, pitch, prims):
    """A copy of the pitched uint8 buffer ``buf`` [B * H * pitch] with ``prims`` [B, P, 8] drawn; pad bytes untouched."""
    out = np.array(buf, np.uint8).reshape(B, H, pitch).copy()
    for b in range(B):
        view = out[b, :, :3 * W].reshape(H, W, 3)
        draw_image(view, prims[b])
    return out.reshape(-1)
