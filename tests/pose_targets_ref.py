"""Host restatement of the ObjectPose training targets (cp_pose_targets, centerpose_amd/pose_targets.py) in numpy: from the
records of ``pack_annotations`` to the arrays of the dataset's ``ret`` for one image ([S, ...]) or a batch ([B, S, ...]).

It restates datasets/dataset_combined.py:957-1130 in float64 / float32 / int64 with the reference's rounding points:
the variant projection truncated with int(), corners truncated into int64 after the visibility test, the affine of a
point taken in float32 and multiplied in float64, the joints assigned back into int64, gaussian_radius with its
(b + sq) / 2, and draw_umich_gaussian's float64 Gaussian merged into the float32 map by a max.  Every float64 sum is
written out in the order the device evaluates it, so the host build of pose_targets_common.h matches it bit for bit.
"""
import math
from fractions import Fraction

import numpy as np

from centerpose_amd import hip

J = 8
FLIP_SWAPS = ((0, 4), (2, 6), (1, 5), (3, 7))  # opt.flip_idx [[1,5],[3,7],[2,6],[4,8]] on the 8 corners
I, O = hip.PT_IMG, hip.PT_OBJ


def _trunc(v):
    """int(v) / an assignment into int64 (toward zero), clamped as the device clamps far-away points."""
    if not v < 4.0e18:
        return 0 if v != v else 4000000000000000000
    if not v > -4.0e18:
        return -4000000000000000000
    return int(v)


def fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic; math.fma needs Python 3.13)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def affine(t, x, y):
    """affine_transform: the point through float32, then np.dot's row evaluation fma(t0, x, t1 * y) + t2 in float64."""
    fx, fy = float(np.float32(x)), float(np.float32(y))
    return fma(t[0], fx, t[1] * fy) + t[2], fma(t[3], fx, t[4] * fy) + t[5]


def _mat4(a, b):
    c = [0.0] * 16
    for i in range(4):
        for j in range(4):
            s = a[i * 4] * b[j]
            for k in range(1, 4):
                s = s + a[i * 4 + k] * b[k * 4 + j]
            c[i * 4 + j] = s
    return c


def project(img, obj, s, S):
    """The variant projection of the 9 keypoints: [(int(vp[1]), int(vp[0]))] and the unrounded (vp[1], vp[0])."""
    q = [float(v) for v in obj[O["quat"]:O["quat"] + 4]]
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    x, y, z, w = q[0] / n, q[1] / n, q[2] / n, q[3] / n
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    r = [x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw),
         2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw),
         2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2]
    t = [float(v) for v in obj[O["loc"]:O["loc"] + 3]]
    o2c, c2o = [0.0] * 16, [0.0] * 16
    for i in range(3):
        for j in range(3):
            o2c[i * 4 + j] = r[i * 3 + j]
            c2o[i * 4 + j] = r[j * 3 + i]
        o2c[i * 4 + 3] = t[i]
        c2o[i * 4 + 3] = -(r[i] * t[0] + r[3 + i] * t[1] + r[6 + i] * t[2])
    o2c[15] = c2o[15] = 1.0
    a = 2 * math.pi / S * s
    cs, sn = math.cos(a), math.sin(a)
    ry = [cs, 0.0, sn, 0.0, 0.0, 1.0, 0.0, 0.0, -sn, 0.0, cs, 0.0, 0.0, 0.0, 0.0, 1.0]
    m = _mat4(_mat4(_mat4([float(v) for v in img[I["proj"]:I["proj"] + 16]], o2c), ry), c2o)
    width, height = float(img[I["width"]]), float(img[I["height"]])
    pts, raw = [], []
    for i in range(9):
        k = [float(v) for v in obj[O["kps3d"] + 3 * i:O["kps3d"] + 3 * i + 3]]
        p = [m[row * 4] * k[0] + m[row * 4 + 1] * k[1] + m[row * 4 + 2] * k[2] + m[row * 4 + 3] * 1.0 for row in range(4)]
        v0 = (p[0] / p[3] + 1.0) / 2.0 * height
        v1 = (p[1] / p[3] + 1.0) / 2.0 * width
        pts.append((_trunc(v1), _trunc(v0)))
        raw.append((v1, v0))
    return pts, raw


def gaussian_radius(height, width):
    mo = 0.7
    b1 = height + width
    c1 = width * height * (1 - mo) / (1 + mo)
    r1 = (b1 + math.sqrt(b1 * b1 - 4 * c1)) / 2
    b2 = 2 * (height + width)
    c2 = (1 - mo) * width * height
    r2 = (b2 + math.sqrt(b2 * b2 - 16 * c2)) / 2
    a3 = 4 * mo
    b3 = -2 * mo * (height + width)
    c3 = (mo - 1) * width * height
    r3 = (b3 + math.sqrt(b3 * b3 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


def object_targets(img, obj, s, S, R, center_3D, abs_scale):
    """One object in variant s: None (not kept) or a dict of what it writes and draws."""
    t = [float(v) for v in img[I["trans"]:I["trans"] + 6]]
    width, height = float(img[I["width"]]), float(img[I["height"]])
    flipped = img[I["flipped"]] != 0
    if int(obj[O["nsym"]]) != 1:
        pts9, _ = project(img, obj, s, S)
        p = [(float(a), float(b)) for a, b in pts9]
    else:
        c = obj[O["cuboid"]:O["cuboid"] + 18]
        p = [(float(c[2 * i]), float(c[2 * i + 1])) for i in range(9)]
    vis, pi = [], []
    for x, y in p[1:]:
        vis.append(1 if (x >= width or x < 0 or y < 0 or y >= height) else 2)
        pi.append([_trunc(x), _trunc(y)])
    if flipped:
        for q in pi:
            q[0] = int(width) - q[0] - 1
        for a, b in FLIP_SWAPS:
            pi[a], pi[b] = pi[b], pi[a]
            vis[a], vis[b] = vis[b], vis[a]
    xy = [affine(t, float(q[0]), float(q[1])) for q in pi]
    bb = [min(v[0] for v in xy), min(v[1] for v in xy), max(v[0] for v in xy), max(v[1] for v in xy)]
    bb = [min(max(v, 0.0), float(R - 1)) for v in bb]
    h, w = bb[3] - bb[1], bb[2] - bb[0]
    cx0, cy0 = p[0]
    visible = not ((cx0 >= width or cx0 < 0 or cy0 < 0 or cy0 >= height) and sum(vis) <= 12)
    if not (((h > 0 and w > 0) or img[I["rot"]] != 0) and visible):
        return None
    radius = max(0, int(gaussian_radius(float(math.ceil(h)), float(math.ceil(w)))))
    if not center_3D:
        ct = (np.float32((bb[0] + bb[2]) / 2), np.float32((bb[1] + bb[3]) / 2))
        ci = (int(ct[0]), int(ct[1]))
        ct = (float(ct[0]), float(ct[1]))
    else:
        ct = affine(t, width - cx0 - 1 if flipped else cx0, cy0)
        ci = (_trunc(ct[0]), _trunc(ct[1]))
        if ci[0] >= R or ci[1] >= R or ci[0] < 0 or ci[1] < 0:
            return None
    sc = obj[O["scale"]:O["scale"] + 3].astype(np.float64)
    r = {"radius": radius, "ct": ci, "ind": ci[1] * R + ci[0], "wh": (w, h), "reg": (ct[0] - ci[0], ct[1] - ci[1]),
         "scale": np.abs(sc) if abs_scale else np.abs(sc) / sc[1], "joints": []}
    for j in range(J):
        x, y = affine(t, float(pi[j][0]), float(pi[j][1]))
        jx, jy = _trunc(x), _trunc(y)
        if vis[j] > 1 and 0 <= jx < R and 0 <= jy < R:
            r["joints"].append((j, jx, jy))
    return r


def draw(heat, x, y, r):
    """draw_umich_gaussian's result: max with float32(exp(-(dx^2+dy^2) / (2 sigma^2))) over the clipped window."""
    d = 2 * r + 1
    sigma = d / 6
    o = np.arange(-r, r + 1)
    g = np.exp(-(o[None, :] * o[None, :] + o[:, None] * o[:, None]) / (2 * sigma * sigma)).astype(np.float32)
    H, W = heat.shape
    y0, y1, x0, x1 = max(0, y - r), min(H, y + r + 1), max(0, x - r), min(W, x + r + 1)
    np.maximum(heat[y0:y1, x0:x1], g[y0 - y + r:y1 - y + r, x0 - x + r:x1 - x + r], out=heat[y0:y1, x0:x1])


def image_targets(img, objs, S, R, center_3D=False, abs_scale=False, K=None):
    """Every target array of one image, [S, ...] (all keys; the caller picks what its options return)."""
    K = objs.shape[0] if K is None else K
    f32 = np.float32
    out = {"hm": np.zeros((S, 1, R, R), f32), "hm_hp": np.zeros((S, J, R, R), f32), "reg_mask": np.zeros((S, K), np.uint8),
           "ind": np.zeros((S, K), np.int64), "hps": np.zeros((S, K, 2 * J), f32),
           "hps_mask": np.zeros((S, K, 2 * J), np.uint8), "hps_uncertainty": np.zeros((S, K, 2 * J), f32),
           "wh": np.zeros((S, K, 2), f32), "reg": np.zeros((S, K, 2), f32), "scale": np.zeros((S, K, 3), f32),
           "scale_uncertainty": np.zeros((S, K, 3), f32), "hp_offset": np.zeros((S, K * J, 2), f32),
           "hp_ind": np.zeros((S, K * J), np.int64), "hp_mask": np.zeros((S, K * J), np.int64)}
    for k in range(int(img[I["num_objs"]])):
        for s in range(int(objs[k, O["nsym"]])):
            r = object_targets(img, objs[k], s, S, R, center_3D, abs_scale)
            if r is None:
                continue
            out["reg_mask"][s, k] = 1
            out["ind"][s, k] = r["ind"]
            out["wh"][s, k] = r["wh"]
            out["reg"][s, k] = r["reg"]
            out["scale"][s, k] = r["scale"]
            cx, cy = r["ct"]
            for j, jx, jy in r["joints"]:
                out["hps"][s, k, 2 * j:2 * j + 2] = (jx - cx, jy - cy)
                out["hps_mask"][s, k, 2 * j:2 * j + 2] = 1
                out["hps_uncertainty"][s, k, 2 * j:2 * j + 2] = r["radius"]
                out["hp_ind"][s, k * J + j] = jy * R + jx
                out["hp_mask"][s, k * J + j] = 1
                draw(out["hm_hp"][s, j], jx, jy, r["radius"])
            draw(out["hm"][s, 0], cx, cy, r["radius"])
    return out


def batch_targets(images, objects, S, R, center_3D=False, abs_scale=False):
    """image_targets for every image of collated records, stacked to [B, S, ...]."""
    per = [image_targets(images[b], objects[b], S, R, center_3D, abs_scale) for b in range(images.shape[0])]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}
