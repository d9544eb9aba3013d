"""Host restatement of the tracking task's training targets (cp_pose_targets_track,
centerpose_amd/pose_targets_track.py) in numpy: from the records of ``pack_track_annotations`` to the arrays of the
dataset's ``ret`` for one image or a batch.

It restates Step 1 of ObjectPoseDataset.__getitem__ in its noise-simulation mode (datasets/dataset_combined.py:555-937,
data_generation_mode == 0) and the three places where Step 2 reads it (:968-972, :983-987, :1106-1137), on top of
tests/pose_targets_ref.py, with the reference's rounding points: the centre a float32 array by box and float64 under
center_3D, astype(int32) truncation, floats assigned into the int64 pts_pre / pt2, pts_single_pre in float32 and
/ down_ratio, the heat np.maximum(1 - 2 ** (sqrt(nx ** 2 + ny ** 2) - 4.5), 0) with numpy's scalar ``**`` (libm's pow).
Every float64 sum is written out in the order the device evaluates it, so the host build of
pose_targets_track_common.h matches it bit for bit.
"""
import math
from types import SimpleNamespace

import numpy as np

from centerpose_amd import hip
from tests import pose_targets_ref as R

J = R.J
I, O = R.I, R.O
TI, P, D, C = hip.PTK_IMG, hip.PTK_PRE, hip.PTK_DRAW, hip.PTK_CUR
OPT_NAMES = ("input_w", "input_h", "down_ratio", "center_3D", "pre_hm", "pre_hm_hp", "hm_heat_random",
             "hm_hp_heat_random", "tracking_label_mode") + hip.PTK_DISTURB


def options(opt):
    """The options the previous-frame logic reads, from a dataset ``opt``."""
    return SimpleNamespace(**{n: getattr(opt, n) for n in OPT_NAMES})


def heat(nx, ny):
    """np.maximum(1 - 2 ** (np.sqrt(nx ** 2 + ny ** 2) - 4.5), 0) on numpy float64 scalars, as the reference calls it."""
    nx, ny = np.float64(nx), np.float64(ny)
    return float(np.maximum(1 - 2 ** (np.sqrt(nx ** 2 + ny ** 2) - 4.5), 0))


def pre_image(img, timg):
    """The current image's record with the previous frame's affine and projection matrix in it."""
    im = np.array(img, np.float64)
    im[I["trans"]:I["trans"] + 6] = timg[TI["trans"]:TI["trans"] + 6]
    im[I["proj"]:I["proj"] + 16] = timg[TI["proj"]:TI["proj"] + 16]
    return im


def _f32(v):
    return float(np.float32(v))


def pre_object(im, pre, S, op):
    """One previous object: a dict with kept / id / chosen (None or the variant) / cts (None or two float64) / pts
    (float32 [8, 2], NaN = None) / pmask [8] / radius / draws [(channel, x, y, k)] (k == 0 included), and for the case
    builders geom (w, h, ct0 once the box passed its tests) and gt {j: the joint's in-frame ground-truth point}."""
    res = {"kept": False, "id": int(pre[P["id"]]), "chosen": None, "cts": None, "pts": np.zeros((J, 2), np.float32),
           "pmask": np.zeros(J, np.uint8), "radius": 0, "draws": [], "geom": None, "gt": {}}
    if pre[P["skip"]] != 0:
        return res
    t = [float(v) for v in im[I["trans"]:I["trans"] + 6]]
    dw = [float(v) for v in pre[P["draws"]:P["draws"] + hip.PTK_NUM_DRAWS]]
    width, height = float(im[I["width"]]), float(im[I["height"]])
    flipped = im[I["flipped"]] != 0
    idsym = int(pre[P["idsym"]])
    if int(pre[O["nsym"]]) != 1:
        pts9, _ = R.project(im, pre, idsym, S)
        p = [(float(a), float(b)) for a, b in pts9]
    else:
        c = pre[O["cuboid"]:O["cuboid"] + 18]
        p = [(float(c[2 * i]), float(c[2 * i + 1])) for i in range(9)]
    vis, pi = [], []
    for x, y in p[1:]:
        vis.append(1 if (x >= width or x < 0 or y < 0 or y >= height) else 2)
        pi.append([R._trunc(x), R._trunc(y)])
    if flipped:
        for q in pi:
            q[0] = int(width) - q[0] - 1
        for a, b in R.FLIP_SWAPS:
            pi[a], pi[b] = pi[b], pi[a]
            vis[a], vis[b] = vis[b], vis[a]
    xy = [R.affine(t, float(q[0]), float(q[1])) for q in pi]
    hx, hy = float(op.input_w - 1), float(op.input_h - 1)
    bb = [min(max(min(v[0] for v in xy), 0.0), hx), min(max(min(v[1] for v in xy), 0.0), hy),
          min(max(max(v[0] for v in xy), 0.0), hx), min(max(max(v[1] for v in xy), 0.0), hy)]
    h, w = bb[3] - bb[1], bb[2] - bb[0]
    cx0, cy0 = p[0]
    visible = not ((cx0 >= width or cx0 < 0 or cy0 < 0 or cy0 >= height) and sum(vis) <= 12)
    if not (((h > 0 and w > 0) or im[I["rot"]] != 0) and visible):
        return res
    radius = max(0, int(R.gaussian_radius(float(math.ceil(h)), float(math.ceil(w)))))
    res["radius"] = radius
    nx, ny = dw[D["ct_noise"]], dw[D["ct_noise"] + 1]
    if not op.center_3D:
        ct0 = (_f32((bb[0] + bb[2]) / 2), _f32((bb[1] + bb[3]) / 2))
        ct = (_f32(ct0[0] + nx * op.hm_disturb * w), _f32(ct0[1] + ny * op.hm_disturb * h))
    else:
        ct0 = R.affine(t, width - cx0 - 1 if flipped else cx0, cy0)
        ct = (ct0[0] + nx * op.hm_disturb * w, ct0[1] + ny * op.hm_disturb * h)
    res["geom"] = (w, h, ct0)
    cix, ciy = R._trunc(ct[0]), R._trunc(ct[1])
    if cix >= op.input_w or ciy >= op.input_h or cix < 0 or ciy < 0:
        return res
    conf = 0.0
    if dw[D["ct_lost"]] > op.lost_disturb:
        conf = dw[D["ct_heat"]] if op.hm_heat_random else 1.0
    dr = float(op.down_ratio)
    if not (conf == 0 and op.tracking_label_mode != 0):
        lab = ct if (conf == 0 or op.tracking_label_mode != 0) else ct0
        res["cts"] = tuple(v / dr if op.center_3D else _f32(v / dr) for v in lab)
    res["kept"] = True
    for j in range(J):
        dj = dw[D["joints"] + D["joint_stride"] * j:D["joints"] + D["joint_stride"] * (j + 1)]
        x, y = R.affine(t, float(pi[j][0]), float(pi[j][1]))
        jx, jy = R._trunc(x), R._trunc(y)
        if not (vis[j] > 1 and 0 <= jx < op.input_w and 0 <= jy < op.input_h):
            continue
        res["gt"][j] = (jx, jy)
        jnx, jny = dj[D["j_noise"]], dj[D["j_noise"] + 1]
        qx = R._trunc(float(jx) + jnx * op.hm_hp_disturb * w)
        qy = R._trunc(float(jy) + jny * op.hm_hp_disturb * h)
        conf_hp = 0.0
        if dj[D["j_lost"]] > op.hp_lost_disturb:
            conf_hp = heat(jnx, jny) if op.hm_hp_heat_random else 1.0
        if conf_hp == 0:
            mode = 1 if op.tracking_label_mode == 0 else 2
        else:
            mode = 0 if op.tracking_label_mode == 0 else (1 if conf != 0 else 2)
        if mode == 2:
            res["pts"][j] = np.nan
        else:
            lx, ly = (jx, jy) if mode == 0 else (qx, qy)
            res["pts"][j] = (np.float32(_f32(lx) / dr), np.float32(_f32(ly) / dr))
            res["pmask"][j] = 1
        if op.pre_hm_hp and conf != 0:
            res["draws"].append((1 + j, qx, qy, conf_hp))
            if dj[D["j_fp"]] < op.hp_fp_disturb:
                res["draws"].append((1 + j, R._trunc(float(jx) + dj[D["j_fp_noise"]] * 0.05 * w),
                                     R._trunc(float(jy) + dj[D["j_fp_noise"] + 1] * 0.05 * h), dj[D["j_fp_peak"]]))
    if op.pre_hm:
        if conf != 0 and op.hm_heat_random:
            conf = heat(nx, ny)
        res["draws"].append((0, cix, ciy, conf))
        if conf != 0:
            res["chosen"] = idsym
        if dw[D["ct_fp"]] < op.fp_disturb:
            c2 = (ct0[0] + dw[D["ct_fp_noise"]] * 0.05 * w, ct0[1] + dw[D["ct_fp_noise"] + 1] * 0.05 * h)
            if not op.center_3D:
                c2 = (_f32(c2[0]), _f32(c2[1]))
            res["draws"].append((0, R._trunc(c2[0]), R._trunc(c2[1]), dw[D["ct_fp_peak"]]))
    return res


def draw(heat_map, x, y, r, k):
    """draw_umich_gaussian with a peak: max with float32(k * exp(-(dx^2+dy^2) / (2 sigma^2))), the product in float64,
    over the window clipped to the map; nothing when the clipped window is empty (utils/image.py:135-150)."""
    H, W = heat_map.shape
    y0, y1, x0, x1 = max(0, y - r), min(H, y + r + 1), max(0, x - r), min(W, x + r + 1)
    if y1 <= y0 or x1 <= x0:
        return
    sigma = (2 * r + 1) / 6
    ox, oy = np.arange(x0, x1) - x, np.arange(y0, y1) - y
    g = np.exp(-(ox[None, :] * ox[None, :] + oy[:, None] * oy[:, None]) / (2 * sigma * sigma))
    np.maximum(heat_map[y0:y1, x0:x1], (g * k).astype(np.float32), out=heat_map[y0:y1, x0:x1])


def image_targets(recs, S, Rr, op, abs_scale=False):
    """Every target array of one image: the current frame's [S, ...] of pose_targets_ref.image_targets with the
    tracking task's skip and variant filter applied, pre_hm / pre_hm_hp [C, input_h, input_w], tracking(_mask),
    tracking_hp(_mask), and 'pre' (the per-object dicts, for the tests)."""
    img, objs = recs["pt_image"], recs["pt_objects"]
    timg, pobj, cobj = recs["ptk_image"], recs["ptk_pre_objects"], recs["ptk_cur_objects"]
    K = objs.shape[0]
    f32 = np.float32
    im = pre_image(img, timg)
    npre = int(timg[TI["num_pre"]])
    pre = [pre_object(im, pobj[k], S, op) for k in range(npre)]
    out = {"pre": pre, "pre_hm": np.zeros((1, op.input_h, op.input_w), f32),
           "pre_hm_hp": np.zeros((J, op.input_h, op.input_w), f32), "tracking": np.zeros((S, K, 2), f32),
           "tracking_mask": np.zeros((S, K), np.uint8), "tracking_hp": np.zeros((S, K, 2 * J), f32),
           "tracking_hp_mask": np.zeros((S, K, 2 * J), np.uint8)}
    for r in pre:
        for c, x, y, k in r["draws"]:
            draw(out["pre_hm"][0] if c == 0 else out["pre_hm_hp"][c - 1], x, y, r["radius"], k)
    # the current frame: an object / variant that the skip or the filter drops is an object with no variant there
    cur = {"hm": np.zeros((S, 1, Rr, Rr), f32), "hm_hp": np.zeros((S, J, Rr, Rr), f32),
           "reg_mask": np.zeros((S, K), np.uint8), "ind": np.zeros((S, K), np.int64), "hps": np.zeros((S, K, 2 * J), f32),
           "hps_mask": np.zeros((S, K, 2 * J), np.uint8), "hps_uncertainty": np.zeros((S, K, 2 * J), f32),
           "wh": np.zeros((S, K, 2), f32), "reg": np.zeros((S, K, 2), f32), "scale": np.zeros((S, K, 3), f32),
           "scale_uncertainty": np.zeros((S, K, 3), f32), "hp_offset": np.zeros((S, K * J, 2), f32),
           "hp_ind": np.zeros((S, K * J), np.int64), "hp_mask": np.zeros((S, K * J), np.int64)}
    for k in range(int(img[I["num_objs"]])):
        if cobj[k, C["skip"]] != 0:
            continue
        nsym = int(objs[k, O["nsym"]])
        for s in range(nsym):
            if op.pre_hm_hp and nsym != 1 and k < npre and pre[k]["chosen"] is not None and pre[k]["chosen"] != s:
                continue
            r = R.object_targets(img, objs[k], s, S, Rr, op.center_3D, abs_scale)
            if r is None:
                continue
            cur["reg_mask"][s, k] = 1
            cur["ind"][s, k] = r["ind"]
            cur["wh"][s, k] = r["wh"]
            cur["reg"][s, k] = r["reg"]
            cur["scale"][s, k] = r["scale"]
            cx, cy = r["ct"]
            m = next((q for q in pre if q["kept"] and q["id"] == int(cobj[k, C["id"]])), None)
            for j, jx, jy in r["joints"]:
                cur["hps"][s, k, 2 * j:2 * j + 2] = (jx - cx, jy - cy)
                cur["hps_mask"][s, k, 2 * j:2 * j + 2] = 1
                cur["hps_uncertainty"][s, k, 2 * j:2 * j + 2] = r["radius"]
                cur["hp_ind"][s, k * J + j] = jy * Rr + jx
                cur["hp_mask"][s, k * J + j] = 1
                R.draw(cur["hm_hp"][s, j], jx, jy, r["radius"])
                if m is not None and not np.isnan(m["pts"][j]).any():
                    out["tracking_hp"][s, k, 2 * j:2 * j + 2] = (float(m["pts"][j, 0]) - jx, float(m["pts"][j, 1]) - jy)
                    out["tracking_hp_mask"][s, k, 2 * j:2 * j + 2] = m["pmask"][j] & 1
            R.draw(cur["hm"][s, 0], cx, cy, r["radius"])
            if m is not None and m["cts"] is not None:
                out["tracking"][s, k] = (m["cts"][0] - cx, m["cts"][1] - cy)
                out["tracking_mask"][s, k] = 1
    out.update(cur)
    return out


def batch_targets(recs, S, Rr, op, abs_scale=False):
    """image_targets for every image of collated records, stacked to [B, ...] ('pre': a list of lists)."""
    B = recs["pt_image"].shape[0]
    per = [image_targets({k: np.asarray(v)[b] for k, v in recs.items()}, S, Rr, op, abs_scale) for b in range(B)]
    return {k: ([p[k] for p in per] if k == "pre" else np.stack([p[k] for p in per])) for k in per[0]}
