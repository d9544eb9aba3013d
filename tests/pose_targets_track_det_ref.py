"""Host restatement of the tracking task's training targets with the detector in the loop (cp_pose_targets_track_det,
centerpose_amd/pose_targets_track.py with a detector) in numpy: ObjectPoseDataset.__getitem__ in data_generation_mode 1
(datasets/dataset_combined.py:464-550, :644-693, :752-763, :792-794, :851-867, :890-911, :939-952), given the detector's
answer as the list ``boxes`` of the reference's tuples (kps_pnp [9, 2], kps_3d_cam, obj_scale, kps_ori [9, 2], the
detection dict with 'ct', 'kps_heatmap_std', 'kps_heatmap_height', 'score'), which is what BaseDetector.run and
ObjectPoseDetector.run_batch return under 'boxes'.

Mode-0 images and the whole current frame are tests/pose_targets_track_ref.py's; only the previous-frame objects of a
mode-1 image are restated here, on the records of pack_track_annotations.  ``boxes_from_records`` turns device-layout
rows (cp_postprocess, cp_pnp_from_post) into that list the way run_batch does, so tests can start from either end.
"""
import math
from types import SimpleNamespace

import numpy as np

from centerpose_amd import hip
from tests import pose_targets_ref as R
from tests import pose_targets_track_ref as TR

J = R.J
I, O = R.I, R.O
TI, P, D = hip.PTK_IMG, hip.PTK_PRE, hip.PTK_DRAW
FLIP_IDX = [[1, 5], [3, 7], [2, 6], [4, 8]]  # opt.flip_idx


def det_options(opt):
    return SimpleNamespace(render_hm_mode=int(opt.render_hm_mode), render_hmhp_mode=int(opt.render_hmhp_mode), c=opt.c)


def boxes_from_records(post, count, pnp, width, height, category, return_slots=False):
    """run_batch's 'boxes' of one image from its device-layout rows: post [K, 120], pnp [K, 40] (float64); with
    ``return_slots`` also the slot each box came from."""
    from centerpose_amd.lib.utils.pnp.cuboid_pnp_shell import finish_detection

    f32_fields = ("obj_scale", "obj_scale_uncertainty", "kps_displacement_std", "tracking", "tracking_hp",
                  "kps_heatmap_std", "kps_heatmap_height")
    opt, meta = SimpleNamespace(c=category), {"width": width, "height": height}
    boxes, slots = [], []
    for k in range(int(count)):
        r, item = post[k], {}
        for name, (off, w) in hip.POST_FIELDS.items():
            v = r[off:off + w]
            if name == "score":
                item[name] = float(v[0])
            elif name == "cls":
                item[name] = int(v[0])
            elif name == "ct":
                item[name] = [v[0], v[1]]
            else:
                item[name] = v.astype(np.float32) if name in f32_fields else v.copy()
        if int(pnp[k, 0]) != 1:
            continue
        ret = finish_detection(opt, meta, item, item["obj_scale"], list(pnp[k, 28:31]), pnp[k, 31:35].copy(),
                               pnp[k, 8:24].reshape(8, 2).copy())
        if ret is not None:
            boxes.append(ret)
            slots.append(k)
    return (boxes, slots) if return_slots else boxes


def instances_2d(img, pobj, npre):
    """:506-532 on the packed previous objects (the raw projected_cuboid, whatever the variant)."""
    width, height, flipped = int(img[I["width"]]), int(img[I["height"]]), img[I["flipped"]] != 0
    out = []
    for k in range(npre):
        c = np.array(pobj[k, O["cuboid"]:O["cuboid"] + 18]).reshape((9, 2)).astype("float32")
        if flipped:
            c[:, 0] = width - c[:, 0] - 1
            for e in FLIP_IDX:  # on the nine rows: the centre trades places with row 4
                a, b = e[0] - 1, e[1] - 1
                c[a], c[b] = c[b].copy(), c[a].copy()
        c[:, 0] = c[:, 0] / width
        c[:, 1] = c[:, 1] / height
        if c[0][0] > 0 and c[0][0] < 1 and c[0][1] > 0 and c[0][1] < 1:
            out.append(c)
        else:
            out.append(np.ones((9, 2)) * -10000)
    return np.array(out).reshape((-1, 9, 2))


def norms(inst, boxes):
    """norms_list [len(boxes), npre] (:542)."""
    return np.array([np.linalg.norm(inst[:, 1:, :] - b[0][1:, :], axis=(1, 2)) for b in boxes]).reshape(len(boxes), len(inst))


def match(inst, boxes):
    """Per previous object the index of its box in ``boxes`` or None (:537-550, :645-661), and norms_list."""
    nl = norms(inst, boxes)
    md = np.array([int(np.argmin(n)) for n in nl], dtype=np.int64)
    sel = []
    for o in range(len(inst)):
        idx = np.where(md == o)[0]
        if len(idx) == 0:
            sel.append(None)
        elif len(idx) == 1:
            sel.append(int(idx[0]))
        else:
            i = int(idx[np.argmin(nl[idx, o])])
            sel.append(None if np.min(nl[i, o]) > 1000 else i)
    return sel, nl


def _f32(v):
    return float(np.float32(v))


def _geometry(im, pre, S, op):
    """The part of pose_targets_track_ref.pre_object both modes share (:575-720): None for a dropped object."""
    if pre[P["skip"]] != 0:
        return None
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
        return None
    radius = max(0, int(R.gaussian_radius(float(math.ceil(h)), float(math.ceil(w)))))
    nx, ny = dw[D["ct_noise"]], dw[D["ct_noise"] + 1]
    if not op.center_3D:
        ct0 = (_f32((bb[0] + bb[2]) / 2), _f32((bb[1] + bb[3]) / 2))
        ct = (_f32(ct0[0] + nx * op.hm_disturb * w), _f32(ct0[1] + ny * op.hm_disturb * h))
    else:
        ct0 = R.affine(t, width - cx0 - 1 if flipped else cx0, cy0)
        ct = (ct0[0] + nx * op.hm_disturb * w, ct0[1] + ny * op.hm_disturb * h)
    return SimpleNamespace(t=t, dw=dw, width=width, height=height, idsym=idsym, vis=vis, pi=pi, w=w, h=h, radius=radius,
                           ct0=ct0, ct=ct)


def _int32(v):
    return int(v) if -2147483649.0 < v < 2147483648.0 else -2 ** 31


def pre_object_det(im, pre, box, last_score, radius_scale, S, op, dop):
    """One previous object of a mode-1 image; ``box``: its matched tuple or None.  The dict of
    pose_targets_track_ref.pre_object, plus 'event' flags for the tests."""
    res = {"kept": False, "id": int(pre[P["id"]]), "chosen": None, "cts": None, "pts": np.zeros((J, 2), np.float32),
           "pmask": np.zeros(J, np.uint8), "radius": 0, "draws": [], "geom": None, "gt": {},
           "event": {"outside": 0, "radius0": 0, "drawn": 0}}
    g = _geometry(im, pre, S, op)
    if g is None:
        return res
    res["radius"], res["geom"] = g.radius, (g.w, g.h, g.ct0)
    dr = float(op.down_ratio)
    ctd = None
    if box is not None:
        ctd = R.affine(g.t, float(box[4]["ct"][0]), float(box[4]["ct"][1]))
        src = box[3] if dop.render_hmhp_mode in (0, 1) else box[0]
        pts = [(float(src[1 + j][0]) * g.width, float(src[1 + j][1]) * g.height) for j in range(J)]
        pts = [R.affine(g.t, x, y) for x, y in pts]
        std = [float(np.float32(v)) for v in np.asarray(box[4]["kps_heatmap_std"]).reshape(-1)]
        height = [float(np.float32(v)) for v in np.asarray(box[4]["kps_heatmap_height"]).reshape(-1)]
    if box is None:
        if op.tracking_label_mode == 0:
            res["cts"] = tuple(v / dr if op.center_3D else _f32(v / dr) for v in g.ct)
    elif op.tracking_label_mode == 0:
        res["cts"] = tuple(v / dr if op.center_3D else _f32(v / dr) for v in g.ct0)
    else:
        res["cts"] = (ctd[0] / dr, ctd[1] / dr)
    res["kept"] = True
    for j in range(J):
        dj = g.dw[D["joints"] + D["joint_stride"] * j:D["joints"] + D["joint_stride"] * (j + 1)]
        x, y = R.affine(g.t, float(g.pi[j][0]), float(g.pi[j][1]))
        jx, jy = R._trunc(x), R._trunc(y)
        if not (g.vis[j] > 1 and 0 <= jx < op.input_w and 0 <= jy < op.input_h):
            continue
        res["gt"][j] = (jx, jy)
        qx = R._trunc(float(jx) + dj[D["j_noise"]] * op.hm_hp_disturb * g.w)
        qy = R._trunc(float(jy) + dj[D["j_noise"] + 1] * op.hm_hp_disturb * g.h)
        if box is None and op.tracking_label_mode != 0:
            res["pts"][j] = np.nan
        else:
            if box is None:
                lx, ly = _f32(qx), _f32(qy)
            elif op.tracking_label_mode == 0:
                lx, ly = _f32(jx), _f32(jy)
            else:
                lx, ly = _f32(pts[j][0]), _f32(pts[j][1])
            res["pts"][j] = (np.float32(lx / dr), np.float32(ly / dr))
            res["pmask"][j] = 1
        if op.pre_hm_hp and box is not None:
            px, py = pts[j]
            if not (px >= 0 and px < op.input_w and py >= 0 and py < op.input_h):
                res["event"]["outside"] += 1
                continue
            if dop.render_hmhp_mode in (1, 3):
                res["draws"].append((1 + j, int(px), int(py), 1.0))
                res["event"]["drawn"] += 1
            elif _int32(std[2 * j] * radius_scale) > 0:
                res["draws"].append((1 + j, int(px), int(py), height[j]))
                res["event"]["drawn"] += 1
            else:
                res["event"]["radius0"] += 1
    if op.pre_hm and box is not None:
        k = 1.0 if dop.render_hm_mode == 0 else float(last_score)
        res["draws"].append((0, max(-10 ** 9, min(10 ** 9, R._trunc(ctd[0]))), max(-10 ** 9, min(10 ** 9, R._trunc(ctd[1]))), k))
        if dop.render_hm_mode == 0 or k != 0:
            res["chosen"] = g.idsym
    return res


def image_targets(recs, boxes, S, Rr, op, dop, abs_scale=False):
    """Every target array of one image (pose_targets_track_ref.image_targets' dict).  ``recs`` holds 'ptk_gen'; a mode-0
    image is the existing restatement, untouched.  ``boxes``: the detector's list for this image (fresh: nothing here
    writes into it).  Adds 'match' (per previous object the box index or None) and 'norms' for a mode-1 image."""
    gen = recs["ptk_gen"]
    base = {k: v for k, v in recs.items() if k not in ("ptk_gen", "ptk_det_meta")}
    if gen[hip.PTK_GEN["mode"]] == 0:
        return TR.image_targets(base, S, Rr, op, abs_scale)
    img, timg, pobj = recs["pt_image"], recs["ptk_image"], recs["ptk_pre_objects"]
    npre = int(timg[TI["num_pre"]])
    im = TR.pre_image(img, timg)
    sel, nl = match(instances_2d(img, pobj, npre), boxes) if boxes and npre else ([None] * npre, np.zeros((len(boxes), npre)))
    last_score = boxes[-1][4]["score"] if boxes else 0.0  # :949-951 read the matching loop's last `result_ori`
    pre = [pre_object_det(im, pobj[k], None if sel[k] is None else boxes[sel[k]], last_score,
                          float(gen[hip.PTK_GEN["radius_scale"]]), S, op, dop) for k in range(npre)]
    # the rest -- drawing the lists, the current frame and its reads of the previous objects -- is the existing
    # restatement's, fed these objects in place of its own
    it, keep = iter(pre), TR.pre_object
    TR.pre_object = lambda *a: next(it)
    try:
        out = TR.image_targets(base, S, Rr, op, abs_scale)
    finally:
        TR.pre_object = keep
    out["match"], out["norms"] = sel, nl
    return out


def batch_targets(recs, boxes, S, Rr, op, dop, abs_scale=False):
    """image_targets for every image of collated records; ``boxes``: one list per image."""
    B = recs["pt_image"].shape[0]
    per = [image_targets({k: np.asarray(v)[b] for k, v in recs.items()}, boxes[b], S, Rr, op, dop, abs_scale)
           for b in range(B)]
    keys = [k for k in per[0] if k not in ("pre", "match", "norms")]
    out = {k: np.stack([p[k] for p in per]) for k in keys}
    out["pre"] = [p["pre"] for p in per]
    out["match"] = [p.get("match") for p in per]
    out["norms"] = [p.get("norms") for p in per]
    return out
