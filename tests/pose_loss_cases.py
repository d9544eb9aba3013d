"""Seeded ObjectPoseLoss cases shared by tools/make_pose_loss_goldens.py and the tests: dataset-shaped ground truth
(Gaussian splats with exact-1.0 peaks at the `ind` positions, masks with holes, masked entries pointing at index 0) and
head outputs, regenerated from numpy seeds so that the golden file only stores results."""
import os
import sys
import types
from types import SimpleNamespace

import numpy as np

REF = os.environ.get("CENTERPOSE_REFERENCE", "/root/reference")

BASE_OPT = dict(mse_loss=False, dense_hp=False, reg_loss="l1", num_stacks=1, hm_hp=True, hps_uncertainty=False,
                reg_bbox=True, wh_weight=0.1, obj_scale=True, obj_scale_weight=1.0, obj_scale_uncertainty=False,
                use_residual=False, dimension_ref=[1.0, 1.0, 1.0], reg_offset=True, off_weight=1.0, reg_hp_offset=True,
                hm_hp_weight=1.0, tracking=False, tracking_weight=1.0, tracking_hp=False, tracking_hp_weight=1.0,
                hm_weight=1.0, hp_weight=1.0, KL_kps_uncertainty=0.1, KL_scale_uncertainty=0.1, eval_oracle_hm=False,
                eval_oracle_hmhp=False, eval_oracle_kps=False, eval_oracle_hp_offset=False, gpus=[-1])

# name -> (seed, B, S, res, J, opt overrides, phase, specials)
CASES = {
    "s1": (1, 2, 1, 32, 8, {}, "train", ()),
    "s4": (2, 3, 4, 32, 8, {}, "train", ("dup", "sat")),
    "s12": (3, 2, 12, 32, 8, {}, "train", ("tie", "nopos")),
    "unc_train": (4, 2, 4, 48, 8, dict(hps_uncertainty=True, obj_scale_uncertainty=True), "train", ("sat",)),
    "unc_val": (5, 2, 4, 48, 8, dict(hps_uncertainty=True, obj_scale_uncertainty=True), "val", ()),
    "residual": (6, 2, 4, 32, 8, dict(use_residual=True, dimension_ref=[0.9, 1.3, 0.7]), "train", ("dup",)),
    "tracking": (7, 2, 4, 32, 8, dict(tracking=True, tracking_hp=True), "train", ()),
    "stacks2": (8, 2, 4, 32, 8, dict(num_stacks=2), "train", ("invalid", "sat")),
    "invalid": (9, 3, 12, 32, 8, {}, "train", ("invalid", "nopos", "dup")),
}
HEAD_CH = {"hm": 1, "hm_hp": None, "hps": None, "hps_uncertainty": None, "wh": 2, "reg": 2, "scale": 3,
           "scale_uncertainty": 3, "hp_offset": 2, "tracking": 2, "tracking_hp": None}


def make_opt(over):
    o = dict(BASE_OPT)
    o.update(over)
    return SimpleNamespace(**o)


def head_names(opt):
    h = ["hm", "hps", "wh", "reg", "scale", "hm_hp", "hp_offset"]
    if opt.hps_uncertainty:
        h.append("hps_uncertainty")
    if opt.obj_scale_uncertainty:
        h.append("scale_uncertainty")
    if opt.tracking:
        h.append("tracking")
    if opt.tracking_hp:
        h.append("tracking_hp")
    return h


def splat(heat, cx, cy, radius, peak=1.0):
    """Adds a Gaussian of the given radius at (cx, cy) by element-wise max; its centre value is exactly `peak`."""
    sigma = (2 * radius + 1) / 6.0
    H, W = heat.shape
    ys, xs = np.arange(-radius, radius + 1), np.arange(-radius, radius + 1)
    g = np.exp(-(xs[None, :] ** 2 + ys[:, None] ** 2) / (2 * sigma * sigma))
    g[g < np.finfo(g.dtype).eps * g.max()] = 0
    g = (g * peak).astype(np.float32)
    g[radius, radius] = np.float32(peak)
    y0, y1, x0, x1 = max(0, cy - radius), min(H, cy + radius + 1), max(0, cx - radius), min(W, cx + radius + 1)
    sub = g[y0 - cy + radius:y1 - cy + radius, x0 - cx + radius:x1 - cx + radius]
    np.maximum(heat[y0:y1, x0:x1], sub, out=heat[y0:y1, x0:x1])


def make_batch(rng, B, S, res, J, K=10, specials=()):
    C = 1
    f32 = np.float32
    hm = np.zeros((B, S, C, res, res), f32)
    hm_hp = np.zeros((B, S, J, res, res), f32)
    ind = np.zeros((B, S, K), np.int64)
    reg_mask = np.zeros((B, S, K), np.uint8)
    hps = np.zeros((B, S, K, 2 * J), f32)
    hps_mask = np.zeros((B, S, K, 2 * J), np.uint8)
    hp_ind = np.zeros((B, S, K * J), np.int64)
    hp_mask = np.zeros((B, S, K * J), np.int64)
    hp_offset = np.zeros((B, S, K * J, 2), f32)
    tracking_mask = np.zeros((B, S, K), np.uint8)
    tracking_hp_mask = np.zeros((B, S, K, 2 * J), np.uint8)
    wh = np.zeros((B, S, K, 2), f32)
    reg = np.zeros((B, S, K, 2), f32)
    scale = np.zeros((B, S, K, 3), f32)
    tracking = np.zeros((B, S, K, 2), f32)
    tracking_hp = np.zeros((B, S, K, 2 * J), f32)
    for b in range(B):
        nobj = int(rng.integers(2, 5))
        centres = [(int(rng.integers(3, res - 3)), int(rng.integers(3, res - 3))) for _ in range(nobj)]
        if "dup" in specials and b == 0:
            centres[1] = centres[0]  # two objects share a centre: repeated index
        for s in range(S):
            if "invalid" in specials and b == B - 1:
                continue  # every variant of the last image is invalid: ind all zero
            for k, (cx, cy) in enumerate(centres):
                if k == 1 and nobj > 2 and s % 2 == 1:
                    continue  # a hole: masked entry, index 0
                peak = 0.9 if ("nopos" in specials and b == 0 and s == S - 1) else 1.0
                splat(hm[b, s, 0], cx, cy, int(rng.integers(1, 4)), peak)
                ind[b, s, k] = cy * res + cx
                reg_mask[b, s, k] = 1
                tracking_mask[b, s, k] = rng.random() < 0.8
                wh[b, s, k] = rng.uniform(2, 12, 2)
                reg[b, s, k] = rng.uniform(0, 1, 2)
                sc = rng.uniform(0.2, 1.5, 3)
                if rng.random() < 0.3:
                    sc[int(rng.integers(0, 3))] = 0.0  # the relative loss' zero-target branch
                scale[b, s, k] = sc
                tracking[b, s, k] = rng.normal(0, 2, 2)
                for j in range(J):
                    ang = 2 * np.pi * (j + s / max(S, 1)) / J
                    px = int(np.clip(cx + round(4 * np.cos(ang)) + int(rng.integers(-1, 2)), 0, res - 1))
                    py = int(np.clip(cy + round(4 * np.sin(ang)) + int(rng.integers(-1, 2)), 0, res - 1))
                    vis = rng.random() < 0.85
                    hps[b, s, k, 2 * j:2 * j + 2] = (px - cx, py - cy) + rng.normal(0, 0.3, 2)
                    hps_mask[b, s, k, 2 * j:2 * j + 2] = 1 if vis else 0
                    tracking_hp[b, s, k, 2 * j:2 * j + 2] = rng.normal(0, 1, 2)
                    tracking_hp_mask[b, s, k, 2 * j:2 * j + 2] = 1 if (vis and rng.random() < 0.7) else 0
                    if vis:
                        splat(hm_hp[b, s, j], px, py, 1)
                        hp_ind[b, s, k * J + j] = py * res + px
                        hp_mask[b, s, k * J + j] = 1
                        hp_offset[b, s, k * J + j] = rng.uniform(0, 1, 2)
        if "tie" in specials and b == 0 and S > 1:
            for a in (hm, hm_hp, ind, reg_mask, hps, hps_mask, hp_ind, hp_mask, hp_offset, tracking_mask,
                      tracking_hp_mask, wh, reg, scale, tracking, tracking_hp):
                a[b, 1] = a[b, 0]  # two byte-identical variants
    return dict(hm=hm, hm_hp=hm_hp, ind=ind, reg_mask=reg_mask, hps=hps, hps_mask=hps_mask, hp_ind=hp_ind,
                hp_mask=hp_mask, hp_offset=hp_offset, wh=wh, reg=reg, scale=scale, tracking=tracking,
                tracking_mask=tracking_mask, tracking_hp=tracking_hp, tracking_hp_mask=tracking_hp_mask)


def make_outputs(rng, opt, B, res, J, specials=()):
    outs = []
    for _ in range(opt.num_stacks):
        o = {}
        for h in head_names(opt):
            ch = HEAD_CH[h] or (J if h == "hm_hp" else 2 * J)
            if h in ("hm", "hm_hp"):
                v = rng.normal(-2.5, 1.5, (B, ch, res, res)).astype(np.float32)
                if "sat" in specials:  # the clamp is active
                    v.reshape(-1)[rng.integers(0, v.size, v.size // 20)] = 20.0
                    v.reshape(-1)[rng.integers(0, v.size, v.size // 20)] = -20.0
            elif h in ("hps_uncertainty", "scale_uncertainty"):
                v = rng.normal(0, 0.5, (B, ch, res, res)).astype(np.float32)
            elif h == "scale":
                v = rng.uniform(0.1, 1.5, (B, ch, res, res)).astype(np.float32)
                if opt.use_residual:
                    v = rng.normal(0, 0.3, (B, ch, res, res)).astype(np.float32)
            else:
                v = rng.normal(0, 3, (B, ch, res, res)).astype(np.float32)
            o[h] = v
        outs.append(o)
    return outs


def case(name):
    """-> (opt, phase, outputs [per-stack dict of float32 arrays], batch dict of arrays).  The seed of a case is bumped
    until every image's best and second-best variants differ by at least 1e-3 relative (bar the exact-tie case)."""
    import torch

    from tests import pose_loss_ref as R

    seed, B, S, res, J, over, phase, specials = CASES[name]
    opt = make_opt(over)
    for attempt in range(100):
        rng = np.random.default_rng(seed * 1000 + attempt)
        batch = make_batch(rng, B, S, res, J, specials=specials)
        outputs = make_outputs(rng, opt, B, res, J, specials)
        r = R.object_pose_loss(opt, [{k: torch.from_numpy(v).double() for k, v in o.items()} for o in outputs],
                               {k: torch.from_numpy(v) if v.dtype != np.float32 else torch.from_numpy(v).double()
                                for k, v in batch.items()}, phase)
        if S == 1 or _margins_ok(r["total"].numpy(), batch["ind"], specials):
            return opt, phase, outputs, batch
    raise RuntimeError("no seed with a clear choice for %s" % name)


def _margins_ok(total, ind, specials):
    for b in range(total.shape[0]):
        valid = ind[b].sum(axis=1) > 0
        v = np.sort(total[b][valid])
        if "tie" in specials and b == 0:
            v = np.sort(np.delete(total[b], 1)[valid[np.arange(len(valid)) != 1]])
        if len(v) > 1 and not (v[1] - v[0] >= 1e-3 * max(abs(v[0]), 1e-30)):
            return False
    return True


def import_reference_loss():
    """The reference's own ObjectPoseLoss class (lib/trains/object_pose.py, unmodified), with the modules it imports but
    does not use in the loss stubbed; None where the reference tree is absent.  The stubs, the reference's modules and
    its path entry are removed again afterwards, so that nothing else in the process sees them."""
    src = os.path.join(REF, "src")
    if not os.path.isfile(os.path.join(src, "lib", "trains", "object_pose.py")):
        return None
    before, path = set(sys.modules), list(sys.path)
    try:
        for name in ("cv2", "numba", "progress", "progress.bar", "lib.utils.debugger", "lib.utils.oracle_utils"):
            sys.modules[name] = types.ModuleType(name)
        sys.modules["progress.bar"].Bar = object
        sys.modules["lib.utils.debugger"].Debugger = object
        sys.modules["lib.utils.oracle_utils"].gen_oracle_map = None
        sys.path.insert(0, src)
        from lib.trains.object_pose import ObjectPoseLoss  # noqa: E402
    finally:
        for name in set(sys.modules) - before:
            del sys.modules[name]
        sys.path[:] = path
    return ObjectPoseLoss
