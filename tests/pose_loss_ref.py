"""A dtype-generic torch restatement of the reference's ObjectPoseLoss (trains/object_pose.py:42-205 with
models/losses.py and models/utils.py:_transpose_and_gather_feat), used in float64 as the yardstick of the device loss.

It does not modify its inputs: the heat-map logits go through torch.sigmoid and the clamp, and the clamped maps are
returned.  The clamp bounds are the float32 values the reference's float32 tensors use."""
import numpy as np
import torch

TERMS = ("hm", "wh", "off", "hp", "hm_hp", "hp_offset", "obj_scale", "tracking", "tracking_hp")
STATS = ("loss", "hm_loss", "hp_loss", "hm_hp_loss", "hp_offset_loss", "wh_loss", "off_loss", "obj_scale_loss",
         "tracking_loss", "tracking_hp_loss")
LO, HI = float(np.float32(1e-4)), float(np.float32(1 - 1e-4))


def clamp_sigmoid(x):
    return torch.clamp(torch.sigmoid(x), LO, HI)


def gather(head, ind):
    """head [B,C,H,W], ind [B,S,N] -> [B,S,N,C]: the value of every channel at each flattened index."""
    B, C = head.shape[:2]
    S, N = ind.shape[1:]
    idx = ind.reshape(B, 1, S * N).expand(B, C, S * N)
    return head.reshape(B, C, -1).gather(2, idx).reshape(B, C, S, N).permute(0, 2, 3, 1)


def focal(p, gt):
    """p [B,C,H,W] (clamped), gt [B,S,C,H,W] -> [B,S]."""
    p = p.unsqueeze(1)
    pos, neg = (gt == 1).to(p.dtype), (gt < 1).to(p.dtype)
    pos_sum = (torch.log(p) * (1 - p) ** 2 * pos).sum(dim=(2, 3, 4))
    neg_sum = (torch.log(1 - p) * p ** 2 * (1 - gt) ** 4 * neg).sum(dim=(2, 3, 4))
    npos = pos.sum(dim=(2, 3, 4))
    return torch.where(npos == 0, -neg_sum, -(pos_sum + neg_sum) / torch.clamp(npos, min=1))


def reg(head, ind, target, mask, mode="l1", unc=None, ref=None, kl=None):
    """One gathered term -> [B,S].  mask [B,S,N] (one per entry, spread over the channels) or [B,S,N,C] (per element)."""
    pred = gather(head, ind)
    m = mask.to(pred.dtype)
    if m.dim() == 3:
        m = m.unsqueeze(3).expand_as(pred)
    t = target.to(pred.dtype)
    if mode == "l1":
        e = torch.abs(t * m - pred * m)
    elif mode == "resid":
        q = torch.exp(pred) * torch.as_tensor(ref, dtype=pred.dtype, device=pred.device)
        e = torch.abs(t * m - q * m)
    elif mode == "rel":
        tr = torch.where(t == 0, torch.full_like(t, float(np.float32(1e-6))), t)
        e = torch.abs((1 * m - pred * m) / tr)
    else:
        u = gather(unc, ind)
        kl = float(np.float32(kl))  # the reference's b = ones_like(a) * kl is a float32 tensor
        a = (t * m - pred * m) ** 2 if mode == "kld_key" else (t - pred) ** 2 * m
        v = torch.exp(u)
        e = (u - np.log(kl) + (kl * torch.exp(-a / kl) + a) / v - 1 + 0.5 * torch.abs(v)) * m
        return e.sum(dim=(2, 3)) / (m.sum(dim=(2, 3)) + 1e-6)
    return e.sum(dim=(2, 3)) / (m.sum(dim=(2, 3)) + 1e-4)


def on_terms(opt):
    on = {"hm", "hp"}
    for t, cond in (("wh", opt.reg_bbox and opt.wh_weight > 0), ("obj_scale", opt.obj_scale and opt.obj_scale_weight > 0),
                    ("off", opt.reg_offset and opt.off_weight > 0), ("hp_offset", opt.reg_hp_offset and opt.off_weight > 0),
                    ("hm_hp", opt.hm_hp and opt.hm_hp_weight > 0), ("tracking", opt.tracking and opt.tracking_weight > 0),
                    ("tracking_hp", opt.tracking_hp and opt.tracking_hp_weight > 0)):
        if cond:
            on.add(t)
    return on


def weights(opt):
    return {"hm": opt.hm_weight, "wh": opt.wh_weight, "off": opt.off_weight, "hp": opt.hp_weight, "hm_hp": opt.hm_hp_weight,
            "hp_offset": opt.off_weight, "obj_scale": opt.obj_scale_weight, "tracking": opt.tracking_weight,
            "tracking_hp": opt.tracking_hp_weight}


def object_pose_loss(opt, outputs, batch, phase, choice=None):
    """outputs: list of per-stack dicts of head tensors (logits for hm / hm_hp); batch: ground-truth tensors.
    ``choice`` [B] (optional) replaces the argmin's choice, to evaluate the loss at another selection.
    Returns dict(loss, stats {name: 0-d}, choice [B], terms {name: [B,S]}, maps [{hm, hm_hp}] per stack)."""
    on = on_terms(opt)
    ns = opt.num_stacks
    train = phase == "train"
    acc = {t: 0 for t in TERMS}
    maps = []
    for s in range(ns):
        o = outputs[s]
        mp = {"hm": clamp_sigmoid(o["hm"])}
        if opt.hm_hp:
            mp["hm_hp"] = clamp_sigmoid(o["hm_hp"])
        maps.append(mp)
        ind = batch["ind"]
        cur = {"hm": focal(mp["hm"], batch["hm"])}
        if opt.hps_uncertainty and train:
            cur["hp"] = reg(o["hps"], ind, batch["hps"], batch["hps_mask"], "kld_key", o["hps_uncertainty"],
                            kl=opt.KL_kps_uncertainty)
        else:
            cur["hp"] = reg(o["hps"], ind, batch["hps"], batch["hps_mask"])
        if "wh" in on:
            cur["wh"] = reg(o["wh"], ind, batch["wh"], batch["reg_mask"])
        if "obj_scale" in on:
            if not train:
                cur["obj_scale"] = reg(o["scale"], ind, batch["scale"], batch["reg_mask"], "rel")
            elif opt.obj_scale_uncertainty:
                cur["obj_scale"] = reg(o["scale"], ind, batch["scale"], batch["reg_mask"], "kld_scale",
                                       o["scale_uncertainty"], kl=opt.KL_scale_uncertainty)
            elif opt.use_residual:
                cur["obj_scale"] = reg(o["scale"], ind, batch["scale"], batch["reg_mask"], "resid", ref=opt.dimension_ref)
            else:
                cur["obj_scale"] = reg(o["scale"], ind, batch["scale"], batch["reg_mask"])
        if "off" in on:
            cur["off"] = reg(o["reg"], ind, batch["reg"], batch["reg_mask"])
        if "hp_offset" in on:
            cur["hp_offset"] = reg(o["hp_offset"], batch["hp_ind"], batch["hp_offset"], batch["hp_mask"])
        if "hm_hp" in on:
            cur["hm_hp"] = focal(mp["hm_hp"], batch["hm_hp"])
        if "tracking" in on:
            cur["tracking"] = reg(o["tracking"], ind, batch["tracking"], batch["tracking_mask"])
        if "tracking_hp" in on:
            cur["tracking_hp"] = reg(o["tracking_hp"], ind, batch["tracking_hp"], batch["tracking_hp_mask"])
        for t, v in cur.items():
            acc[t] = acc[t] + v / ns
    w = weights(opt)
    total = sum(w[t] * acc[t] for t in TERMS if t in on)
    valid = batch["ind"].sum(dim=2) > 0
    x = total * valid.to(total.dtype) + torch.where(valid, torch.zeros_like(total), torch.full_like(total, float("inf")))
    if choice is None:
        choice = torch.argmin(x, dim=1)
    rows = torch.arange(total.shape[0], device=total.device)
    chosen = {t: (acc[t][rows, choice].mean() if t in on else torch.zeros((), dtype=total.dtype, device=total.device))
              for t in TERMS}
    loss = sum(w[t] * chosen[t] for t in TERMS)
    stats = {"loss": loss}
    for k in STATS[1:]:
        stats[k] = chosen[k[:-5]]
    terms = {t: (acc[t] if t in on else torch.zeros_like(total)) for t in TERMS}
    return {"loss": loss, "stats": stats, "choice": choice, "terms": terms, "maps": maps, "total": total}
