"""ObjectPoseLoss on the device: the reference's training loss (trains/object_pose.py:22-205) with its constructor and
call signature, computed by the cp_pose_loss_* kernels.

    loss, loss_stats, choice_list = ObjectPoseLoss(opt)(outputs, batch, phase)

``outputs`` is the model's list of per-stack head dicts, ``batch`` the dataset's collated ground truth on the same device.
``loss`` is a 0-d tensor with autograd to every head a counted term uses, ``loss_stats`` the reference's ten keys as 0-d
device tensors (a term that is off gives 0), ``choice_list`` the int64 [B] variant index per image.  As in the
reference, ``outputs[s]['hm']`` (and ``['hm_hp']`` with opt.hm_hp) hold clamp(sigmoid(logit)) afterwards, and the
tensor that held the logits holds sigmoid(logit): ``_sigmoid``'s ``sigmoid_`` side effect.  That tensor stays
differentiable as after ``sigmoid_``: a gradient arriving on it is chained through the sigmoid by the backward kernel.
The clamped maps are not differentiable here (the reference's trainer only reads them).

A reference tree picks it up with one line before the trainer is built:
    lib.trains.object_pose.ObjectPoseLoss = centerpose_amd.pose_loss.ObjectPoseLoss
"""
import torch

from . import hip

_REFUSED = (("mse_loss", "opt.mse_loss: MSELoss reduces the heat maps to a scalar, not a [B,S] matrix "
                         "(the reference marks it unsupported, object_pose.py:27)"),
            ("dense_hp", "opt.dense_hp: L1Loss(reduction='sum') gives a scalar, not a [B,S] matrix "
                         "(the reference marks it unsupported, object_pose.py:30)"),
            ("eval_oracle_hm", "opt.eval_oracle_hm: an oracle evaluation path on the host"),
            ("eval_oracle_hmhp", "opt.eval_oracle_hmhp: an oracle evaluation path on the host"),
            ("eval_oracle_kps", "opt.eval_oracle_kps: an oracle evaluation path on the host (numba)"),
            ("eval_oracle_hp_offset", "opt.eval_oracle_hp_offset: an oracle evaluation path on the host (numba)"))


def loss_config(opt, phase):
    """(terms, flags, weights) of cp_pose_loss_desc for ``opt`` and ``phase``: which terms count, as the reference's
    ``if`` chain decides (object_pose.py:76-160)."""
    T = hip.POSE_LOSS_TERMS
    on = {"hm", "hp"}
    if opt.reg_bbox and opt.wh_weight > 0:
        on.add("wh")
    if opt.obj_scale and opt.obj_scale_weight > 0:
        on.add("obj_scale")
    if opt.reg_offset and opt.off_weight > 0:
        on.add("off")
    if opt.reg_hp_offset and opt.off_weight > 0:
        on.add("hp_offset")
    if opt.hm_hp and opt.hm_hp_weight > 0:
        on.add("hm_hp")
    if opt.tracking and opt.tracking_weight > 0:
        on.add("tracking")
    if opt.tracking_hp and opt.tracking_hp_weight > 0:
        on.add("tracking_hp")
    terms = sum(1 << i for i, t in enumerate(T) if t in on)
    flags = (hip.PL_VAL if phase != "train" else 0) | (hip.PL_RESIDUAL if opt.use_residual else 0) | \
            (hip.PL_HPS_UNCERTAINTY if opt.hps_uncertainty else 0) | \
            (hip.PL_SCALE_UNCERTAINTY if opt.obj_scale_uncertainty else 0) | (hip.PL_HM_HP_MAPS if opt.hm_hp else 0)
    w = {"hm": opt.hm_weight, "wh": opt.wh_weight, "off": opt.off_weight, "hp": opt.hp_weight, "hm_hp": opt.hm_hp_weight,
         "hp_offset": opt.off_weight, "obj_scale": opt.obj_scale_weight, "tracking": opt.tracking_weight,
         "tracking_hp": opt.tracking_hp_weight}
    return terms, flags, [float(w[t]) for t in T]


class _PoseLossFn(torch.autograd.Function):
    # Every tensor the backward needs goes through save_for_backward, none onto ctx: the dirtied logits are outputs of
    # this node, and a tensor held in a ctx attribute would close a cycle (tensor -> grad_fn -> ctx -> tensor) that
    # keeps the heads, the ground truth and the workspace of every step alive.
    @staticmethod
    def forward(ctx, cfg, batch, layout, *flat):
        ns, names = layout
        outputs = [dict(zip(names, flat[s * len(names):(s + 1) * len(names)])) for s in range(ns)]
        terms, flags, weights, kl_kps, kl_scale, dimension_ref = cfg
        loss, stats, choice, _, clamped, state = hip.pose_loss_forward(outputs, batch, terms, flags, weights, kl_kps,
                                                                       kl_scale, dimension_ref)
        dirty = [o[h] for o in outputs for h in ("hm", "hm_hp") if h in state["heads"]]
        ctx.mark_dirty(*dirty)
        maps = [c for pair in clamped for c in pair if c is not None]
        ctx.mark_non_differentiable(stats, choice, *maps)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(state["ws"], *state["keep"], *flat)
        ctx.desc, ctx.layout, ctx.heads = state["desc"], layout, state["heads"]  # no tensors: see the class comment
        ctx.nkeep, ctx.nmaps = len(state["keep"]), len(maps)
        return (loss, stats, choice, *maps, *dirty)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss, _dstats, _dchoice, *rest):
        ns, names = ctx.layout
        saved = ctx.saved_tensors
        ws, keep, flat = saved[0], saved[1:1 + ctx.nkeep], saved[1 + ctx.nkeep:]
        outputs = [dict(zip(names, flat[s * len(names):(s + 1) * len(names)])) for s in range(ns)]
        # gradients arriving on the dirtied logits tensors (which hold sigmoid(logit)), in the order they were returned
        ddirty = iter(rest[ctx.nmaps:])
        dmaps = [tuple(next(ddirty) if h in ctx.heads else None for h in ("hm", "hm_hp")) for _ in range(ns)]
        if dloss is None:
            dloss = torch.zeros(1, dtype=torch.float32, device=ws.device)
        state = {"desc": ctx.desc, "ws": ws, "keep": keep, "heads": ctx.heads, "outputs": outputs}
        grads = hip.pose_loss_backward(state, dloss, dmaps)
        return (None, None, None, *[grads[s].get(h) for s in range(ns) for h in names])


class ObjectPoseLoss(torch.nn.Module):
    """Drop-in for the reference's ObjectPoseLoss(opt) (trains/object_pose.py:22-205).  Refuses, at construction, the
    options the device path does not cover: mse_loss, dense_hp, reg_loss other than 'l1', eval_oracle_*."""

    def __init__(self, opt):
        super().__init__()
        for name, why in _REFUSED:
            if getattr(opt, name, False):
                raise NotImplementedError("ObjectPoseLoss on the device: %s" % why)
        if getattr(opt, "reg_loss", "l1") != "l1":
            raise NotImplementedError("ObjectPoseLoss on the device: opt.reg_loss=%r; only 'l1' (RegL1Loss) is supported "
                                      "(the reference marks RegLoss unsupported, object_pose.py:36)" % opt.reg_loss)
        self.opt = opt

    def forward(self, outputs, batch, phase):
        opt = self.opt
        terms, flags, weights = loss_config(opt, phase)
        ref = tuple(float(x) for x in opt.dimension_ref) if opt.use_residual else (1.0, 1.0, 1.0)
        cfg = (terms, flags, weights, float(opt.KL_kps_uncertainty), float(opt.KL_scale_uncertainty), ref)
        heads, _ = hip._pl_used(terms, flags)
        names = tuple(h for h in hip.POSE_LOSS_HEADS if h in heads)
        ns = int(opt.num_stacks)
        flat = [outputs[s][h] for s in range(ns) for h in names]
        res = _PoseLossFn.apply(cfg, batch, (ns, names), *flat)
        loss, stats, choice = res[0], res[1], res[2]
        maps_per = [h for h in ("hm", "hm_hp") if h in names]
        maps = res[3:3 + ns * len(maps_per)]
        for s in range(ns):
            for j, h in enumerate(maps_per):
                outputs[s][h] = maps[s * len(maps_per) + j]
        loss_stats = {k: stats[i] for i, k in enumerate(hip.POSE_LOSS_STATS)}
        loss_stats["loss"] = loss
        return loss, loss_stats, choice
