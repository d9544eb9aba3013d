"""``PoseNetGRU``: the reference's ``dlav1_34`` tracking network (``DLASeg`` with the ConvGRU, pose_dla_dcn.py:457-570) as one
trainable ``nn.Module`` whose layers all run on the library, forward and backward.

Backbone and up-sampling are ``pose_net.py``'s (``DLA``, ``DLAUp``, ``IDAUp``).  Behind them sits ``conv_gru.ConvGRU`` (3 steps, 4
with ``opt.tracking_task``), and every head is conv3x3 -> GroupNorm -> ReLU -> conv1x1 on the GRU step the reference routes
it to (pose_dla_dcn.py:545-563): ``conv.Conv2d``, ``group_norm.GroupNorm`` with the ReLU fused, ``conv.Conv2d``.  The module tree
and ``state_dict()`` are the reference's (``synth.param_spec('dlav1_34', ...)``), so its checkpoints load with ``strict=True``.

``HipPoseNet.load_module()`` takes a trained ``PoseNetGRU`` into the inference engine; ``PoseNetGRU.from_model(model)`` builds
one from a ``HipPoseNet`` of arch ``dlav1_34``.
"""
from collections import OrderedDict

import torch
from torch import nn

from .conv import Conv2d
from .conv_gru import ConvGRU
from .group_norm import GroupNorm
from .pose_net import compose_backbone, run_backbone

# pose_dla_dcn.py:545-563: the GRU step each head reads
_ROUTE = {"hm": 0, "wh": 0, "reg": 0, "hm_hp": 1, "hp_offset": 1, "hps": 1, "scale": 2}
_ROUTE_TRACKING = {"tracking": 0, "tracking_hp": 0, "hm": 1, "wh": 1, "reg": 1, "hm_hp": 2, "hp_offset": 2, "hps": 2,
                   "hps_uncertainty": 2, "scale": 3, "scale_uncertainty": 3}


def gn_groups(channels):
    """GN.py:4-9"""
    return 32 if channels % 32 == 0 else 16


def _head(classes, head_conv, is_hm):
    """pose_dla_dcn.py:491-510 under the reference's Sequential indices 0, 1, 3; the ReLU (index 2) runs inside the GroupNorm"""
    gn = GroupNorm(gn_groups(head_conv), head_conv)
    gn.relu = True
    final = Conv2d(head_conv, classes, 1, stride=1, padding=0, bias=True)
    if is_hm:
        nn.init.constant_(final.bias, -2.19)
    return nn.Sequential(Conv2d(64, head_conv, 3, padding=1, bias=True), gn, nn.Identity(), final)


class PoseNetGRU(nn.Module):
    """``PoseNetGRU(heads, head_conv=256, opt=None)``: ``dlav1_34``.  ``heads`` maps head name -> classes (``opt.heads``); ``opt``
    may set ``pre_img`` / ``pre_hm`` / ``pre_hm_hp`` (which previous-frame stems exist) and ``tracking_task`` (4 GRU steps and the
    tracking routing), as for ``create_model``.  ``forward(x, pre_img=None, pre_hm=None, pre_hm_hp=None)`` takes NCHW images on
    the device and returns ``[z]``, ``z`` the dict of raw head maps, like ``DLASeg``."""
    arch = "dlav1_34"

    def __init__(self, heads, head_conv=256, opt=None):
        super().__init__()
        self.heads = OrderedDict(heads)
        self.head_conv = int(head_conv)
        if self.head_conv <= 0:
            raise NotImplementedError("PoseNetGRU: head_conv must be positive, got %d" % self.head_conv)
        self.tracking_task = bool(opt is not None and getattr(opt, "tracking_task", False))
        self.route = _ROUTE_TRACKING if self.tracking_task else _ROUTE
        for name in self.heads:
            if name not in self.route:
                raise NotImplementedError("PoseNetGRU: head %r is fed by no ConvGRU step (%s routes %s)"
                                          % (name, "tracking_task" if self.tracking_task else "the plain network", sorted(self.route)))
        compose_backbone(self, opt)
        steps = 4 if self.tracking_task else 3
        self.convGRU = ConvGRU(64, [64], 3, step=steps, effective_step=list(range(steps)))
        self.ida_up = self._modules.pop("ida_up")  # the reference registers it after the ConvGRU (the state dict's order)
        for name, classes in self.heads.items():
            if name in self._modules or hasattr(self, name):
                raise ValueError("PoseNetGRU: head name %r collides with an attribute of the module" % name)
            self.add_module(name, _head(classes, self.head_conv, "hm" in name))

    def forward(self, x, pre_img=None, pre_hm=None, pre_hm_hp=None):
        outputs, _ = self.convGRU(run_backbone(self, x, pre_img, pre_hm, pre_hm_hp))
        z = {}
        for name in self.heads:
            h = getattr(self, name)
            z[name] = h[3](h[1](h[0](outputs[self.route[name]])))
        return [z]

    @classmethod
    def from_model(cls, model):
        """A ``PoseNetGRU`` holding copies of a ``HipPoseNet``'s current parameters and buffers (train it, then
        ``model.load_module(net)``)."""
        if getattr(model, "arch", None) != cls.arch:
            raise NotImplementedError("PoseNetGRU.from_model: the model is %r, not %s" % (getattr(model, "arch", None), cls.arch))
        net = cls(model.heads, model.head_conv, model.opt)
        net.load_state_dict(model.state_dict(), strict=True)
        return net
