"""``PoseHeads``: the prediction heads of the reference's networks as ONE autograd function over the fused HIP kernels.

The reference builds, per head, ``nn.Sequential(Conv2d(Cin, head_conv, 3, padding=1), ReLU, Conv2d(head_conv, classes, 1))``
and runs them in a loop on the same feature map (pose_dla_dcn.py:491-521 and :537-539; resnet_dcn.py likewise).  This module
owns the same parameters under the same state-dict names (``hm.0.weight``, ``hm.0.bias``, ``hm.2.weight``, ``hm.2.bias``, ...)
with the same deterministic initial values (``hm*`` final bias -2.19, other biases 0, :509-512), so
``load_state_dict(checkpoint, strict=False)`` takes a reference checkpoint and ``state_dict()`` merges back into one.

Forward is ``hip.pose_heads_forward`` (the same kernels, and so the same values, inside and outside grad mode); backward is one
``hip.pose_heads_backward`` call with every head's gradient (``None`` for a head the loss does not use).  Only the feature
map and the parameters are saved between the two: the hidden layers are recomputed, never stored.  The backward is float32
unless the module's ``backward_precision`` is "f16x3", which moves its three wide contractions per head onto split-binary16
matrix instructions (``hip.ops.pose_heads_backward_prec``; ``set_backward_precision`` sets it on a whole network).
"""
from collections import OrderedDict

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import hip as _hip
from ._layers import _precision_name, _set_backward_precision


class _PoseHeadsFn(Function):
    @staticmethod
    def forward(ctx, feat, backward_precision, *flat):
        params = [tuple(flat[4 * i:4 * i + 4]) for i in range(len(flat) // 4)]
        outs = _hip.pose_heads_forward(feat, params)
        ctx.backward_precision = backward_precision
        ctx.save_for_backward(feat, *flat)
        ctx.set_materialize_grads(False)   # a head the loss does not use arrives as None, not as a zero map
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_outs):
        feat, flat = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        params = [tuple(flat[4 * i:4 * i + 4]) for i in range(len(flat) // 4)]
        need_feat = ctx.needs_input_grad[0]
        gfeat, grads = _hip.ops.pose_heads_backward_prec(feat, params, list(grad_outs), need_feat_grad=need_feat,
                                                         precision=ctx.backward_precision)
        out = [gfeat, None]
        for i, g in enumerate(grads):
            out.extend(g[k] if ctx.needs_input_grad[2 + 4 * i + k] else None for k in range(4))
        return tuple(out)


class _Slot(nn.Module):
    """One layer's ``weight`` / ``bias`` under the index the reference's Sequential gives it."""

    def __init__(self, weight, bias):
        super().__init__()
        self.weight = nn.Parameter(weight)
        self.bias = nn.Parameter(bias)


class PoseHeads(nn.Module):
    """``PoseHeads(heads, in_channels, head_conv)``: ``heads`` maps head name -> classes (``opt.heads``).  ``forward(feat)``
    takes the [B, in_channels, H, W] feature map (NCHW-contiguous or channels_last) and returns the reference's ``z`` dict.
    ``backward_precision``: "f32" or "f16x3", the arithmetic of the backward's matrix products; an attribute, read at every
    forward, so a built module can be switched (``set_backward_precision``).  The forward's follows
    ``hip.set_default_precision``."""

    def __init__(self, heads, in_channels=64, head_conv=256, backward_precision="f32"):
        super().__init__()
        self.backward_precision = _precision_name(backward_precision)
        if head_conv <= 0:
            raise NotImplementedError("PoseHeads: head_conv must be positive (the single-convolution head form is not built)")
        if in_channels % 32 or head_conv % 32:
            raise NotImplementedError("PoseHeads: in_channels and head_conv must be multiples of 32, got %d and %d"
                                      % (in_channels, head_conv))
        self.heads = OrderedDict(heads)
        self.in_channels, self.head_conv = int(in_channels), int(head_conv)
        for name, classes in self.heads.items():
            if not 1 <= int(classes) <= 64:
                raise NotImplementedError("PoseHeads: head %r has %d classes (1..64 are built)" % (name, classes))
            # nn.Conv2d's own initialiser for the weights; biases as the reference sets them (pose_dla_dcn.py:509-512)
            c0 = nn.Conv2d(in_channels, head_conv, 3, padding=1)
            c1 = nn.Conv2d(head_conv, int(classes), 1)
            nn.init.zeros_(c0.bias)
            nn.init.constant_(c1.bias, -2.19 if 'hm' in name else 0.0)
            seq = nn.Module()
            seq.add_module('0', _Slot(c0.weight.detach().clone(), c0.bias.detach().clone()))
            seq.add_module('2', _Slot(c1.weight.detach().clone(), c1.bias.detach().clone()))
            self.add_module(name, seq)

    def head_params(self, name):
        seq = getattr(self, name)
        a, b = getattr(seq, '0'), getattr(seq, '2')
        return a.weight, a.bias, b.weight, b.bias

    def forward(self, feat):
        flat = [p for name in self.heads for p in self.head_params(name)]
        outs = _PoseHeadsFn.apply(feat, _precision_name(self.backward_precision), *flat)
        return OrderedDict(zip(self.heads, outs))


def set_backward_precision(module, name):
    """Set ``backward_precision`` ("f32" or "f16x3") on every ``PoseHeads`` under ``module`` (itself included); returns how many
    head blocks were set.  Besides the ``PoseHeads`` that are sub-modules it reaches the two ways a net holds its heads: a
    ``PoseHeads`` kept outside the sub-module tree as ``_head_block`` (``PoseNet``, whose state-dict keys carry no prefix), and a
    net that runs ``_PoseHeadsFn`` on its own parameters and carries the name as ``heads_backward_precision``
    (``PoseNetHourglass``, one block per stack, counted once).  ``conv.set_backward_precision`` is the switch of the
    ``Conv2d`` layers and leaves all of these alone."""
    def targets(m):
        for h in (m, m.__dict__.get("_head_block")):
            if isinstance(h, PoseHeads):
                yield h, "backward_precision"
        if hasattr(m, "heads_backward_precision"):
            yield m, "heads_backward_precision"

    return _set_backward_precision(module, name, targets)
