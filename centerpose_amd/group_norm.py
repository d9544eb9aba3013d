"""GroupNorm on the library's kernels, forward and backward, fused with the ReLU that follows it: ``group_norm``,
``GroupNorm`` and ``use_hip_group_norms``.  The sibling of ``norm.py``.

The heads of the reference's ``dlav1_34`` are conv3x3 -> ``nn.GroupNorm`` -> ReLU -> conv1x1 (pose_dla_dcn.py:491-521, groups by
GN.py: 32 when the width divides by 32, else 16).  ``group_norm`` is one autograd function over ``cp_groupnorm_forward_nhwc``
(one statistics pass and one fused apply pass) and ``cp_groupnorm_backward_nhwc`` (one reduction and one apply pass);
float32, bitwise reproducible.  ``GroupNorm`` is ``nn.GroupNorm`` with that forward and nothing else changed, and
``use_hip_group_norms(model)`` re-classes a tree's eligible layers in place, the contract of ``norm.use_hip_norms``.

``num_channels % 4 != 0``, a group width that is neither 1, 2 nor a multiple of 4 (48 channels in 16 groups) and bf16 are not
built.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import hip as _hip
from ._layers import _nhwc, _on_device, _reclass


class _GroupNormFn(Function):
    @staticmethod
    def forward(ctx, x, num_groups, weight, bias, eps, relu):
        y, mean, invstd = _hip.group_norm_forward(_nhwc(x), num_groups, weight, bias, eps, act=1 if relu else 0)
        ctx.groups, ctx.relu, ctx.affine = num_groups, relu, weight is not None
        ctx.save_for_backward(*((x, mean, invstd) + ((weight,) if ctx.affine else ()) + ((y,) if relu else ())))
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, mean, invstd = ctx.saved_tensors[:3]
        weight = ctx.saved_tensors[3] if ctx.affine else None
        y = ctx.saved_tensors[-1] if ctx.relu else None
        need_x, _, need_w, need_b = ctx.needs_input_grad[:4]
        if not (need_x or need_w or need_b):
            return (None,) * 6
        gx, gw, gb = _hip.group_norm_backward(_nhwc(x), _nhwc(grad_out), ctx.groups, mean, invstd, gamma=weight, y=y,
                                              need_x_grad=need_x, need_gamma_grad=need_w, need_beta_grad=need_b)
        return (gx.permute(0, 3, 1, 2) if need_x else None, None, gw, gb, None, None)


def _group_refusal(C, G):
    """Why the kernels refuse ``C`` channels in ``G`` groups, or None."""
    if C % 4 or not 4 <= C <= 4096:
        return "num_channels = %d is not a multiple of 4 in 4..4096" % C
    if G < 1 or C % G:
        return "num_groups = %d does not divide num_channels = %d" % (G, C)
    if C // G not in (1, 2) and (C // G) % 4:
        return "%d channels per group (only 1, 2 or a multiple of 4 is built)" % (C // G)
    return None


def group_norm(x, num_groups, weight, bias, eps=1e-5, relu=False):
    """``relu?(F.group_norm(x, num_groups, weight, bias, eps))`` on the HIP kernels with autograd.  ``x`` is a logical [B,C,H,W]
    float32 tensor on the device, NCHW-contiguous or channels_last (the kernels read NHWC; channels_last costs no copy); the
    result and the gradients are channels_last.  ``weight`` / ``bias`` None: 1 / 0.  ``C % 4 == 0`` and ``C / num_groups`` 1, 2
    or a multiple of 4."""
    _on_device(x)
    if x.dim() != 4:
        raise RuntimeError("group_norm: x must be [B,C,H,W], got %s" % (tuple(x.shape),))
    for name, t in (("x", x), ("weight", weight), ("bias", bias)):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("group_norm: %s is %s (only float32 is built)" % (name, t.dtype))
    why = _group_refusal(x.shape[1], int(num_groups))
    if why:
        raise RuntimeError("group_norm: " + why)
    return _GroupNormFn.apply(x, int(num_groups), weight, bias, float(eps), bool(relu))


class GroupNorm(nn.GroupNorm):
    """``nn.GroupNorm`` whose forward and backward run on the library (``group_norm``).  Constructor, parameters, initial
    values, ``state_dict`` and ``repr`` are ``nn.GroupNorm``'s; ``relu = True`` fuses a following ReLU into the layer."""
    relu = False

    def forward(self, input):
        return group_norm(input, self.num_groups, self.weight, self.bias, self.eps, self.relu)


def _refusal(m):
    """Why the library cannot run this nn.GroupNorm's configuration, or None."""
    why = _group_refusal(m.num_channels, m.num_groups)
    if why:
        return why
    for t in (m.weight, m.bias):
        if t is not None and t.dtype != torch.float32:
            return "dtype %s (only float32 is built)" % t.dtype
    return None


def use_hip_group_norms(module):
    """Re-class every eligible ``nn.GroupNorm`` under ``module`` (itself included) to ``GroupNorm`` in place: the Parameter
    objects, the module names and the state-dict keys stay as they are.  Returns ``(converted, skipped)``: the converted
    modules' names and ``{name: reason}`` for the GroupNorm layers left alone (``num_channels % 4``, a group width the kernels
    refuse, a dtype other than float32, user-derived subclasses).  Modules that already are ``GroupNorm`` appear in neither, and
    no other kind of module is mentioned or touched."""
    return _reclass(module, (nn.GroupNorm,), GroupNorm, _refusal)
