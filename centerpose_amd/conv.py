"""Ordinary convolutions on the library's kernels, forward and backward: ``conv2d``, ``Conv2d`` and ``use_hip_convs``.

The reference's backbones are mostly ``nn.Conv2d``: DLA's ``BasicBlock`` 3x3 pairs (pose_dla_dcn.py:48-62), the 1x1 ``Root`` and
``project`` layers, ResNet's 1x1 stride-2 down-samples and the 3x3 ``conv_offset_mask`` of every ``DCN`` (DCNv2/dcn_v2.py:118-128).
``conv2d`` is one autograd function over ``cp_conv2d_nhwc`` (forward; precision follows ``hip.set_default_precision``) and
``cp_conv2d_backward_nhwc`` (backward; bitwise reproducible; float32 unless the layer's ``backward_precision`` is "f16x3",
which moves the weight and data gradient of the MFMA geometries onto split-binary16 matrix instructions:
``cp_conv2d_backward_prec_nhwc``).  ``Conv2d`` is ``nn.Conv2d`` with that forward and nothing else changed, and ``use_hip_convs(model)`` re-classes a tree's eligible convolutions in place, so a network that trains through
torch moves its convolutions onto the library in one line and keeps its parameters, optimizer state and checkpoints.

BatchNorm and the residual adds are ``norm.py``'s (``use_hip_norms``); pooling and everything else stay torch's; dilation, groups
and ``in_channels % 4 != 0`` are not built.
"""
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import hip as _hip
from ._layers import _nhwc, _on_device, _one, _precision_name, _reclass, _same, _set_backward_precision


class _Conv2dFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, relu, backward_precision):
        y = _hip.conv2d_nhwc(_nhwc(x), weight, shift=bias, stride=stride, pad=pad, act=1 if relu else 0)
        ctx.stride, ctx.pad, ctx.relu, ctx.has_bias = stride, pad, relu, bias is not None
        ctx.backward_precision = backward_precision
        if relu:
            ctx.save_for_backward(x, weight, y)
        else:
            ctx.save_for_backward(x, weight)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors[:2]
        y = ctx.saved_tensors[2] if ctx.relu else None
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_x or need_w or need_b):
            return None, None, None, None, None, None, None
        gx, gw, gb = _hip.ops.conv2d_backward_prec(_nhwc(x), weight, _nhwc(grad_out), stride=ctx.stride, pad=ctx.pad, y=y,
                                                   need_x_grad=need_x, need_bias_grad=need_b,
                                                   precision=ctx.backward_precision)
        return (gx.permute(0, 3, 1, 2) if need_x else None, gw if need_w else None, gb if need_b else None, None, None, None,
                None)


def _geometry_refusal(cin, kh, kw, stride, pad):
    """Why the kernels cannot run a convolution of this geometry, or None: the one rule of ``conv2d``, ``Conv2d`` and
    ``use_hip_convs``, and the library's own for the backward (``conv_bwd_shape_error``, csrc/ops.hip).  Kernel 1..7 on each axis,
    stride 1..4, ``0 <= pad < min(kh, kw)``, ``cin`` a positive multiple of 4."""
    if cin < 4 or cin % 4:
        return "in_channels = %d is not a multiple of 4" % cin
    if not (1 <= kh <= 7 and 1 <= kw <= 7 and 1 <= stride <= 4 and 0 <= pad < min(kh, kw)):
        return "geometry outside kernel 1..7, stride 1..4, padding < kernel"
    return None


def conv2d(x, weight, bias=None, stride=1, padding=0, relu=False, backward_precision="f32"):
    """``relu?(F.conv2d(x, weight, bias, stride, padding))`` on the HIP kernels with autograd.  ``x`` is a logical [B,Cin,H,W] tensor on
    the device, NCHW-contiguous or channels_last (the kernels read NHWC; channels_last costs no copy); the result is
    channels_last.  Dilation 1, groups 1, and the geometry of ``_geometry_refusal``: what the backward refuses raises
    NotImplementedError here, before the forward runs.  ``backward_precision``: "f32" or "f16x3", the arithmetic of the backward's
    matrix products (``hip.ops.conv2d_backward_prec``); the forward's follows ``hip.set_default_precision``."""
    backward_precision = _precision_name(backward_precision)
    _on_device(x)
    if x.dim() != 4 or weight.dim() != 4 or weight.shape[1] != x.shape[1]:
        raise RuntimeError("conv2d: x must be [B,Cin,H,W] and weight [Cout,Cin,KH,KW], got %s and %s"
                           % (tuple(x.shape), tuple(weight.shape)))
    stride, padding = _one(stride, "conv2d", "stride"), _one(padding, "conv2d", "padding")
    why = _geometry_refusal(int(weight.shape[1]), int(weight.shape[2]), int(weight.shape[3]), stride, padding)
    if why:
        raise NotImplementedError("conv2d: " + why)
    return _Conv2dFn.apply(x, weight, bias, stride, padding, bool(relu), backward_precision)


def _refusal(m):
    """Why the library cannot run this nn.Conv2d's configuration, or None."""
    if tuple(m.dilation) != (1, 1):
        return "dilation %r (only 1 is built)" % (tuple(m.dilation),)
    if m.groups != 1:
        return "groups = %d (only 1 is built)" % m.groups
    if m.padding_mode != 'zeros':
        return "padding_mode %r (only 'zeros' is built)" % m.padding_mode
    if isinstance(m.padding, str):
        return "string padding %r" % m.padding
    if not (_same(m.stride) and _same(m.padding)):
        return "stride / padding differ between the axes"
    return _geometry_refusal(m.in_channels, m.kernel_size[0], m.kernel_size[1], m.stride[0], m.padding[0])


class Conv2d(nn.Conv2d):
    """``nn.Conv2d`` whose forward and backward run on the library (``conv2d``).  Constructor, parameters, initial values,
    ``state_dict`` and ``repr`` are ``nn.Conv2d``'s; ``relu = True`` fuses a following ReLU into the layer;
    ``backward_precision = "f16x3"`` runs the backward's matrix products in split binary16 (``set_backward_precision``)."""
    relu = False
    backward_precision = "f32"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        why = _refusal(self)
        if why:
            raise NotImplementedError("centerpose_amd.conv.Conv2d: " + why)

    def forward(self, input):
        return conv2d(input, self.weight, self.bias, self.stride[0], self.padding[0], self.relu, self.backward_precision)


def set_backward_precision(module, name):
    """Set ``backward_precision`` ("f32" or "f16x3") on every ``Conv2d`` under ``module`` (itself included); returns how many were
    set.  One line moves a network built on these layers -- ``PoseNet``, ``PoseNetGRU``, ``PoseNetHourglass`` -- onto the mode."""
    return _set_backward_precision(module, name, lambda m: [(m, "backward_precision")] if isinstance(m, Conv2d) else [])


def use_hip_convs(module, backward_precision=None):
    """Re-class every eligible ``nn.Conv2d`` under ``module`` (itself included) to ``Conv2d`` in place: the Parameter objects, the
    module names and the state-dict keys stay as they are.  Returns ``(converted, skipped)``: the converted modules' names and
    ``{name: reason}`` for the convolutions left alone (groups, dilation, ``in_channels % 4``, transposed or subclassed
    convolutions).  Modules that already are ``Conv2d`` appear in neither.  ``backward_precision``: None leaves every layer's
    attribute alone; a name sets it on every ``Conv2d`` under ``module`` afterwards (``set_backward_precision``)."""
    if backward_precision is not None:
        _precision_name(backward_precision)
    res = _reclass(module, (nn.Conv2d,), Conv2d, _refusal, of=" of nn.Conv2d",
                   unbuilt=((nn.ConvTranspose2d, "ConvTranspose2d is not built"),))
    if backward_precision is not None:
        set_backward_precision(module, backward_precision)
    return res
