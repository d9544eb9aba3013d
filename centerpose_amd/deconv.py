"""Transposed convolutions on the library's kernels, forward and backward: ``conv_transpose2d``, ``ConvTranspose2d`` and
``use_hip_deconvs``.

Both backbone families up-sample with ``nn.ConvTranspose2d``.  DLA's ``IDAUp`` (pose_dla_dcn.py:402-417) runs
``layers[i] = up(proj(layers[i]))`` and then ``node(layers[i] + layers[i - 1])`` with the depth-wise
``up = ConvTranspose2d(o, o, 2f, stride=f, padding=f // 2, groups=o, bias=False)``; resnet_dcn.py:232-240 stacks three dense
``ConvTranspose2d(planes, planes, 4, stride=2, padding=1, bias=False)``.  ``conv_transpose2d`` is one autograd function over
``cp_conv_transpose2d_dw_nhwc`` / ``cp_conv_transpose2d_nhwc`` (forward; the dense one's precision follows
``hip.set_default_precision``) and ``cp_conv_transpose2d_backward_nhwc`` (backward; bitwise reproducible; float32 unless the
layer's ``backward_precision`` is "f16x3", which moves the dense layer's weight and data gradient onto split-binary16 matrix
instructions: ``cp_conv_transpose2d_backward_prec_nhwc``; the depth-wise layers have no matrix product and stay float32).
``ConvTranspose2d`` is ``nn.ConvTranspose2d`` with that forward and nothing else changed, and ``use_hip_deconvs(model)`` re-classes
a tree's eligible layers in place, as ``conv.use_hip_convs`` and ``norm.use_hip_norms`` do for theirs.

A bias, ``output_padding``, dilation and every other kernel / stride pair are not built.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import hip as _hip
from ._layers import _nhwc, _on_device, _one, _precision_name, _reclass, _same, _set_backward_precision

_DW_TABLE_BYTES = 61440  # the depth-wise kernels' LDS weight table (include/centerpose_hip.h)


class _ConvTranspose2dFn(Function):
    _backward_precision = "f32"  # (the backward reads it from the function class its context belongs to)

    @staticmethod
    def forward(ctx, x, weight, add, stride, pad, groups):
        xh = _nhwc(x)
        if groups == 1:
            y = _hip.conv_transpose2d(xh, weight)
        else:
            y = _hip.conv_transpose2d_dw(xh, weight, stride, add=None if add is None else _nhwc(add))
        ctx.stride, ctx.pad, ctx.groups = stride, pad, groups
        ctx.save_for_backward(x, weight)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_add = ctx.needs_input_grad[:3]
        gx = gw = None
        if need_x or need_w:
            gx, gw = _hip.ops.conv_transpose2d_backward(_nhwc(x), weight, _nhwc(grad_out), ctx.stride, ctx.pad, ctx.groups,
                                                        need_x_grad=need_x, precision=ctx._forward_cls._backward_precision)
        return (gx.permute(0, 3, 1, 2) if need_x else None, gw if need_w else None, grad_out if need_add else None, None, None,
                None)


class _ConvTranspose2dF16x3Fn(_ConvTranspose2dFn):
    """The same function with the backward's matrix products in split binary16 (the arguments stay the six above)."""
    _backward_precision = "f16x3"


_FUNCTIONS = {"f32": _ConvTranspose2dFn, "f16x3": _ConvTranspose2dF16x3Fn}


def _geometry_refusal(cin, cout, k, stride, pad, groups):
    """Why (Cin, Cout, K, stride, pad, groups) is outside the two geometries the library runs, or None."""
    if groups == 1:
        if (k, stride, pad) != (4, 2, 1):
            return "geometry outside the table: a dense layer must be kernel 4, stride 2, padding 1 (got %d, %d, %d)" % (k, stride, pad)
        if cin % 32 or cout % 32:
            return "geometry outside the table: dense channels (%d -> %d) must be multiples of 32" % (cin, cout)
        return None
    if not (groups == cin == cout):
        return "geometry outside the table: groups = %d is neither 1 nor depth-wise (in = out = groups; got %d -> %d)" % (groups, cin, cout)
    if stride not in (2, 4) or k != 2 * stride or pad != stride // 2:
        return ("geometry outside the table: a depth-wise layer must be stride f in {2, 4}, kernel 2f, padding f // 2 "
                "(got kernel %d, stride %d, padding %d)" % (k, stride, pad))
    if cin % 4:
        return "geometry outside the table: channels = %d is not a multiple of 4" % cin
    if cin * k * k * 4 > _DW_TABLE_BYTES:
        return "geometry outside the table: %d channels x %d taps do not fit the kernels' LDS weight table" % (cin, k * k)
    return None


def _refusal(m):
    """Why the library cannot run this nn.ConvTranspose2d's configuration, or None."""
    if m.bias is not None:
        return "a bias is not built"
    if tuple(m.output_padding) != (0, 0):
        return "output_padding %r (only 0 is built)" % (tuple(m.output_padding),)
    if tuple(m.dilation) != (1, 1):
        return "dilation %r (only 1 is built)" % (tuple(m.dilation),)
    if m.padding_mode != 'zeros':
        return "padding_mode %r (only 'zeros' is built)" % m.padding_mode
    if m.weight.dtype != torch.float32:
        return "dtype %s (only float32 is built)" % m.weight.dtype
    if not (_same(m.kernel_size) and _same(m.stride) and _same(m.padding)):
        return "geometry outside the table: kernel / stride / padding differ between the axes"
    return _geometry_refusal(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0], m.groups)


def conv_transpose2d(x, weight, stride, padding, groups=1, add=None, backward_precision="f32"):
    """``F.conv_transpose2d(x, weight, None, stride, padding, groups=groups) (+ add)`` on the HIP kernels with autograd.  ``x`` is a
    logical [B,Cin,H,W] tensor on the device, NCHW-contiguous or channels_last (the kernels read NHWC; channels_last costs no
    copy); the result and the gradients are channels_last.  Depth-wise (groups == Cin == Cout, stride f in {2, 4}, kernel 2f,
    padding f // 2; ``add`` [B,C,fH,fW] is IDAUp's ``+ layers[i - 1]``, fused, and its gradient is grad_out itself) or dense
    (groups 1, kernel 4, stride 2, padding 1, channels % 32 == 0; precision: ``hip.set_default_precision``).
    ``backward_precision``: "f32" or "f16x3", the arithmetic of the dense backward's matrix products
    (``hip.ops.conv_transpose2d_backward``); a depth-wise layer is float32 in either."""
    backward_precision = _precision_name(backward_precision)
    _on_device(x)
    groups = int(groups)
    if x.dim() != 4 or weight.dim() != 4 or weight.shape[0] != x.shape[1] or weight.shape[2] != weight.shape[3] or groups < 1:
        raise RuntimeError("conv_transpose2d: x must be [B,Cin,H,W] and weight [Cin,Cout/groups,K,K], got %s and %s"
                           % (tuple(x.shape), tuple(weight.shape)))
    stride, padding = _one(stride, "conv_transpose2d", "stride"), _one(padding, "conv_transpose2d", "padding")
    why = _geometry_refusal(x.shape[1], weight.shape[1] * groups, weight.shape[2], stride, padding, groups)
    if why:
        raise NotImplementedError("conv_transpose2d: " + why)
    if add is not None:
        if groups == 1:
            raise NotImplementedError("conv_transpose2d: `add` is fused into the depth-wise layer only")
        want = (x.shape[0], x.shape[1], stride * x.shape[2], stride * x.shape[3])
        if tuple(add.shape) != want:
            raise RuntimeError("conv_transpose2d: add has shape %s, expected %s" % (tuple(add.shape), want))
    return _FUNCTIONS[backward_precision].apply(x, weight, add, stride, padding, groups)


class ConvTranspose2d(nn.ConvTranspose2d):
    """``nn.ConvTranspose2d`` whose forward and backward run on the library (``conv_transpose2d``).  Constructor, parameters,
    initial values, ``state_dict`` and ``repr`` are ``nn.ConvTranspose2d``'s; ``forward(input, add)`` adds ``add`` to the
    up-sampled tensor inside the kernel (depth-wise layers: IDAUp's ``layers[i] + layers[i - 1]``);
    the instance attribute ``backward_precision`` ("f32" at construction and after a re-class; ``set_backward_precision``) set to
    "f16x3" runs a dense layer's backward matrix products in split binary16.  The class body adds nothing but ``forward``."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.backward_precision = "f32"
        why = _refusal(self)
        if why:
            raise NotImplementedError("centerpose_amd.deconv.ConvTranspose2d: " + why)

    def forward(self, input, add=None):
        return conv_transpose2d(input, self.weight, self.stride[0], self.padding[0], self.groups, add, getattr(self, "backward_precision", "f32"))


def set_backward_precision(module, name):
    """Set ``backward_precision`` ("f32" or "f16x3") on every ``ConvTranspose2d`` under ``module`` (itself included); returns how
    many were set.  ``PoseNetResDCN`` has three dense ones; a depth-wise layer takes the name and stays float32."""
    return _set_backward_precision(module, name, lambda m: [(m, "backward_precision")] if isinstance(m, ConvTranspose2d) else [])


def use_hip_deconvs(module, backward_precision=None):
    """Re-class every eligible ``nn.ConvTranspose2d`` under ``module`` (itself included) to ``ConvTranspose2d`` in place: the
    Parameter objects, the module names and the state-dict keys stay as they are.  Returns ``(converted, skipped)``: the
    converted modules' names and ``{name: reason}`` for the transposed convolutions left alone (a bias, ``output_padding``,
    dilation, a dtype other than float32, a geometry outside the two the library runs, subclasses).  Modules that already are
    ``ConvTranspose2d`` appear in neither, and no other kind of module is mentioned or touched.  ``backward_precision``: None
    leaves every layer's attribute alone; a name sets it on every ``ConvTranspose2d`` under ``module`` afterwards
    (``set_backward_precision``)."""
    if backward_precision is not None:
        _precision_name(backward_precision)
    res = _reclass(module, (nn.ConvTranspose2d,), ConvTranspose2d, _refusal, of=" of nn.ConvTranspose2d",
                   converted_hook=lambda m: setattr(m, "backward_precision", "f32"))
    if backward_precision is not None:
        set_backward_precision(module, backward_precision)
    return res
