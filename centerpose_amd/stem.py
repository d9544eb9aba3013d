"""The image stems on the library's kernels, forward and backward: ``stem_conv2d``, ``StemConv2d`` and ``use_hip_stems``.

The first layer of every backbone is a 7x7, padding-3 convolution of an image: ``base.base_layer.0`` (3 -> 16), ``pre_img_layer.0``
(3 -> 16) and ``pre_hm_layer.0`` (1 -> 16) of DLA (pose_dla_dcn.py:247-271) and ``conv1`` (3 -> 64, stride 2) of resnet_dcn.py.
``conv.Conv2d`` refuses them (``in_channels % 4``).  ``stem_conv2d`` reads the image as the NCHW planes a data loader hands over:
the forward re-lays them to 4-channel NHWC, as the inference engine's exact-f32 stem does, and runs the library's convolution on
the weight zero-padded to four input channels (precision: ``hip.set_default_precision``); the backward is
``cp_conv2d_stem_backward``, a float32 MFMA contraction for the weight and bias gradients (bitwise reproducible).  There is no
input gradient: the input is an image, and asking for one raises.

``StemConv2d`` is ``nn.Conv2d`` with that forward and nothing else changed, and ``use_hip_stems(model)`` re-classes a tree's
stems in place, as ``conv.use_hip_convs`` does for the other convolutions.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import hip as _hip
from ._layers import _nhwc, _on_device, _one, _reclass, _same


class _StemConv2dFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, relu):
        x = _hip._dev(x)
        w = _hip._dev(weight)
        cout, cin = w.shape[0], w.shape[1]
        # planes -> [B,H,W,4] with zero planes behind the image's; the weight likewise
        x4 = x.new_zeros((x.shape[0], x.shape[2], x.shape[3], 4))
        x4[..., :cin] = x.permute(0, 2, 3, 1)
        w4 = w.new_zeros((cout, 4, 7, 7))
        w4[:, :cin] = w
        y = _hip.conv2d_nhwc(x4, w4, shift=bias, stride=stride, pad=3, act=1 if relu else 0)
        ctx.stride, ctx.relu, ctx.has_bias = stride, relu, bias is not None
        ctx.save_for_backward(*((x, y) if relu else (x,)))
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x = ctx.saved_tensors[0]
        y = ctx.saved_tensors[1] if ctx.relu else None
        need_w = ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_w or need_b):
            return None, None, None, None, None
        gw, gb = _hip.conv2d_stem_backward(x, _nhwc(grad_out), stride=ctx.stride, y=y, need_bias_grad=need_b)
        return None, gw if need_w else None, gb if need_b else None, None, None


_RECLASS_MAX_COUT = 64  # use_hip_stems: what it has always re-classed
_MAX_COUT = 128         # stem_conv2d and a directly constructed StemConv2d (the hourglass's 3 -> 128 stem)


def _geometry_refusal(cin, cout, kernel, stride, pad, max_cout=_MAX_COUT):
    """Why (Cin, Cout, kernel, stride, padding) is not a stem the library runs, or None.  ``max_cout``: 128 for ``stem_conv2d``
    and ``StemConv2d``, 64 for what ``use_hip_stems`` re-classes."""
    if not 1 <= cin <= 3:
        return "in_channels = %d is outside 1..3" % cin
    if (kernel, pad) != (7, 3) or stride not in (1, 2):
        return "geometry outside kernel 7, padding 3, stride 1 or 2 (got %d, %d, %d)" % (kernel, pad, stride)
    if cout % 16 or not 16 <= cout <= max_cout:
        return "out_channels = %d is not a multiple of 16 from 16 to %d" % (cout, max_cout)
    return None


def stem_conv2d(x, weight, bias=None, stride=1, relu=False):
    """``relu?(F.conv2d(x, weight, bias, stride, padding=3))`` for a 7x7 stem on the HIP kernels with autograd.  ``x`` is a
    [B,Cin,H,W] float32 image on the device with Cin in 1..3 (NCHW planes); ``weight`` [Cout,Cin,7,7] with Cout a multiple of 16
    from 16 to 128; stride 1 or 2.  The result is channels_last.  ``x`` must not require a gradient."""
    _on_device(x)
    if x.dim() != 4 or weight.dim() != 4 or weight.shape[1] != x.shape[1]:
        raise RuntimeError("stem_conv2d: x must be [B,Cin,H,W] and weight [Cout,Cin,7,7], got %s and %s"
                           % (tuple(x.shape), tuple(weight.shape)))
    if weight.shape[2] != weight.shape[3]:
        raise NotImplementedError("stem_conv2d: the kernel must be square, got %s" % (tuple(weight.shape[2:]),))
    stride = _one(stride, "stem_conv2d", "stride")
    why = _geometry_refusal(weight.shape[1], weight.shape[0], weight.shape[2], stride, 3)
    if why:
        raise NotImplementedError("stem_conv2d: " + why)
    if x.requires_grad:
        raise NotImplementedError("stem_conv2d: the input is an image; its gradient is not built (detach it)")
    return _StemConv2dFn.apply(x, weight, bias, stride, bool(relu))


def _eligible(m, max_cout=_MAX_COUT):
    return (tuple(m.dilation) == (1, 1) and m.groups == 1 and m.padding_mode == 'zeros' and not isinstance(m.padding, str)
            and _same(m.kernel_size) and _same(m.stride) and _same(m.padding) and m.weight.dtype == torch.float32
            and _geometry_refusal(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0], max_cout) is None)


class StemConv2d(nn.Conv2d):
    """``nn.Conv2d`` for a 7x7 image stem whose forward and backward run on the library (``stem_conv2d``).  Constructor,
    parameters, initial values, ``state_dict`` and ``repr`` are ``nn.Conv2d``'s; ``relu = True`` fuses a following ReLU.
    Constructed directly it takes ``out_channels`` in multiples of 16 up to 128 (``use_hip_stems`` re-classes up to 64 only)."""
    relu = False

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if not _eligible(self):
            raise NotImplementedError("centerpose_amd.stem.StemConv2d: only Conv2d(1..3, 16 | 32 | ... | 128, 7, stride 1 | 2, "
                                      "padding 3) without dilation or groups is built")

    def _get_name(self):
        return "Conv2d"  # repr stays nn.Conv2d's, as it does for the other re-classed layers

    def forward(self, input):
        return stem_conv2d(input, self.weight, self.bias, self.stride[0], self.relu)


def use_hip_stems(module):
    """Re-class every exact ``nn.Conv2d`` under ``module`` (itself included) that is an image stem -- ``in_channels`` in 1..3,
    kernel 7, padding 3, stride 1 or 2, ``out_channels`` in {16, 32, 48, 64}, no dilation or groups -- to ``StemConv2d`` in
    place: the Parameter objects, the module names and the state-dict keys stay as they are.  Returns ``(converted, skipped)``;
    ``skipped`` is always empty, because every other module (``conv.use_hip_convs`` reports the convolutions) is left
    unmentioned and untouched.  A second call converts nothing.  The wider stems ``StemConv2d`` itself accepts (80 .. 128 output
    channels) are left alone here, as they always were: a caller's tree changes only where it did before."""
    return _reclass(module, (nn.Conv2d,), StemConv2d, lambda m: not _eligible(m, _RECLASS_MAX_COUT))[0], {}
