"""``DCNv2`` / ``DCN`` over ``_ext.dcn_v2_forward`` / ``_ext.dcn_v2_backward`` (the HIP kernels behind include/centerpose_hip.h).

What is contractual here is the reference's surface (DCNv2/dcn_v2.py:57-128): the constructor argument order, the state-dict
names (``weight``, ``bias``, ``conv_offset_mask.weight`` / ``.bias``), the initial values, and what ``forward`` means.  The
engine (csrc/engine_forward.hip) never goes through these modules; they exist for code that builds the reference's layers one by one
(the reference's own ``testcpu.py`` self-checks run against them, tests/test_gpu_parity.py)."""
import collections

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from centerpose_amd._layers import _precision_name, _set_backward_precision

from . import _ext

_Geometry = collections.namedtuple("_Geometry", "kernel stride pad dilation groups")


def _two(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


class _DCNv2(Function):
    """The reference's autograd function (dcn_v2.py:16-51): forward through ``_ext.dcn_v2_forward`` (the same kernels, and so
    the same values, as a call outside grad mode), backward through ``_ext.dcn_v2_backward``."""

    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups, backward_precision="f32"):
        ctx.backward_precision = _precision_name(backward_precision)
        ctx.stride, ctx.padding, ctx.dilation = _two(stride), _two(padding), _two(dilation)
        ctx.kernel_size = _two(weight.shape[2:4])
        ctx.deformable_groups = int(deformable_groups)
        output = _ext.dcn_v2_forward(input, weight, bias, offset, mask, ctx.kernel_size[0], ctx.kernel_size[1],
                                     ctx.stride[0], ctx.stride[1], ctx.padding[0], ctx.padding[1], ctx.dilation[0],
                                     ctx.dilation[1], ctx.deformable_groups)
        ctx.save_for_backward(input, offset, mask, weight, bias)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input, offset, mask, weight, bias = ctx.saved_tensors
        args = (input, weight, bias, offset, mask, grad_output, ctx.kernel_size[0], ctx.kernel_size[1], ctx.stride[0],
                ctx.stride[1], ctx.padding[0], ctx.padding[1], ctx.dilation[0], ctx.dilation[1], ctx.deformable_groups)
        if ctx.backward_precision == "f32":
            grads = _ext.dcn_v2_backward(*args)
        else:
            grads = _ext.dcn_v2_backward_prec(*args, precision=ctx.backward_precision)
        grad_input, grad_offset, grad_mask, grad_weight, grad_bias = grads
        # (one None per non-tensor argument; autograd drops the last where backward_precision was not passed)
        return grad_input, grad_offset, grad_mask, grad_weight, grad_bias, None, None, None, None, None


# the reference's nine arguments (dcn_v2.py:54), and an optional tenth: backward_precision
dcn_v2_conv = _DCNv2.apply


class DCNv2(nn.Module):
    """Modulated deformable convolution whose offsets and masks are inputs (dcn_v2.py:57-91).  ``backward_precision``: read
    at every forward, so a built module can be switched (``set_backward_precision``)."""
    backward_precision = "f32"

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__()
        g = _Geometry(_two(kernel_size), _two(stride), _two(padding), _two(dilation), int(deformable_groups))
        self.in_channels, self.out_channels = in_channels, out_channels
        # the reference's attribute names, for callers that read them back
        self.kernel_size, self.stride, self.padding, self.dilation, self.deformable_groups = g
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *g.kernel))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def taps(self):
        """Sampling points per output pixel: kernel area x deformable groups (a mask value each, two offsets each)."""
        return self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]

    def reset_parameters(self):
        bound = float(self.in_channels * self.kernel_size[0] * self.kernel_size[1]) ** -0.5   # 1 / sqrt(fan-in), dcn_v2.py:74-77
        nn.init.uniform_(self.weight, -bound, bound)
        nn.init.zeros_(self.bias)

    def _apply_op(self, x, offset, mask):
        return dcn_v2_conv(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                           self.deformable_groups, self.backward_precision)

    def forward(self, input, offset, mask):
        n = self.taps()
        if offset.shape[1] != 2 * n or mask.shape[1] != n:
            raise AssertionError("DCNv2: offset / mask need %d / %d channels, got %d / %d"
                                 % (2 * n, n, offset.shape[1], mask.shape[1]))
        return self._apply_op(input, offset, mask)


class DCN(DCNv2):
    """DCNv2 that predicts its own offsets and masks with a zero-initialised convolution of the same geometry
    (dcn_v2.py:94-128): the 3n channels of that convolution are [2n offsets | n mask logits]."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups)
        self.conv_offset_mask = nn.Conv2d(in_channels, 3 * self.taps(), self.kernel_size, self.stride, self.padding, bias=True)
        for t in (self.conv_offset_mask.weight, self.conv_offset_mask.bias):
            nn.init.zeros_(t)

    def forward(self, input):
        n = self.taps()
        om = self.conv_offset_mask(input)
        return self._apply_op(input, om[:, :2 * n].contiguous(), torch.sigmoid(om[:, 2 * n:]))


def set_backward_precision(module, name):
    """Set ``backward_precision`` ("f32" or "f16x3") on every ``DCNv2`` / ``DCN`` under ``module`` (itself included); returns how
    many were set.  ``PoseNet``, ``PoseNetGRU`` and the resdcn trees are built on these layers.  The offset convolutions inside
    ``DCN`` are not touched: ``centerpose_amd.conv.set_backward_precision`` is their switch."""
    return _set_backward_precision(module, name, lambda m: [(m, "backward_precision")] if isinstance(m, DCNv2) else [])
