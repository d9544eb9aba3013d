"""The hourglass merge on the library's kernels, forward and backward: ``upsample2_add`` and ``UpsampleAdd``.  The sibling of
``pool.py``.

Every ``kp_module`` of the stacked hourglass ends in ``up1 + Upsample(scale_factor=2)(low3)`` (large_hourglass.py:95-112 and
:176-187: ``make_unpool_layer``, ``MergeUp``), nearest neighbour: ten merges per step of the two-stack network, the first two on
its largest activations.  ``upsample2_add`` is one autograd function over ``cp_upsample2_add_nhwc`` and
``cp_upsample2_add_backward_nhwc``: one pass each way instead of torch's three.  It saves nothing: the gradient of ``low`` is
the sum of each 2x2 cell of the incoming gradient in a fixed order (bitwise reproducible), and the gradient of ``up1`` is the
incoming gradient itself -- the same tensor, no kernel and no copy.

Other scale factors, interpolation modes and ``C % 4 != 0`` are not built.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._layers import _nhwc, _on_device
from .hip import ops as _ops


class _Upsample2AddFn(Function):
    @staticmethod
    def forward(ctx, up1, low):
        ctx.low_shape = tuple(low.shape)
        return _ops.upsample2_add_forward(_nhwc(up1), _nhwc(low)).permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        grad_low = None
        if ctx.needs_input_grad[1]:
            B, C, H, W = ctx.low_shape
            grad_low = _ops.upsample2_add_backward(_nhwc(grad_out), (B, H, W, C)).permute(0, 3, 1, 2)
        return grad_out if ctx.needs_input_grad[0] else None, grad_low


def upsample2_add(up1, low):
    """``up1 + F.interpolate(low, scale_factor=2)`` (nearest) on the HIP kernels with autograd.  ``low`` is a logical [B,C,H,W]
    float32 tensor on the device and ``up1`` [B,C,2H,2W], each NCHW-contiguous or channels_last (the kernels read NHWC;
    channels_last costs no copy); ``C % 4 == 0``.  The result and the gradient of ``low`` are channels_last; the gradient of
    ``up1`` is the incoming gradient itself."""
    for name, t in (("up1", up1), ("low", low)):
        _on_device(t)
        if t.dim() != 4:
            raise RuntimeError("upsample2_add: %s must be [B,C,H,W], got %s" % (name, tuple(t.shape)))
        if t.dtype != torch.float32:
            raise RuntimeError("upsample2_add: %s is %s (only float32 is built)" % (name, t.dtype))
    B, C, H, W = low.shape
    if tuple(up1.shape) != (B, C, 2 * H, 2 * W):
        raise RuntimeError("upsample2_add: up1 has shape %s, expected %s for low %s"
                           % (tuple(up1.shape), (B, C, 2 * H, 2 * W), tuple(low.shape)))
    if C < 4 or C % 4:
        raise NotImplementedError("upsample2_add: C = %d is not a positive multiple of 4" % C)
    return _Upsample2AddFn.apply(up1, low)


class UpsampleAdd(nn.Module):
    """``kp_module``'s ``up2`` and ``merge`` as one layer: ``forward(up1, low)`` is ``upsample2_add(up1, low)``.  No parameters."""

    def forward(self, up1, low):
        return upsample2_add(up1, low)
