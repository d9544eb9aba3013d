"""Max-pooling on the library's kernels, forward and backward: ``max_pool2d``, ``MaxPool2d`` and ``use_hip_pools``.  The sibling
of ``conv.py`` and ``norm.py``.

Every ``Tree`` of the DLA backbone with stride 2 pools its input with ``nn.MaxPool2d(2, stride=2)`` (pose_dla_dcn.py:211-224:
the pooled tensor feeds the ``project`` residual and, at a level root, the ``Root``), and ``resdcn_*`` pools after its stem with
``nn.MaxPool2d(3, stride=2, padding=1)`` (resnet_dcn.py).  ``max_pool2d`` is one autograd function over
``cp_maxpool2d_forward_nhwc`` and ``cp_maxpool2d_backward_nhwc``: it saves ``x`` only, and the backward recomputes every window's
winner with torch's tie rule (the first maximum in row-major order), so both directions are bitwise torch's.  ``MaxPool2d`` is
``nn.MaxPool2d`` with that forward and nothing else changed, and ``use_hip_pools(model)`` re-classes a tree's eligible layers in
place, the contract of ``norm.use_hip_norms``.

Other geometries, dilation, ``ceil_mode``, ``return_indices`` and ``C % 4 != 0`` are not built.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import hip as _hip
from ._layers import _nhwc, _on_device, _one, _reclass, _same

_GEOMETRIES = ((2, 2, 0), (3, 2, 1))


class _MaxPool2dFn(Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, pad):
        y = _hip.max_pool2d_forward(_nhwc(x), kernel, stride, pad)
        ctx.geo = (kernel, stride, pad)
        ctx.save_for_backward(x)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        return _hip.max_pool2d_backward(_nhwc(x), _nhwc(grad_out), *ctx.geo).permute(0, 3, 1, 2), None, None, None


def _geometry_refusal(kernel, stride, pad):
    if (kernel, stride, pad) not in _GEOMETRIES:
        return ("geometry outside the table: (kernel, stride, padding) must be (2, 2, 0) or (3, 2, 1), got (%d, %d, %d)"
                % (kernel, stride, pad))
    return None


def max_pool2d(x, kernel_size, stride=None, padding=0):
    """``F.max_pool2d(x, kernel_size, stride, padding)`` on the HIP kernels with autograd.  ``x`` is a logical [B,C,H,W] float32
    tensor on the device, NCHW-contiguous or channels_last (the kernels read NHWC; channels_last costs no copy); the result and
    the gradient are channels_last.  (kernel, stride, padding) is (2, 2, 0), which floors, or (3, 2, 1); ``C % 4 == 0``."""
    _on_device(x)
    if x.dim() != 4:
        raise RuntimeError("max_pool2d: x must be [B,C,H,W], got %s" % (tuple(x.shape),))
    if x.dtype != torch.float32:
        raise RuntimeError("max_pool2d: x is %s (only float32 is built)" % x.dtype)
    kernel = _one(kernel_size, "max_pool2d", "kernel_size")
    stride = kernel if stride is None or stride == [] or stride == () else _one(stride, "max_pool2d", "stride")
    pad = _one(padding, "max_pool2d", "padding")
    why = _geometry_refusal(kernel, stride, pad)
    if why:
        raise NotImplementedError("max_pool2d: " + why)
    return _MaxPool2dFn.apply(x, kernel, stride, pad)


def _refusal(m):
    """Why the library cannot run this nn.MaxPool2d's configuration, or None."""
    if m.dilation not in (1, (1, 1), [1, 1]):
        return "dilation %r (only 1 is built)" % (m.dilation,)
    if m.ceil_mode:
        return "ceil_mode is not built"
    if m.return_indices:
        return "return_indices is not built"
    stride = m.kernel_size if m.stride is None else m.stride
    if not (_same(m.kernel_size) and _same(stride) and _same(m.padding)):
        return "geometry outside the table: kernel / stride / padding differ between the axes"
    return _geometry_refusal(*(_one(v, "max_pool2d", "geometry") for v in (m.kernel_size, stride, m.padding)))


class MaxPool2d(nn.MaxPool2d):
    """``nn.MaxPool2d`` whose forward and backward run on the library (``max_pool2d``).  Constructor, attributes and ``repr`` are
    ``nn.MaxPool2d``'s."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        why = _refusal(self)
        if why:
            raise NotImplementedError("centerpose_amd.pool.MaxPool2d: " + why)

    def forward(self, input):
        return max_pool2d(input, self.kernel_size, self.stride, self.padding)


def use_hip_pools(module):
    """Re-class every eligible ``nn.MaxPool2d`` under ``module`` (itself included) to ``MaxPool2d`` in place: the module names and
    attributes stay as they are.  Returns ``(converted, skipped)``: the converted modules' names and ``{name: reason}`` for the
    max-pool layers left alone (``dilation != 1``, ``ceil_mode``, ``return_indices``, a geometry other than (2, 2, 0) and
    (3, 2, 1), subclasses).  Modules that already are ``MaxPool2d`` appear in neither, and no other kind of module is mentioned
    or touched."""
    return _reclass(module, (nn.MaxPool2d,), MaxPool2d, _refusal)
