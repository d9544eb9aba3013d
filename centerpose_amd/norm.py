"""BatchNorm2d on the library's kernels, forward and backward, fused with the residual add and the ReLU that follow it:
``batch_norm``, ``BatchNorm2d`` and ``use_hip_norms``.  The sibling of ``conv.py``.

Every convolution and every DCN of the reference's backbones is followed by a training-mode ``nn.BatchNorm2d(momentum=0.1)``,
most of those by a ReLU, and the second layer of each residual block and every ``Root`` by ``out += residual`` in between
(pose_dla_dcn.py:40-62 ``BasicBlock``, pose_dla_dcn.py:150-168 ``Root``, pose_dla_dcn.py:381 the DCN's ``actf``,
resnet_dcn.py).  ``batch_norm`` is one autograd function over ``cp_batchnorm_forward_nhwc`` (one statistics pass and one fused
apply pass) and ``cp_batchnorm_backward_nhwc`` (one reduction and one apply pass); float32, bitwise reproducible.
``BatchNorm2d`` is ``nn.BatchNorm2d`` with that forward and nothing else changed, and ``use_hip_norms(model)`` re-classes a
tree's eligible layers in place, the contract of ``conv.use_hip_convs``.

GroupNorm is ``group_norm.py``'s (``use_hip_group_norms``); ``SyncBatchNorm``, the same layer with the statistics of a process
group's global batch, is ``sync_norm.py``'s (``use_hip_sync_norms``, ``DataParallel(sync_batchnorm=True)``).  ``BatchNorm1d/3d``,
bf16 and ``num_features % 4 != 0`` are not built.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import hip as _hip
from ._layers import _nhwc, _on_device, _reclass


class _BatchNormFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, training, momentum, eps, relu):
        xh = _nhwc(x)
        y, mean, invstd = _hip.batch_norm_forward(xh, weight, bias, None if residual is None else _nhwc(residual), running_mean,
                                                  running_var, training, momentum, eps, act=1 if relu else 0)
        ctx.training, ctx.relu, ctx.affine = training, relu, weight is not None
        ctx.save_for_backward(*((x, mean, invstd) + ((weight,) if ctx.affine else ()) + ((y,) if relu else ())))
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, mean, invstd = ctx.saved_tensors[:3]
        weight = ctx.saved_tensors[3] if ctx.affine else None
        y = ctx.saved_tensors[-1] if ctx.relu else None
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        if not (need_x or need_w or need_b or need_r):
            return (None,) * 10
        gx, gr, gw, gb = _hip.batch_norm_backward(_nhwc(x), _nhwc(grad_out), mean, invstd, gamma=weight, y=y, training=ctx.training,
                                                  need_x_grad=need_x, need_residual_grad=need_r, need_gamma_grad=need_w,
                                                  need_beta_grad=need_b)
        return (gx.permute(0, 3, 1, 2) if need_x else None, gw, gb, gr.permute(0, 3, 1, 2) if need_r else None) + (None,) * 6


def _check_args(op, x, weight, bias, running_mean, running_var, residual):
    """The argument checks of ``batch_norm`` and ``sync_norm.sync_batch_norm``, under the operator's own name."""
    _on_device(x)
    if x.dim() != 4:
        raise RuntimeError("%s: x must be [B,C,H,W], got %s" % (op, tuple(x.shape)))
    for name, t in (("x", x), ("residual", residual), ("weight", weight), ("bias", bias), ("running_mean", running_mean),
                    ("running_var", running_var)):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("%s: %s is %s (only float32 is built)" % (op, name, t.dtype))
    if residual is not None and residual.shape != x.shape:
        raise RuntimeError("%s: residual has shape %s, expected %s" % (op, tuple(residual.shape), tuple(x.shape)))


def batch_norm(x, weight, bias, running_mean, running_var, training, momentum, eps, residual=None, relu=False):
    """``relu?(F.batch_norm(x, running_mean, running_var, weight, bias, training, momentum, eps) [+ residual])`` on the HIP kernels
    with autograd.  ``x`` and ``residual`` are logical [B,C,H,W] float32 tensors on the device, NCHW-contiguous or channels_last
    (the kernels read NHWC; channels_last costs no copy); the result and the gradients are channels_last.  ``weight`` / ``bias``
    None: 1 / 0.  ``training``: running_mean / running_var (None, or float32 device tensors) are updated in place; otherwise
    they are the statistics and must be given.  ``C % 4 == 0``."""
    _check_args("batch_norm", x, weight, bias, running_mean, running_var, residual)
    if not training and (running_mean is None or running_var is None):
        raise RuntimeError("batch_norm: evaluation needs running_mean and running_var")
    return _BatchNormFn.apply(x, weight, bias, residual, running_mean, running_var, bool(training), float(momentum), float(eps),
                              bool(relu))


def _bookkeeping(m):
    """nn.BatchNorm2d's bookkeeping for one forward of ``m`` (torch/nn/modules/batchnorm.py, _BatchNorm.forward): counts the
    batch and returns this call's ``(running_mean, running_var, training, momentum)``.  A function, not a method: the layer
    classes add nothing to ``nn.BatchNorm2d`` but ``forward`` and ``relu``."""
    factor = 0.0 if m.momentum is None else m.momentum
    if m.training and m.track_running_stats and m.num_batches_tracked is not None:
        m.num_batches_tracked.add_(1)
        if m.momentum is None:  # cumulative moving average
            factor = 1.0 / float(m.num_batches_tracked)
    training = m.training or (m.running_mean is None and m.running_var is None)
    track = not m.training or m.track_running_stats
    return m.running_mean if track else None, m.running_var if track else None, training, factor


class BatchNorm2d(nn.BatchNorm2d):
    """``nn.BatchNorm2d`` whose forward and backward run on the library (``batch_norm``).  Constructor, parameters, buffers,
    initial values, ``state_dict`` and ``repr`` are ``nn.BatchNorm2d``'s; ``forward(input, residual)`` adds ``residual`` after
    the normalisation and ``relu = True`` fuses a following ReLU into the layer."""
    relu = False

    def forward(self, input, residual=None):
        self._check_input_dim(input)
        return batch_norm(input, self.weight, self.bias, *_bookkeeping(self), self.eps, residual, self.relu)


def _refusal(m):
    """Why the library cannot run this nn.BatchNorm2d's configuration, or None."""
    if m.num_features % 4 or not 4 <= m.num_features <= 4096:
        return "num_features = %d is not a multiple of 4 in 4..4096" % m.num_features
    for t in (m.weight, m.bias, m.running_mean, m.running_var):
        if t is not None and t.dtype != torch.float32:
            return "dtype %s (only float32 is built)" % t.dtype
    return None


def use_hip_norms(module):
    """Re-class every eligible ``nn.BatchNorm2d`` under ``module`` (itself included) to ``BatchNorm2d`` in place: the Parameter and
    buffer objects, the module names and the state-dict keys stay as they are.  Returns ``(converted, skipped)``: the
    converted modules' names and ``{name: reason}`` for the BatchNorm2d layers left alone (``num_features % 4``, a dtype other
    than float32, subclasses such as ``SyncBatchNorm``-converted or user-derived ones).  Modules that already are
    ``BatchNorm2d`` appear in neither, and no other kind of module is mentioned or touched."""
    return _reclass(module, (nn.BatchNorm2d,), BatchNorm2d, _refusal, also=(nn.SyncBatchNorm,))
