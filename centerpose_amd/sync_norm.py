"""SyncBatchNorm on the library's kernels: ``norm.BatchNorm2d`` whose training statistics are those of the GLOBAL batch of a
process group (one process per GPU, the batch sharded by images): ``sync_batch_norm``, ``SyncBatchNorm`` and
``use_hip_sync_norms``.  The sibling of ``norm.py``; ``data_parallel.DataParallel(sync_batchnorm=True)`` converts a network.

What it guarantees:

* the statistics are the global batch's: every rank normalises with the same ``mean`` / ``invstd``, bit for bit, and every
  rank's running statistics stay identical with no ``sync_buffers()`` (the variance unbiased by the global n / (n - 1));
* the gradients are those of the mean of the rank losses: with ``L_r`` each rank's loss on its own shard, ``grad_x`` is the
  gradient of ``sum_r L_r`` through the shared statistics, and ``weight.grad`` / ``bias.grad`` are LOCAL sums, which
  ``DataParallel.reduce_gradients()`` averages like every other parameter gradient -- the convention of ``nn.SyncBatchNorm``
  under DDP.  After the reduction every parameter gradient is that of ``(1 / world) sum_r L_r`` on the concatenated batch
  with BatchNorm over all of it, whatever the number of ranks;
* float32, no atomics, no backend SUM (two all-gathers per layer and step; the ranks are merged in rank order on the device,
  a rank being one more level of the Chan merge that already merges a tensor's slabs): bitwise reproducible, and at world
  size 1 bitwise ``norm.batch_norm``.

Every rank must hold at least one image (``input.shape[0] >= 1``): a global batch must give every rank a shard.  Nothing
here reads a device value on the host; the global count stays on the device between the forward and the backward.
"""
import torch.distributed as dist
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import distributed as cpd
from . import hip as _hip
from ._layers import _nhwc, _reclass
from .norm import BatchNorm2d, _bookkeeping, _check_args, _refusal, batch_norm


class _SyncBatchNormFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, momentum, eps, relu, group):
        xh = _nhwc(x)
        records = cpd.all_gather_flat(_hip.sync_norm.stats(xh), group)
        y, mean, invstd, count = _hip.sync_norm.forward(xh, records, weight, bias, None if residual is None else _nhwc(residual),
                                                        running_mean, running_var, momentum, eps, act=1 if relu else 0)
        ctx.relu, ctx.affine, ctx.group = relu, weight is not None, group
        ctx.save_for_backward(*((x, mean, invstd, count) + ((weight,) if ctx.affine else ()) + ((y,) if relu else ())))
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, mean, invstd, count = ctx.saved_tensors[:4]
        weight = ctx.saved_tensors[4] if ctx.affine else None
        y = ctx.saved_tensors[-1] if ctx.relu else None
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        if not (need_x or need_w or need_b or need_r):
            return (None,) * 10
        # (the collective below is entered whenever the function is in the graph: which inputs need a gradient is a
        # property of the graph, the same on every rank)
        xh, gh = _nhwc(x), _nhwc(grad_out)
        sums, gw, gb = _hip.sync_norm.backward_reduce(xh, gh, mean, invstd, y=y, need_gamma_grad=need_w, need_beta_grad=need_b)
        gx = gr = None
        if need_x:
            sums_all = cpd.all_gather_flat(sums, ctx.group)
            gx, gr = _hip.sync_norm.backward_apply(xh, gh, mean, invstd, count, sums_all, gamma=weight, y=y, need_x_grad=True,
                                                   need_residual_grad=need_r)
        elif need_r:
            gr = _hip.sync_norm.backward_apply(xh, gh, mean, invstd, count, sums.unsqueeze(0), gamma=weight, y=y, need_x_grad=False,
                                               need_residual_grad=True)[1]
        return (gx.permute(0, 3, 1, 2) if need_x else None, gw, gb, gr.permute(0, 3, 1, 2) if need_r else None) + (None,) * 6


def sync_batch_norm(x, weight, bias, running_mean, running_var, training, momentum, eps, residual=None, relu=False, group=None):
    """``norm.batch_norm`` with the statistics of the global batch over ``group`` (None: the default process group).  In
    evaluation, without an initialised process group and at world size 1 it IS ``norm.batch_norm``; otherwise every rank of
    the group must call it, in the same order, each with at least one image."""
    if not training or not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return batch_norm(x, weight, bias, running_mean, running_var, training, momentum, eps, residual, relu)
    _check_args("sync_batch_norm", x, weight, bias, running_mean, running_var, residual)
    if x.shape[0] == 0:
        raise RuntimeError("sync_batch_norm: this rank has no image (a global batch must give every rank at least one)")
    return _SyncBatchNormFn.apply(x, weight, bias, residual, running_mean, running_var, float(momentum), float(eps), bool(relu), group)


class SyncBatchNorm(BatchNorm2d):
    """``norm.BatchNorm2d`` (same constructor, parameters, buffers, ``state_dict``, ``relu`` and ``forward(input, residual)``)
    that normalises with the global batch's statistics over ``process_group`` (None: the default group) while training.  In
    ``eval()``, without an initialised process group and at world size 1 it takes ``BatchNorm2d``'s path unchanged.  An input
    without images raises before any collective: a global batch must give every rank at least one image."""
    process_group = None

    def forward(self, input, residual=None):
        self._check_input_dim(input)
        if input.shape[0] == 0:
            raise RuntimeError("SyncBatchNorm: this rank has no image (a global batch must give every rank at least one)")
        return sync_batch_norm(input, self.weight, self.bias, *_bookkeeping(self), self.eps, residual, self.relu, self.process_group)


def use_hip_sync_norms(module, group=None):
    """``norm.use_hip_norms`` for data-parallel training: re-class every ``norm.BatchNorm2d`` and every eligible plain
    ``nn.BatchNorm2d`` or ``nn.SyncBatchNorm`` under ``module`` (itself included) to ``SyncBatchNorm`` in place, over
    ``group`` (None: the default group; an ``nn.SyncBatchNorm`` then keeps its own ``process_group``).  The Parameter and buffer
    objects, the module names and the state-dict keys stay as they are.  Returns ``(converted, skipped)``: the converted
    modules' names and ``{name: reason}`` for the layers left alone (``num_features % 4``, a dtype other than float32,
    user-derived subclasses).  Modules that already are ``SyncBatchNorm`` appear in neither (their group is left alone), and
    no other kind of module is mentioned or touched."""
    def regroup(m):   # (a layer's own ``relu = True`` is an instance attribute and stays)
        own = m.__dict__.pop("process_group", None)   # (nn.SyncBatchNorm's instance attribute)
        m.process_group = group if group is not None else own

    return _reclass(module, (BatchNorm2d, nn.BatchNorm2d, nn.SyncBatchNorm), SyncBatchNorm, _refusal, converted_hook=regroup)
