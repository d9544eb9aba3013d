"""SyncBatchNorm's four device phases (cp_batchnorm_sync_*, csrc/batchnorm.hip): the training BatchNorm of ``ops.py`` with the
statistics of a process group's global batch.  The library holds no communicator: ``stats`` -> all-gather the records ->
``forward``; ``backward_reduce`` -> all-gather the sums -> ``backward_apply``.  The autograd function and the module on top of
these calls are ``centerpose_amd.sync_norm``'s.  Reached as ``hip.sync_norm.NAME``."""
import torch

from . import _abi
from .ops import _bn_vec, _norm_ws


def record_floats(C):
    """Floats of one rank's record ``mean[C] | M2[C] | count`` (cp_batchnorm_sync_record_floats): 2 C + 4, the count an int32
    bit pattern in the first word of the last 16-byte slot."""
    n = int(_abi.lib().cp_batchnorm_sync_record_floats(int(C)))
    if n == 0:
        _abi._refuse("sync_batch_norm")
    return n


def _ws(x):
    return _norm_ws("sync_batch_norm", _abi.lib().cp_batchnorm_workspace_bytes, x)


def _flat(t, n, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
        raise RuntimeError("sync_batch_norm: %s must be a contiguous float32 tensor of %d elements on the HIP device" % (name, n))
    return t


def stats(x, record=None):
    """Forward, phase A (cp_batchnorm_sync_stats_nhwc): x [B,H,W,C] NHWC -> this rank's record [record_floats(C)] (written
    into ``record`` when given)."""
    geo, ws = _ws(x)
    x = _abi._dev(x)
    n = record_floats(geo[3])
    record = torch.empty(n, device=x.device, dtype=torch.float32) if record is None else _flat(record, n, "record")
    rc = _abi.lib().cp_batchnorm_sync_stats_nhwc(_abi._stream(), *_abi._ptrs(x, record), *geo, _abi._ptr(ws), ws.numel())
    _abi._check(rc, "cp_batchnorm_sync_stats_nhwc")
    return record


def forward(x, records, gamma=None, beta=None, residual=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, act=0):
    """Forward, phase B (cp_batchnorm_sync_forward_nhwc): ``records`` [world, record_floats(C)] in rank order (the all-gather
    of ``stats``' results) -> (y [B,H,W,C], save_mean [C], save_invstd [C], save_count [1]): the global statistics, the same
    bits on every rank; running_mean / running_var, when given, are updated IN PLACE with them.  ``save_count`` is the global
    count of values per channel as a float on the device, for ``backward_apply``."""
    L = _abi.lib()
    geo, ws = _ws(x)
    x = _abi._dev(x)
    C = geo[3]
    if records.dim() != 2:
        raise RuntimeError("sync_batch_norm: records must be [world, %d]" % record_floats(C))
    world = records.shape[0]
    _flat(records, world * record_floats(C), "records")
    gamma, beta = _bn_vec(gamma, C, "gamma"), _bn_vec(beta, C, "beta")
    residual = _abi._dev_opt(residual)
    _abi._check_shapes("sync_batch_norm", [("residual", residual, x.shape)])
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None:
            _flat(t, C, name)
    y = torch.empty_like(x)
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    invstd = torch.empty_like(mean)
    count = torch.empty(1, device=x.device, dtype=torch.float32)
    rc = L.cp_batchnorm_sync_forward_nhwc(_abi._stream(), *_abi._ptrs(x, gamma, beta, residual, running_mean, running_var, y, mean,
                                                                      invstd, count, records), int(world), *geo, float(momentum),
                                          float(eps), int(act), _abi._ptr(ws), ws.numel())
    _abi._check(rc, "cp_batchnorm_sync_forward_nhwc")
    return y, mean, invstd, count


def backward_reduce(x, grad_out, save_mean, save_invstd, y=None, need_gamma_grad=True, need_beta_grad=True, sums=None):
    """Backward, phase A (cp_batchnorm_sync_backward_reduce_nhwc) -> (sums [2 C], grad_gamma, grad_beta): this rank's
    ``sum g | invstd * sum g (x - mean)`` against the global statistics (g = grad_out, gated by y > 0 when ``y``, the
    activated output, is given), and the LOCAL parameter gradients (copies of the two halves), None where not asked for."""
    geo, ws = _ws(x)
    x, grad_out, y = _abi._dev(x), _abi._dev(grad_out), _abi._dev_opt(y)
    C = geo[3]
    _abi._check_shapes("sync_batch_norm_backward", (("grad_out", grad_out, x.shape), ("y", y, x.shape)))
    save_mean, save_invstd = _bn_vec(save_mean, C, "save_mean"), _bn_vec(save_invstd, C, "save_invstd")
    sums = torch.empty(2 * C, device=x.device, dtype=torch.float32) if sums is None else _flat(sums, 2 * C, "sums")
    grad_g = torch.empty(C, device=x.device, dtype=torch.float32) if need_gamma_grad else None
    grad_b = torch.empty(C, device=x.device, dtype=torch.float32) if need_beta_grad else None
    rc = _abi.lib().cp_batchnorm_sync_backward_reduce_nhwc(_abi._stream(), *_abi._ptrs(x, y, grad_out, save_mean, save_invstd, sums,
                                                                                      grad_g, grad_b), *geo, _abi._ptr(ws), ws.numel())
    _abi._check(rc, "cp_batchnorm_sync_backward_reduce_nhwc")
    return sums, grad_g, grad_b


def backward_apply(x, grad_out, save_mean, save_invstd, save_count, sums_all, gamma=None, y=None, need_x_grad=True,
                   need_residual_grad=False):
    """Backward, phase B (cp_batchnorm_sync_backward_apply_nhwc): ``sums_all`` [world, 2 C] in rank order (the all-gather of
    ``backward_reduce``'s sums), added in rank order -> (grad_x, grad_residual), None where not asked for.  Without ``y``
    grad_residual is ``grad_out`` itself, not a copy."""
    geo, ws = _ws(x)
    x, grad_out, y = _abi._dev(x), _abi._dev(grad_out), _abi._dev_opt(y)
    C = geo[3]
    _abi._check_shapes("sync_batch_norm_backward", (("grad_out", grad_out, x.shape), ("y", y, x.shape)))
    gamma, save_mean, save_invstd = _bn_vec(gamma, C, "gamma"), _bn_vec(save_mean, C, "save_mean"), _bn_vec(save_invstd, C, "save_invstd")
    if sums_all.dim() != 2:
        raise RuntimeError("sync_batch_norm: sums_all must be [world, %d]" % (2 * C))
    world = sums_all.shape[0]
    _flat(sums_all, world * 2 * C, "sums_all")
    _flat(save_count, 1, "save_count")
    grad_x = torch.empty_like(x) if need_x_grad else None
    grad_res = torch.empty_like(x) if need_residual_grad and y is not None else None
    if grad_x is not None or grad_res is not None:
        rc = _abi.lib().cp_batchnorm_sync_backward_apply_nhwc(_abi._stream(), *_abi._ptrs(x, y, grad_out, gamma, save_mean, save_invstd,
                                                                                         sums_all), int(world),
                                                              *_abi._ptrs(save_count, grad_x, grad_res), *geo, _abi._ptr(ws),
                                                              ws.numel())
        _abi._check(rc, "cp_batchnorm_sync_backward_apply_nhwc")
    if need_residual_grad and y is None:
        grad_res = grad_out
    return grad_x, grad_res
