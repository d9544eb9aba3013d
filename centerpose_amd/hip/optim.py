"""The optimizer step: gradient-norm clipping + Adam over all tensors of a param group (cp_adam_*, csrc/optim.hip) -- the
``clip_grad_norm_(model.parameters(), 100.); optimizer.step()`` of the reference's trains/base_trainer.py:91-99 with the
``torch.optim.Adam`` of test.py:41.  The table and state layouts are the header's (include/centerpose_hip.h); the
``torch.optim.Optimizer`` on top of these calls is ``centerpose_amd.optim.Adam``.  Below it, the gradient pack of data-parallel
training (cp_grad_*, csrc/grad_pack.hip), which ``centerpose_amd.data_parallel.DataParallel`` is built on."""
import ctypes

import torch

from . import _abi

# the header's constants
ADAM_CHUNK = 4096
ADAM_TENSOR_BYTES = 48
ADAM_CHUNK_BYTES = 16
ADAM_VEC = 1
ADAM_SKIP_NONFINITE = 1
ADAM_STATE_NORM = 0
ADAM_STATE_COEF = 4
ADAM_STATE_SKIPPED = 8
ADAM_STATE_STEPS = 16


def adam_state_bc_offset(n_tensors):
    """CP_ADAM_STATE_BC(n): byte offset of the float64 [2][n_tensors] bias corrections in the state block."""
    return 16 + (n_tensors * 4 + 7) // 8 * 8


def adam_state_bytes(n_tensors):
    return int(_abi.lib().cp_adam_state_bytes(int(n_tensors)))


def adam_workspace_bytes(n_chunks):
    return int(_abi.lib().cp_adam_workspace_bytes(int(n_chunks)))


class AdamArrays(object):
    """The host arrays cp_adam_table_build reads, allocated once for ``n`` tensors: device addresses ``p``, ``g``, ``m``,
    ``v``, element counts ``lengths`` and the 0/1 ``active`` flags, all indexable and assignable in place."""

    def __init__(self, n):
        self.n = int(n)
        self.p, self.g, self.m, self.v = [(ctypes.c_void_p * self.n)() for _ in range(4)]
        self.lengths = (ctypes.c_int64 * self.n)()
        self.active = (ctypes.c_int * self.n)()


def adam_table_bytes(arrays):
    """(bytes, n_chunks) of the table of ``arrays.lengths`` / ``arrays.active``; refused lengths raise ValueError."""
    n_chunks = ctypes.c_int(0)
    L = _abi.lib()
    nbytes = L.cp_adam_table_bytes(arrays.n, arrays.lengths, arrays.active, ctypes.byref(n_chunks))
    if nbytes == 0:
        raise ValueError("centerpose_hip: cp_adam_table_bytes: %s" % L.cp_last_error().decode())
    return int(nbytes), n_chunks.value


def adam_table_build(host_buffer, arrays):
    """cp_adam_table_build into ``host_buffer``, a contiguous CPU uint8 tensor (pinned for an asynchronous upload):
    returns n_chunks.  Refused arguments raise ValueError."""
    if host_buffer.is_cuda or host_buffer.dtype != torch.uint8 or not host_buffer.is_contiguous():
        raise ValueError("adam_table_build: the table is laid out in host memory: a contiguous CPU uint8 tensor")
    n_chunks = ctypes.c_int(0)
    rc = _abi.lib().cp_adam_table_build(ctypes.c_void_p(host_buffer.data_ptr()), host_buffer.numel(), arrays.n, arrays.p, arrays.g,
                                        arrays.m, arrays.v, arrays.lengths, arrays.active, ctypes.byref(n_chunks))
    _abi._check_args(rc, "cp_adam_table_build")
    return n_chunks.value


def adam_step(table, n_tensors, n_chunks, state, lr, beta1, beta2, eps, weight_decay, max_norm, skip_nonfinite=False, workspace=None):
    """cp_adam_step on the current stream: clip (``max_norm`` > 0; None or <= 0: off) and update every tensor of the DEVICE
    ``table`` (the uploaded bytes of ``adam_table_build``).  ``state``: the device uint8 state block of
    ``adam_state_bytes(n_tensors)`` bytes, zeroed once by the caller; it holds the step counters and, after the call,
    total_norm, the coefficient and the skipped flag.  p, exp_avg and exp_avg_sq are written, the gradients are not.
    ``workspace``: a device uint8 tensor of ``adam_workspace_bytes(n_chunks)`` or None (allocated here).  Never
    synchronises; refused arguments, a ``table`` or ``state`` too small for ``n_tensors`` / ``n_chunks`` included, raise
    ValueError before any launch.  Returns None."""
    _abi._on_device(table, state, what="adam_step")
    L = _abi.lib()
    n_tensors, n_chunks = int(n_tensors), int(n_chunks)
    # the library sees two device addresses: what they must hold is checked here, where the tensors' sizes are known
    if n_tensors >= 1 and n_chunks >= 0:
        if table.numel() * table.element_size() < n_tensors * ADAM_TENSOR_BYTES + n_chunks * ADAM_CHUNK_BYTES:
            raise ValueError("adam_step: table is smaller than %d tensor and %d chunk records" % (n_tensors, n_chunks))
        if state.numel() * state.element_size() < L.cp_adam_state_bytes(n_tensors):
            raise ValueError("adam_step: state is smaller than adam_state_bytes(%d)" % n_tensors)
    nbytes = L.cp_adam_workspace_bytes(n_chunks)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=table.device)
    _abi._on_device(workspace, what="adam_step")
    rc = L.cp_adam_step(_abi._stream(), _abi._ptr(table), n_tensors, n_chunks, float(lr), float(beta1), float(beta2), float(eps),
                        float(weight_decay), float(max_norm) if max_norm is not None else 0.0,
                        ADAM_SKIP_NONFINITE if skip_nonfinite else 0, _abi._ptr(state), _abi._ptr(workspace), workspace.numel() * workspace.element_size())
    _abi._check_args(rc, "cp_adam_step")


# ---- the gradient pack of data-parallel training (cp_grad_*, csrc/grad_pack.hip) ----
GRAD_TENSOR_BYTES = 16
GRAD_CHUNK_BYTES = 16
GRAD_VEC = 1
GRAD_ZERO = 2


def _lengths_array(lengths):
    return (ctypes.c_int64 * len(lengths))(*[int(n) for n in lengths])


def grad_flat_layout(lengths):
    """The flat gradient buffer of tensors of these element counts: ``(offsets, flat_elems)``.  ``offsets`` has one entry per
    tensor (a multiple of 4 floats each) and a last one, where the ``len(lengths)`` float flags start; ``flat_elems`` is the
    length of all of it.  The lengths alone decide it, so every rank gets the same.  Refused lengths raise ValueError."""
    L = _abi.lib()
    n = len(lengths)
    arr = _lengths_array(lengths)
    total = L.cp_grad_flat_elems(n, arr)
    if total == 0:
        raise ValueError("centerpose_hip: cp_grad_flat_elems: %s" % L.cp_last_error().decode())
    offsets = (ctypes.c_int64 * (n + 1))()
    _abi._check_args(L.cp_grad_flat_offsets(n, arr, offsets), "cp_grad_flat_offsets")
    return list(offsets), int(total)


class GradPackArrays(object):
    """The host arrays cp_grad_pack_table_build reads, allocated once for tensors of ``lengths``: the device addresses
    ``src`` (assignable in place; None / 0: the tensor has no gradient), ``lengths`` and the layout's ``offsets``."""

    def __init__(self, lengths):
        self.n = len(lengths)
        self.src = (ctypes.c_void_p * self.n)()
        self.lengths = _lengths_array(lengths)
        offsets, self.flat_elems = grad_flat_layout(lengths)
        self.offsets = (ctypes.c_int64 * (self.n + 1))(*offsets)


def grad_pack_table_bytes(arrays):
    """(bytes, n_chunks) of the pack table of ``arrays.lengths``: both depend on the lengths alone."""
    n_chunks = ctypes.c_int(0)
    L = _abi.lib()
    nbytes = L.cp_grad_pack_table_bytes(arrays.n, arrays.lengths, ctypes.byref(n_chunks))
    if nbytes == 0:
        raise ValueError("centerpose_hip: cp_grad_pack_table_bytes: %s" % L.cp_last_error().decode())
    return int(nbytes), n_chunks.value


def grad_pack_table_build(host_buffer, arrays):
    """cp_grad_pack_table_build into ``host_buffer``, a contiguous CPU uint8 tensor (pinned for an asynchronous upload):
    returns n_chunks.  Refused arguments raise ValueError."""
    if host_buffer.is_cuda or host_buffer.dtype != torch.uint8 or not host_buffer.is_contiguous():
        raise ValueError("grad_pack_table_build: the table is laid out in host memory: a contiguous CPU uint8 tensor")
    n_chunks = ctypes.c_int(0)
    rc = _abi.lib().cp_grad_pack_table_build(ctypes.c_void_p(host_buffer.data_ptr()), host_buffer.numel(), arrays.n, arrays.src,
                                             arrays.lengths, arrays.offsets, ctypes.byref(n_chunks))
    _abi._check_args(rc, "cp_grad_pack_table_build")
    return n_chunks.value


def grad_pack(table, n_tensors, n_chunks, flat, scale=1.0, flat_elems=None):
    """cp_grad_pack on the current stream, one launch: ``flat[offset_i + k] = scale * g_i[k]`` for every tensor of the DEVICE
    ``table`` (the uploaded bytes of ``grad_pack_table_build``) that has a source, zeros for the others, and the 1.0 / 0.0
    flags behind the last tensor.  ``flat``: a contiguous float32 device tensor, zeroed once by the caller (the padding
    between the tensors is never written); ``flat_elems``: the layout's length where ``flat`` is longer (nothing at or past
    it is written).  A source that is its own destination is scaled in place.  Never synchronises; refused arguments raise
    ValueError before any launch.  Returns None."""
    _abi._on_device(table, flat, what="grad_pack")
    n_tensors, n_chunks = int(n_tensors), int(n_chunks)
    if flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError("grad_pack: flat must be a contiguous float32 tensor")
    flat_elems = flat.numel() if flat_elems is None else int(flat_elems)
    if flat_elems > flat.numel():
        raise ValueError("grad_pack: flat_elems %d is more than flat holds (%d)" % (flat_elems, flat.numel()))
    if n_tensors >= 1 and n_chunks >= 0 and table.numel() * table.element_size() < (n_tensors + 1) * GRAD_TENSOR_BYTES + n_chunks * GRAD_CHUNK_BYTES:
        raise ValueError("grad_pack: table is smaller than %d tensor and %d chunk records" % (n_tensors + 1, n_chunks))
    rc = _abi.lib().cp_grad_pack(_abi._stream(), _abi._ptr(table), n_tensors, n_chunks, _abi._ptr(flat), flat_elems, float(scale))
    _abi._check_args(rc, "cp_grad_pack")
