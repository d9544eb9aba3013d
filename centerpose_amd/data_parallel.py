"""``DataParallel``: data-parallel training with ONE PROCESS PER GPU (torchrun / ``distributed.init_from_env``) -- not torch's
single-process ``nn.DataParallel``, which the reference wraps ``ModelWithLoss`` in (trains/base_trainer.py:42-48), and not
``DistributedDataParallel`` either: no hooks, no buckets.  After ``backward()`` one call, ``reduce_gradients()``, packs every
gradient of the model into a flat float32 buffer with one library launch (``hip.optim.grad_pack``, scaled by 1 / world), runs
one all-reduce over that buffer and hands the gradients back as views of it.  The buffer never moves, so the device table of
``optim.Adam`` is laid out and uploaded once instead of once per step (``Adam.table_uploads``).

    torch.cuda.set_device(local_rank)                       # first: init_from_env binds RCCL to the current device
    rank, world = distributed.init_from_env()
    net = DataParallel(PoseNet(heads).to(device))          # rank 0's parameters and buffers everywhere
    opt = optim.Adam(net.parameters(), lr, max_grad_norm=100.)
    for batch in loader:                                    # the GLOBAL batch, the same on every rank
        mine = distributed.shard_batch(batch, rank, world)
        loss, stats = criterion(net(mine["input"]), mine)   # the mean over this rank's images
        opt.zero_grad(set_to_none=True)
        loss.backward()
        net.reduce_gradients()
        opt.step()
        stats = net.reduce_stats(stats)                     # means over the ranks (the reference: loss_stats[l].mean())
    net.sync_buffers()                                      # before evaluating or saving
    torch.save(net.module.state_dict(), path)

What the reduced gradient is: the mean over the ranks of each rank's own mean-loss gradient, the reference's ``loss.mean()``
over the replicas (base_trainer.py:89), for uneven shards too (a rank with fewer images weighs as much as the others).

Gradient accumulation needs no code: call ``backward()`` for every micro-batch and ``reduce_gradients()`` after the last one
only; autograd has summed the micro-batches in ``.grad`` by then.

Which parameters have a gradient must be the same on every rank.  It is a property of the graph (``PoseNet``'s unused
``project`` parameters have none anywhere); ``active_sets_differ`` says whether the last call saw it broken, and the first call
checks it on the host and raises.

BatchNorm: by default every rank normalises with the statistics of its own shard, and between two ``sync_buffers()`` calls
each rank's running statistics are its own; ``sync_buffers()`` gives everyone rank 0's, which is what survives in the
reference, where only replica 0's buffers are kept.  ``DataParallel(net, sync_batchnorm=True)`` re-classes the network's
BatchNorm layers to ``sync_norm.SyncBatchNorm`` (``use_hip_sync_norms``): the statistics are the global batch's, the reduced
gradient is that of the mean of the rank losses on the concatenated batch whatever the number of ranks, and the running
statistics are identical on every rank with no ``sync_buffers()``.  The price is two small all-gathers per BatchNorm layer
and step; every rank's shard must then hold at least one image.
"""
import torch
import torch.distributed as dist
from torch import nn

from . import distributed as cpd
from . import hip
from .optim import _check_params, _same_layout
from .sync_norm import use_hip_sync_norms


class _Runtime(object):
    """What reduce_gradients keeps between calls: the host arrays the pack table is built from, the device table and the
    pinned buffers it is uploaded from (the pattern of optim._Group)."""

    def __init__(self, arrays, device):
        self.arrays = arrays
        self.table_bytes, self.n_chunks = hip.optim.grad_pack_table_bytes(arrays)
        self.table = torch.empty(self.table_bytes, dtype=torch.uint8, device=device)
        self.src = [None] * arrays.n   # None: never set (0 is "no gradient")
        self.pinned = []               # [buffer, event of its last upload]
        self.uploads = 0

    def upload(self):
        for slot in self.pinned:
            if slot[1].query():
                break
        else:
            slot = [torch.empty(self.table_bytes, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
            self.pinned.append(slot)
        hip.optim.grad_pack_table_build(slot[0], self.arrays)
        self.table.copy_(slot[0], non_blocking=True)
        slot[1].record()
        self.uploads += 1


class DataParallel(nn.Module):
    """``DataParallel(module, group=None, stage_on_host=None, sync_batchnorm=False)``: ``module`` on this process's GPU, one
    process per GPU (see the module text; this is NOT torch's single-process ``nn.DataParallel``).  ``.module`` is the network (what ``state_dict`` consumers such as
    the reference's ``save_model`` look for), ``forward`` delegates to it.  Construction broadcasts rank 0's parameters and
    buffers (two coalesced broadcasts: the float tensors, the integer ones) and allocates the zeroed flat gradient buffer on
    the module's device.  Every parameter must be float32, strided and dense, by ``optim.Adam``'s rule.

    ``stage_on_host``: None (default) hands the device buffer to the backend and falls back to staging through one pinned
    host buffer if the backend refuses device tensors; True stages from the first call.  ``comm_path`` says which ran:
    "device", "pinned host" or "none" (world size 1 or no process group: no collective).  Staging is the one path that
    waits for the device.

    ``sync_batchnorm=True`` first re-classes the module's BatchNorm layers to ``sync_norm.SyncBatchNorm`` over ``group``
    (``sync_norm.use_hip_sync_norms``; what it returned is kept as ``sync_batchnorm_converted`` / ``sync_batchnorm_skipped``).
    The default leaves the module as it is.

    ``layout_copies`` counts the gradients that had to be copied into their parameter's memory layout; ``pack_table_uploads``
    the uploads of the pack table (one per call whose gradient addresses changed: a few KB)."""

    def __init__(self, module, group=None, stage_on_host=None, sync_batchnorm=False):
        super().__init__()
        self.module = module
        self.group = group
        self.sync_batchnorm_converted, self.sync_batchnorm_skipped = use_hip_sync_norms(module, group) if sync_batchnorm else ([], {})
        named = list(module.named_parameters())
        if not named:
            raise ValueError("DataParallel: the module has no parameters")
        self._names = [k for k, _ in named]
        self._params = [p for _, p in named]
        _check_params(self._params)
        dev = self._params[0].device
        if any(p.device != dev for p in self._params):
            raise NotImplementedError("DataParallel: the parameters must live on one device (one process per GPU)")
        self.device = dev
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self._lengths = [p.numel() for p in self._params]
        self._offsets, self.flat_elems = hip.optim.grad_flat_layout(self._lengths)
        self.flat = torch.zeros(self.flat_elems, dtype=torch.float32, device=dev)
        n = len(self._params)
        self._counts = self.flat[self._offsets[n]:self._offsets[n] + n]   # the flags; after the all-reduce: ranks with a gradient
        self._views = [None] * n
        self._rt = None
        self._stage = bool(stage_on_host) if stage_on_host is not None else None
        self._host = None
        self._checked = False
        self.comm_path = "none"
        self.layout_copies = 0
        self.active_sets_differ = torch.zeros((), dtype=torch.bool, device=dev)
        if self.world > 1:
            cpd.broadcast_coalesced(self._params + list(module.buffers()), 0, group)

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    @property
    def pack_table_uploads(self):
        return self._rt.uploads if self._rt is not None else 0

    def _view(self, i):
        p, v = self._params[i], self._views[i]
        if v is None or v.stride() != p.stride() or v.shape != p.shape:   # created once; again only if the parameter's layout moved
            v = self._views[i] = self.flat.as_strided(p.shape, p.stride(), self._offsets[i])
        return v

    def _all_reduce(self):
        if self._stage is not True:
            try:
                dist.all_reduce(self.flat, dist.ReduceOp.SUM, group=self.group)
                self._stage, self.comm_path = False, "device"
                return
            except RuntimeError:
                if self._stage is False:   # it has worked before: not a backend that refuses device tensors
                    raise
                self._stage = True
        if self._host is None:
            self._host = torch.empty(self.flat_elems, dtype=torch.float32, pin_memory=True)
        self._host.copy_(self.flat, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        dist.all_reduce(self._host, dist.ReduceOp.SUM, group=self.group)
        self.flat.copy_(self._host, non_blocking=True)
        self.comm_path = "pinned host"

    @torch.no_grad()
    def reduce_gradients(self):
        """Call after ``backward()``: pack (x 1 / world), one all-reduce (SUM), and ``p.grad`` of every parameter that had a
        gradient becomes its view of the flat buffer (the parameter's shape and strides; the same tensor object every call).
        A parameter without a gradient keeps ``grad = None``.  Queues everything on the current stream and waits for
        nothing (but see ``stage_on_host``); the first call alone reads ``active_sets_differ`` on the host and raises
        RuntimeError if the ranks disagree about which parameters have a gradient."""
        if not self.flat.is_cuda:
            raise RuntimeError("centerpose_amd.data_parallel.DataParallel: parameters must live on the HIP device (no CPU path)")
        if self._params[0].device != self.device:
            raise RuntimeError("DataParallel: the module has moved to %s since it was wrapped on %s: move it first, wrap it then"
                               % (self._params[0].device, self.device))
        if self._rt is None:
            self._rt = _Runtime(hip.optim.GradPackArrays(self._lengths), self.device)
        rt = self._rt
        flat_ptr = self.flat.data_ptr()
        keep, dirty = [], False   # gradients copied into their parameter's layout live until the launch is queued
        for i, p in enumerate(self._params):
            g = p.grad
            if g is None:
                ptr = 0
            else:
                if g.dtype != torch.float32:
                    raise NotImplementedError("centerpose_amd.optim.Adam: float32 gradients only (got %s)" % g.dtype)
                if g.layout != torch.strided:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                if g.stride() != p.stride() and not _same_layout(g, p):
                    c = torch.empty_like(p, memory_format=torch.preserve_format)
                    c.copy_(g)
                    g = c
                    keep.append(c)
                    self.layout_copies += 1
                # an empty gradient has no address of its own: its (empty) place in the buffer stands for "has a gradient"
                ptr = g.data_ptr() if g.numel() else flat_ptr + 4 * self._offsets[i]
            if ptr != rt.src[i]:
                rt.src[i], rt.arrays.src[i], dirty = ptr, ptr or None, True
        with torch.cuda.device(self.device):
            if dirty:
                rt.upload()
            hip.optim.grad_pack(rt.table, rt.arrays.n, rt.n_chunks, self.flat, 1.0 / self.world, self.flat_elems)
            if self.world > 1:
                self._all_reduce()
        for i, p in enumerate(self._params):
            if p.grad is not None:
                p.grad = self._view(i)
        c = self._counts
        self.active_sets_differ = ((c != 0) & (c != self.world)).any()
        if not self._checked:
            self._checked = True
            if bool(self.active_sets_differ):
                counts = c.cpu().tolist()
                bad = ["%s (on %d of %d ranks)" % (self._names[i], int(k), self.world) for i, k in enumerate(counts) if k not in (0, self.world)]
                raise RuntimeError("DataParallel: the ranks disagree about which parameters have a gradient: %s%s"
                                   % (", ".join(bad[:5]), " and %d more" % (len(bad) - 5) if len(bad) > 5 else ""))

    def sync_buffers(self, src=0):
        """Every rank gets rank ``src``'s buffers (BatchNorm running statistics, ``num_batches_tracked``): one coalesced
        broadcast per dtype.  Call it before evaluating or saving."""
        if self.world > 1:
            cpd.broadcast_coalesced(list(self.module.buffers()), src, self.group)

    def reduce_stats(self, stats):
        """``{name: scalar}`` (0-dim tensors or numbers, e.g. the loss terms) -> ``{name: mean over the ranks}`` as 0-dim
        float32 tensors on the module's device, with one all-reduce of the packed vector.  The names must be the same, in
        the same order, on every rank."""
        keys = list(stats)
        if not keys:
            return {}
        vec = torch.stack([torch.as_tensor(stats[k], dtype=torch.float32, device=self.device).detach().reshape(()) for k in keys])
        if self.world > 1:
            cpd.all_reduce_sum(vec, self.group)
            vec = vec / self.world
        return dict(zip(keys, vec.unbind(0)))
