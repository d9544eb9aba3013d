"""``Adam``: the update of the reference's training step (trains/base_trainer.py:91-99: ``clip_grad_norm_(model.parameters(),
100.); optimizer.step()`` with test.py:41's ``torch.optim.Adam(model.parameters(), opt.lr)``) as one library call per param
group -- ``hip.optim.adam_step``: at most three launches whatever the number of tensors, no host synchronisation, bitwise
reproducible.  A ``torch.optim.Optimizer`` whose ``state_dict`` is interchangeable with ``torch.optim.Adam``'s.

What differs from ``clip_grad_norm_`` + ``torch.optim.Adam``, all of it on purpose:
  * ``.grad`` is left UNSCALED: the clip coefficient is applied while the gradient is read, and nothing writes it back;
  * clipping is per param group (the reference has one group: that is ``clip_grad_norm_`` over ``model.parameters()``);
  * ``step`` of a parameter's state is a float32 device scalar (as with torch's ``fused=True``), a view of the group's state
    block while the optimizer lives and a tensor of its own in ``state_dict()``.
"""
import torch

from . import hip

_TORCH_DEFAULTS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                       decoupled_weight_decay=False)
_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")


def _dense(t):
    """The tensor covers ``numel`` consecutive elements from its first (contiguous in some order of its dimensions)."""
    expect = 1
    for stride, size in sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz > 1):
        if stride != expect:
            return t.numel() == 0
        expect *= size
    return True


def _same_layout(g, p):
    return all(a == b for a, b, size in zip(g.stride(), p.stride(), p.shape) if size > 1)


def _check_params(params):
    """Adam's rule for what it updates (data_parallel.DataParallel packs the same tensors): float32, strided, dense."""
    for p in params:
        if p.dtype != torch.float32 or p.layout != torch.strided:
            raise NotImplementedError("centerpose_amd.optim.Adam: float32 strided parameters only (got %s, %s)" % (p.dtype, p.layout))
        if not _dense(p):
            raise NotImplementedError("centerpose_amd.optim.Adam: a parameter that is a non-dense view (shape %s, strides %s) "
                                      "is not implemented" % (tuple(p.shape), p.stride()))


class _Group(object):
    """What one param group keeps between steps, none of it part of ``state_dict``: the host arrays the table is built from,
    the device table, state block and workspace, and the pinned buffers the table is uploaded from."""

    def __init__(self, params, owner):
        n = len(params)
        self.owner = owner   # the optimizer, whose table_uploads counts the uploads of all its groups
        dev = params[0].device
        if any(p.device != dev for p in params):   # one table, one state block, one launch set: one device
            raise NotImplementedError("centerpose_amd.optim.Adam: the parameters of a param group must live on one device "
                                      "(%s and others here): give every device a group of its own" % dev)
        self.n, self.device = n, dev
        self.arrays = hip.optim.AdamArrays(n)
        self.p_ptr, self.g_ptr, self.p_stride, self.has_state = [None] * n, [0] * n, [None] * n, [False] * n
        for i, p in enumerate(params):
            self.arrays.lengths[i] = p.numel()
            self.arrays.active[i] = 1
        self.table_bytes, max_chunks = hip.optim.adam_table_bytes(self.arrays)   # every tensor active: the largest table
        for i in range(n):
            self.arrays.active[i] = 0
        self.table = torch.empty(self.table_bytes, dtype=torch.uint8, device=dev)
        self.block = torch.zeros(hip.optim.adam_state_bytes(n), dtype=torch.uint8, device=dev)
        self.workspace = torch.empty(hip.optim.adam_workspace_bytes(max_chunks), dtype=torch.uint8, device=dev)
        o = hip.optim.ADAM_STATE_STEPS
        self.steps = self.block[o:o + 4 * n].view(torch.float32)
        self.norm = self.block[hip.optim.ADAM_STATE_NORM:hip.optim.ADAM_STATE_NORM + 4].view(torch.float32)[0]
        self.skipped = self.block[hip.optim.ADAM_STATE_SKIPPED:hip.optim.ADAM_STATE_SKIPPED + 1].view(torch.bool)[0]
        self.pinned = []   # [buffer, event of its last upload]
        self.n_chunks = 0
        self.dirty = True

    def upload(self):
        """Lay the table out in a pinned buffer no upload is still reading and copy it to the device, asynchronously."""
        for slot in self.pinned:
            if slot[1].query():
                break
        else:
            slot = [torch.empty(self.table_bytes, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
            self.pinned.append(slot)
        self.n_chunks = hip.optim.adam_table_build(slot[0], self.arrays)
        self.table.copy_(slot[0], non_blocking=True)
        slot[1].record()
        self.dirty = False
        self.owner._table_uploads += 1


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (amsgrad=False, maximize=False) with the gradient-norm clipping of ``clip_grad_norm_`` folded in.

    ``max_grad_norm``: clip the group's gradients to this total 2-norm (None or 0: no clipping); ``skip_nonfinite``: a step
    whose gradient norm is inf or NaN changes nothing -- no parameter, no state, no step count -- and raises
    ``last_step_skipped``; by default such a step goes through the arithmetic as it does in torch.  Both are group keys, as
    ``lr`` is: each is read from the group at every step, so ``for g in opt.param_groups: g['lr'] = lr`` works as ever.

    ``last_grad_norm`` (0-dim float32) and ``last_step_skipped`` (0-dim bool) are device tensors, views of the state block
    the step writes: reading them on the host is the caller's synchronisation, ``step()`` itself never waits for the device.
    ``last_grad_norm`` is NaN after a step that did not measure it (no clipping and no ``skip_nonfinite``).  With more than
    one group they hold one value per group.  ``layout_copies`` counts the gradients that had to be copied into their
    parameter's memory layout before a step, ``table_uploads`` (read-only) the uploads of a group's device table.

    Streams and devices.  ``step()`` queues everything on the stream that is current when it is called, in order: the upload
    of the group's one device table, then the launches that read it.  Call every ``step()`` of an optimizer on the same
    stream (or order the streams yourself): a step on another stream could overwrite the table under the launches of the one
    before.  The parameters of a group live on one device (refused otherwise); groups may sit on different devices."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None, skip_nonfinite=False,
                 **torch_options):
        for k in torch_options:
            if k not in _TORCH_DEFAULTS:
                raise TypeError("Adam: unexpected argument %r" % k)
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("centerpose_amd.optim.Adam: a tensor lr is not supported (pass a float)")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: %r" % (betas[0],))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: %r" % (betas[1],))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if max_grad_norm is not None and not 0.0 <= max_grad_norm:
            raise ValueError("Invalid max_grad_norm value: %r" % (max_grad_norm,))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        defaults.update(_TORCH_DEFAULTS)
        defaults.update(torch_options)
        defaults.update(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        self._groups = None
        self.layout_copies = 0
        self._table_uploads = 0
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_group(group)

    @staticmethod
    def _check_options(group):
        for k in _REFUSED:
            if group.get(k):
                raise NotImplementedError("centerpose_amd.optim.Adam: %s=True is not implemented" % k)
        if isinstance(group["lr"], torch.Tensor):
            raise NotImplementedError("centerpose_amd.optim.Adam: a tensor lr is not supported (pass a float)")

    @classmethod
    def _check_group(cls, group):
        cls._check_options(group)
        _check_params(group["params"])

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:   # a checkpoint of torch.optim.Adam has none of this class's keys, an old one not all of torch's
            for k, v in self.defaults.items():
                group.setdefault(k, v)
            self._check_group(group)
        self._groups = None   # the step counters go back into state blocks at the next step
        self.__dict__.setdefault("layout_copies", 0)   # (unpickling restores defaults, state and param_groups alone)
        self.__dict__.setdefault("_table_uploads", 0)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._groups = None

    def state_dict(self):
        """``torch.optim.Adam``'s: ``state[i]`` = {step, exp_avg, exp_avg_sq} for every parameter that has taken a step,
        ``param_groups`` with torch's keys plus ``max_grad_norm`` / ``skip_nonfinite``.  ``step`` is a copy (a float32 scalar
        on the parameter's device; no synchronisation), not the view into the state block the live state holds."""
        sd = super().state_dict()
        sd["state"] = {k: dict(st, step=st["step"].clone()) if isinstance(st.get("step"), torch.Tensor) else st
                       for k, st in sd["state"].items()}   # new dicts: super() packs the live ones
        return sd

    def _runtime(self):
        """The _Group of every param group, (re)built after construction, load_state_dict and add_param_group: the step
        counts of the states move into the new state blocks, and the states hold views of them from then on."""
        if self._groups is not None:
            return self._groups
        groups = []
        for group in self.param_groups:
            params = group["params"]
            if not params:
                groups.append(None)
                continue
            for p in params:
                if not p.is_cuda:
                    raise RuntimeError("centerpose_amd.optim.Adam: parameters must live on the HIP device (no CPU path)")
            rt = _Group(params, self)
            host = torch.zeros(rt.n, dtype=torch.float32)
            on_host = False
            for i, p in enumerate(params):
                st = self.state.get(p)
                if not st:
                    continue
                step = st["step"]
                if isinstance(step, torch.Tensor) and step.is_cuda:
                    rt.steps[i].copy_(step.reshape(()))
                else:
                    host[i] = float(step)
                    on_host = True
                st["step"] = rt.steps[i]
                for k in ("exp_avg", "exp_avg_sq"):   # a loaded state has the checkpoint's layout
                    if not _same_layout(st[k], p) or st[k].dtype != torch.float32:
                        t = torch.empty_like(p, memory_format=torch.preserve_format)
                        t.copy_(st[k])
                        st[k] = t
                rt.arrays.m[i], rt.arrays.v[i] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                rt.has_state[i] = True
            if on_host:   # counts that came from the host (a torch.optim.Adam checkpoint) are added to the zeros in their places
                rt.steps.add_(host.to(rt.steps.device))
            groups.append(rt)
        self._groups = groups
        return groups

    @property
    def table_uploads(self):
        """How many times a group's device table was laid out and uploaded since construction: once per step while the
        gradients are fresh allocations, once in all while their addresses stay put (``data_parallel.DataParallel``'s views
        of its flat buffer)."""
        return self._table_uploads

    @property
    def last_grad_norm(self):
        if self._groups is None:
            return None
        groups = [g for g in self._groups if g is not None]
        return groups[0].norm if len(groups) == 1 else torch.stack([g.norm for g in groups])

    @property
    def last_step_skipped(self):
        if self._groups is None:
            return None
        groups = [g for g in self._groups if g is not None]
        return groups[0].skipped if len(groups) == 1 else torch.stack([g.skipped for g in groups])

    @torch.no_grad()
    def step(self, closure=None):
        """One clip + Adam update of every parameter that has a ``.grad``; the others, their state and their step count
        do not move.  One ``hip.optim.adam_step`` call per param group, no host synchronisation.  Returns None (the
        closure's loss where one is given, as every torch optimizer)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group, rt in zip(self.param_groups, self._runtime()):
            if rt is None:
                continue
            self._check_options(group)
            a = rt.arrays
            keep = []   # gradients copied into their parameter's layout live until the launch is queued
            n_active = 0
            for i, p in enumerate(group["params"]):
                g = grad = p.grad
                if g is None:
                    if a.active[i]:
                        a.active[i], rt.g_ptr[i], rt.dirty = 0, 0, True
                    continue
                n_active += 1
                pp = p.data_ptr()
                if pp != rt.p_ptr[i]:   # first step, or the parameter's memory was replaced (.to(), .data = ...)
                    if not p.is_cuda:
                        raise RuntimeError("centerpose_amd.optim.Adam: parameters must live on the HIP device (no CPU path)")
                    if not _dense(p):
                        raise NotImplementedError("centerpose_amd.optim.Adam: a parameter that is a non-dense view is not implemented")
                    rt.p_ptr[i], rt.p_stride[i], a.p[i], rt.dirty = pp, p.stride(), pp, True
                if g.dtype != torch.float32:
                    raise NotImplementedError("centerpose_amd.optim.Adam: float32 gradients only (got %s)" % g.dtype)
                if g.layout != torch.strided:
                    if g.is_sparse:
                        raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                    g = g.to_dense()
                if g.stride() != rt.p_stride[i] and not _same_layout(g, p):
                    c = torch.empty_like(p, memory_format=torch.preserve_format)
                    c.copy_(g)
                    g = c
                    self.layout_copies += 1
                if g is not grad:
                    keep.append(g)
                if not rt.has_state[i]:
                    st = self.state[p]
                    st["step"] = rt.steps[i]
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    a.m[i], a.v[i], rt.has_state[i], rt.dirty = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), True, True
                gp = g.data_ptr()
                if gp != rt.g_ptr[i] or not a.active[i]:
                    a.active[i], rt.g_ptr[i], a.g[i], rt.dirty = 1, gp, gp, True
            if n_active == 0:
                continue
            with torch.cuda.device(rt.device):   # the current stream of the group's device
                if rt.dirty:
                    rt.upload()
                hip.optim.adam_step(rt.table, rt.n, rt.n_chunks, rt.block, group["lr"], group["betas"][0], group["betas"][1],
                                    group["eps"], group["weight_decay"], group["max_grad_norm"], group["skip_nonfinite"], rt.workspace)
        return loss
