"""GPU tests of data-parallel training (pytest -m gpu): ``hip.optim.grad_pack`` against torch, bit for bit, and
``centerpose_amd.data_parallel.DataParallel`` + ``optim.Adam`` against the same steps without the wrapper (world size 1) and
against a single-process emulation (two ranks on the one GPU of the test box over gloo; two RCCL ranks cannot share a device,
tests/test_bench_gpu.py rehearses the same way).  The RCCL run itself is a pre-flight for a box with two GPUs.

Every comparison is ``torch.equal``.  Why the two-rank run can equal the emulation bit for bit: the pack multiplies by
1 / 2, an exact power of two; the all-reduce of two ranks is one two-operand sum, which is commutative; the emulation forms
``g0 * 0.5 + g1 * 0.5`` with separate torch operations (no fused multiply-add); and Adam's vector or element path follows the
alignment of p, g, m and v, 16-byte aligned in both runs.

Children: every test that starts processes joins them under one 120 s limit, terminates what is left then, and fails at once
when a child ends with anything but exit code 0.
"""
import copy
import os
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp
from torch import nn

from centerpose_amd import hip
from centerpose_amd.conv import Conv2d
from centerpose_amd.norm import BatchNorm2d
from centerpose_amd.optim import Adam

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 3, 4, 5, 4095, 4096, 4097, 8193]
UNALIGNED, ABSENT, CHANNELS_LAST = 8, 5, 9   # the 8193 source is 4-byte aligned only, the 4095 one absent; a tenth tensor
GUARD = 64


# ---- grad_pack against torch ----

def _pack_case(device):
    """Sources of LENGTHS (one at storage offset 1, one absent) and, behind them, the channels_last [8, 4, 3, 3] gradient:
    (gradients or None, lengths)."""
    g = torch.Generator().manual_seed(23)
    grads = []
    for i, n in enumerate(LENGTHS):
        if i == ABSENT:
            grads.append(None)
        elif i == UNALIGNED:
            grads.append(torch.randn(n + 1, generator=g).to(device)[1:])
        else:
            grads.append(torch.randn(n, generator=g).to(device))
    grads.append(torch.randn(8, 4, 3, 3, generator=g).to(device).contiguous(memory_format=torch.channels_last))
    lengths = LENGTHS + [8 * 4 * 3 * 3]
    assert grads[UNALIGNED].data_ptr() % 16 == 4 and not grads[CHANNELS_LAST].is_contiguous()
    return grads, lengths


def _memory_order(t):
    """The elements of a dense tensor in the order they lie in memory."""
    return t.as_strided((t.numel(),), (1,), t.storage_offset())


def _table(arrays, device):
    nbytes, n_chunks = hip.optim.grad_pack_table_bytes(arrays)
    host = torch.empty(nbytes, dtype=torch.uint8)
    assert hip.optim.grad_pack_table_build(host, arrays) == n_chunks
    return host.to(device), n_chunks


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0], ids=["1", "0.5", "third"])
def test_grad_pack_equals_torch(device, scale):
    grads, lengths = _pack_case(device)
    n = len(lengths)
    a = hip.optim.GradPackArrays(lengths)
    for i, t in enumerate(grads):   # (the empty gradient has no address of its own: any non-null one says "has a gradient")
        a.src[i] = None if t is None else t.data_ptr() or grads[1].data_ptr()
    table, n_chunks = _table(a, device)
    offsets, total = list(a.offsets), a.flat_elems
    results = []
    for _ in range(2):
        buf = torch.zeros(total + GUARD, dtype=torch.float32, device=device)
        buf[total:] = float("nan")
        hip.optim.grad_pack(table, n, n_chunks, buf, scale, flat_elems=total)
        results.append(buf)
    buf = results[0]
    s = torch.tensor(scale, dtype=torch.float32, device=device)
    written = torch.zeros(total, dtype=torch.bool, device=device)
    for i, t in enumerate(grads):
        region = buf[offsets[i]:offsets[i] + lengths[i]]
        written[offsets[i]:offsets[i] + lengths[i]] = True
        if t is None:
            assert not bool(region.any()), i
            continue
        assert torch.equal(region, _memory_order(t) * s), (i, lengths[i])
        if scale == 1.0:
            assert torch.equal(region.view(torch.int32), _memory_order(t).view(torch.int32)), i   # a plain copy
    # the channels_last gradient lands in its parameter's layout: the view DataParallel hands back reads the same values
    t = grads[CHANNELS_LAST]
    assert torch.equal(buf.as_strided(t.shape, t.stride(), offsets[CHANNELS_LAST]), t * s)
    flags = buf[offsets[n]:offsets[n] + n]
    written[offsets[n]:offsets[n] + n] = True
    assert flags.tolist() == [0.0 if t is None else 1.0 for t in grads]
    assert int((~written).sum()) > 0 and not bool(buf[:total][~written].any())     # the padding floats are still 0
    assert bool(torch.isnan(buf[total:]).all())                                     # the guard is untouched
    assert torch.equal(results[0].view(torch.int32), results[1].view(torch.int32))  # two calls, identical bytes


def test_grad_pack_in_place(device):
    """A source that is its own destination is scaled in place; the other regions and the padding are as before."""
    lengths = [5, 8193, 4096, 3]
    a = hip.optim.GradPackArrays(lengths)
    offsets, total = list(a.offsets), a.flat_elems
    g = torch.Generator().manual_seed(29)
    buf = torch.zeros(total, dtype=torch.float32, device=device)
    others = [torch.randn(n, generator=g).to(device) for n in lengths]
    before = torch.randn(lengths[1], generator=g).to(device)
    buf[offsets[1]:offsets[1] + lengths[1]] = before
    for i, t in enumerate(others):
        a.src[i] = t.data_ptr()
    a.src[1] = buf.data_ptr() + 4 * offsets[1]
    table, n_chunks = _table(a, device)
    hip.optim.grad_pack(table, len(lengths), n_chunks, buf, 0.5)
    for i, t in enumerate(others):
        want = before * 0.5 if i == 1 else t * 0.5
        assert torch.equal(buf[offsets[i]:offsets[i] + lengths[i]], want), i
    assert not bool(buf[offsets[0] + 5:offsets[1]].any()) and buf[offsets[4]:offsets[4] + 4].tolist() == [1.0] * 4
    with pytest.raises(ValueError, match="flat_elems"):
        hip.optim.grad_pack(table, len(lengths), n_chunks, buf[:8192], 0.5)
    with pytest.raises(ValueError, match="16-byte aligned"):
        hip.optim.grad_pack(table, len(lengths), n_chunks, buf[1:], 0.5, flat_elems=total - 4)
    with pytest.raises(ValueError, match="non-finite scale"):
        hip.optim.grad_pack(table, len(lengths), n_chunks, buf, float("nan"))


# ---- the toy model ----

class Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = Conv2d(4, 16, 3, padding=1)
        self.bn = BatchNorm2d(16)
        self.bn.relu = True
        self.conv2 = Conv2d(16, 8, 1)
        self.never_used = nn.Parameter(torch.ones(5))

    def forward(self, x):
        return self.conv2(self.bn(self.conv1(x)))


MAX_NORM = 1e-3   # far below the toy's gradient norm: the clip engages at every step
LR = 0.05


def _toy(seed, device):
    torch.manual_seed(seed)
    return Toy().to(device).train()


def _toy_data(steps, batch, device):
    g = torch.Generator().manual_seed(31)
    return ([torch.randn(batch, 4, 8, 8, generator=g).to(device) for _ in range(steps)],
            [torch.randn(batch, 8, 8, 8, generator=g).to(device) for _ in range(steps)])


def _backward(net, x, lin):
    """This process's mean loss over its images, and its gradients."""
    loss = (net(x) * lin).sum() / x.shape[0]
    loss.backward()
    return loss.detach()


def _state_vector(params, opt, buffers=()):
    """Parameters, Adam moments and step counts (and float views of the buffers) as one float32 vector, for bitwise comparison."""
    parts = [p.detach().reshape(-1) for p in params]
    for p in params:
        st = opt.state.get(p, {})
        parts += [st[k].reshape(-1) for k in ("exp_avg", "exp_avg_sq", "step") if k in st]
    parts += [b.detach().reshape(-1).to(torch.float32) for b in buffers]
    return torch.cat(parts)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _plain_steps(device):
    """Two clipped Adam steps of the toy model without the wrapper: (model, optimizer)."""
    xs, lins = _toy_data(2, 2, device)
    plain = _toy(3, device)
    opt_plain = Adam(plain.parameters(), lr=LR, max_grad_norm=MAX_NORM)
    held = []   # the gradients of earlier steps stay alive, so that every step's are fresh allocations, as in a real loop
    for x, lin in zip(xs, lins):
        opt_plain.zero_grad(set_to_none=True)
        _backward(plain, x, lin)
        opt_plain.step()
        assert float(opt_plain.last_grad_norm) > 10 * MAX_NORM
        held.append([p.grad for p in plain.parameters()])
    return plain, opt_plain


def test_world1_equals_the_plain_steps(device):
    from centerpose_amd.data_parallel import DataParallel

    xs, lins = _toy_data(2, 2, device)
    plain, opt_plain = _plain_steps(device)
    net = DataParallel(_toy(3, device))
    assert net.world == 1 and net.flat.device == device and net.flat.data_ptr() % 16 == 0 and not bool(net.flat.any())
    opt = Adam(net.parameters(), lr=LR, max_grad_norm=MAX_NORM)
    views = None
    for x, lin in zip(xs, lins):
        opt.zero_grad(set_to_none=True)
        _backward(net, x, lin)
        net.reduce_gradients()
        grads = [p.grad for p in net.parameters()]
        assert views is None or all(a is b for a, b in zip(views, grads))   # created once and kept
        views = grads
        opt.step()
    assert net.comm_path == "none" and not bool(net.active_sets_differ) and net.layout_copies == 0
    lo, hi = net.flat.data_ptr(), net.flat.data_ptr() + 4 * net.flat_elems
    for (k, p), q in zip(net.module.named_parameters(), plain.parameters()):
        if k == "never_used":
            assert p.grad is None and q.grad is None and len(opt.state.get(p, {})) == 0
            continue
        assert lo <= p.grad.data_ptr() < hi and p.grad.data_ptr() % 16 == 0 and p.grad.shape == p.shape and p.grad.stride() == p.stride()
        assert torch.equal(p.grad, q.grad), k   # scale 1: the very gradient
    a = _state_vector(list(net.parameters()), opt, net.module.buffers())
    b = _state_vector(list(plain.parameters()), opt_plain, plain.buffers())
    assert _bits_equal(a, b)
    assert opt.table_uploads == 1 and opt_plain.table_uploads == 2   # the point of the views
    assert 1 <= net.pack_table_uploads <= 2   # (2 unless the allocator hands the second step's gradients the first's addresses)


def test_world1_other_ways_a_gradient_arrives(device):
    """The same two steps with a gradient in another memory layout than its parameter's (copied into it, counted) and, at the
    second step, with zero_grad(set_to_none=False): autograd then accumulates into the views, the pack finds every source at
    its own destination and scales in place (one more upload of the pack table, for the new addresses; none after that)."""
    from centerpose_amd.data_parallel import DataParallel

    xs, lins = _toy_data(2, 2, device)
    plain, opt_plain = _plain_steps(device)
    net = DataParallel(_toy(3, device))
    opt = Adam(net.parameters(), lr=LR, max_grad_norm=MAX_NORM)
    w = net.module.conv1.weight
    for step, (x, lin) in enumerate(zip(xs, lins)):
        opt.zero_grad(set_to_none=(step == 0))
        _backward(net, x, lin)
        if step == 0:
            w.grad = w.grad.contiguous(memory_format=torch.channels_last)
            assert w.grad.stride() != w.stride()
        else:
            assert all(p.grad is v for p, v in zip(net.parameters(), views) if v is not None)
        net.reduce_gradients()
        views = [p.grad for p in net.parameters()]
        opt.step()
    assert net.layout_copies == 1 and net.pack_table_uploads == 2 and opt.table_uploads == 1
    assert w.grad.stride() == w.stride() and net.module.never_used.grad is None
    for (k, p), q in zip(net.module.named_parameters(), plain.parameters()):
        assert torch.equal(p, q), k
        for name in opt.state.get(p, {}):
            assert torch.equal(opt.state[p][name], opt_plain.state[q][name]), (k, name)


# ---- two ranks ----

def _run_ranks(target, world=2, *args):
    """Start ``target(rank, world, port, queue, *args)`` once per rank and return what the ranks put on the queue, by rank."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35000 + (os.getpid() % 2000)
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + 120
    res = {}
    try:
        while len(res) < world:
            try:
                rank, out = q.get(timeout=0.5)
                res[rank] = out
            except Exception:   # queue.Empty
                bad = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not bad, "a rank ended with exit code %s" % bad
                assert time.monotonic() < deadline, "the ranks did not finish in 120 s"
        for p in procs:
            p.join(timeout=max(0.0, deadline - time.monotonic()))
            assert p.exitcode == 0, "a rank ended with exit code %s" % p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    return [res[r] for r in range(world)]


def _init(rank, world, port, backend):
    """The process group of a child; returns the device of this rank (gloo: both ranks on device 0)."""
    sys.path.insert(0, REPO)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if backend == "nccl":
        os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    from centerpose_amd import distributed as d

    device = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(device)
    assert d.init_from_env(backend) == (rank, world)
    return device


def _same_as_rank0(vec):
    """Whether this rank's ``vec`` equals rank 0's, bit for bit."""
    ref = vec.clone()
    torch.distributed.broadcast(ref, 0)
    return _bits_equal(ref, vec)


def _emulate(nets, opt, xs, lins, world, backward):
    """The single-process emulation of one step per entry of ``xs``: ``nets[r]`` stands for rank r (the same parameters, its own
    buffers), the shards' gradients are combined as g0 * 0.5 + g1 * 0.5 and ``opt`` (over nets[0]) takes a plain step."""
    from centerpose_amd import distributed as d

    assert world == 2
    for x, lin in zip(xs, lins):
        for r, net in enumerate(nets):
            net.zero_grad(set_to_none=True)
            s, e = d.shard_range(x.shape[0], r, world)
            backward(net, x[s:e], lin[s:e] if isinstance(lin, torch.Tensor) else {k: v[s:e] for k, v in lin.items()})
        for p0, p1 in zip(nets[0].parameters(), nets[1].parameters()):
            assert (p0.grad is None) == (p1.grad is None)
            if p0.grad is not None:
                a = p0.grad * 0.5
                b = p1.grad * 0.5
                p0.grad = a + b
        opt.step()
        with torch.no_grad():
            for p0, p1 in zip(nets[0].parameters(), nets[1].parameters()):
                p1.copy_(p0)


def _toy_worker(rank, world, port, q, backend, stage):
    device = _init(rank, world, port, backend)
    from centerpose_amd import distributed as d
    from centerpose_amd.data_parallel import DataParallel

    steps = 3
    xs, lins = _toy_data(steps, 4, device)
    net = DataParallel(_toy(100 + rank, device), stage_on_host=stage)   # seeded differently: the broadcast makes them rank 0's
    opt = Adam(net.parameters(), lr=LR, max_grad_norm=MAX_NORM)
    out = {"clipped": True}
    for x, lin in zip(xs, lins):
        mine = d.shard_batch({"x": x, "lin": lin}, rank, world)
        assert mine["x"].shape[0] == 2
        opt.zero_grad(set_to_none=True)
        _backward(net, mine["x"], mine["lin"])
        net.reduce_gradients()
        opt.step()
        out["clipped"] = out["clipped"] and float(opt.last_grad_norm) > 10 * MAX_NORM
    params = list(net.parameters())
    out["ranks_equal"] = _same_as_rank0(_state_vector(params, opt))
    out["comm_path"] = net.comm_path
    out["differ"] = bool(net.active_sets_differ)
    out["never_used_has_no_grad"] = net.module.never_used.grad is None
    out["table_uploads"] = opt.table_uploads
    if rank == 0:
        nets = [_toy(100, device), _toy(100, device)]
        emu = Adam(nets[0].parameters(), lr=LR, max_grad_norm=MAX_NORM)
        _emulate(nets, emu, xs, lins, world, _backward)
        out["emulation_equal"] = _bits_equal(_state_vector(params, opt, net.module.buffers()),
                                             _state_vector(list(nets[0].parameters()), emu, nets[0].buffers()))
        # where they part, if they do: the first parameter (or moment) that differs
        out["first_difference"] = next((k for (k, p), e in zip(net.module.named_parameters(), nets[0].parameters())
                                        if not torch.equal(p, e)), None)
    torch.cuda.synchronize()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
    q.put((rank, out))


def _check_toy(res, comm_path):
    print("data_parallel toy: %s" % (res,))
    for out in res:
        assert out["ranks_equal"] and out["clipped"] and not out["differ"] and out["never_used_has_no_grad"]
        assert out["comm_path"] == comm_path and out["table_uploads"] == 1
    assert res[0]["emulation_equal"], res[0]["first_difference"]


@pytest.mark.parametrize("stage", [None, True], ids=["device_tensors", "pinned_host"])
def test_two_ranks_on_one_gpu_over_gloo(device, stage):
    _check_toy(_run_ranks(_toy_worker, 2, "gloo", stage), "pinned host" if stage else "device")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="pre-flight for a multi-GPU box: needs two visible GPUs")
def test_two_gpus_over_rccl_preflight(device):
    """The first thing to run on a box with more than one GPU (the builder never had one): the toy steps with the "nccl"
    backend = RCCL, one device per rank, dmabuf IPC (HSA_ENABLE_IPC_MODE_LEGACY=0)."""
    _check_toy(_run_ranks(_toy_worker, 2, "nccl", None), "device")


# ---- PoseNet, two ranks ----

def _pose_case():
    """tests/pose_net_ref.py's case (B = 2, 3 x 64 x 96, head_conv 64) for rank 0's shard and a second draw of the same kind
    for rank 1's: (state dict, x [4,3,64,96], lin {head: [4,c,16,24]})."""
    from tests import pose_net_ref as R

    sd = R.case_state_dict(False)
    x, _, _, lin = R.case_inputs(False)
    g = torch.Generator().manual_seed(R.SEED + 1)
    x = torch.cat([x, torch.randn(x.shape, generator=g)])
    lin = {h: torch.cat([v, torch.randn(v.shape, generator=g)]) for h, v in lin.items()}
    return sd, x, lin


def _pose_backward(net, x, lin):
    z = net(x)[0]
    loss = sum((z[h] * lin[h]).sum() for h in z) / x.shape[0]
    loss.backward()
    return loss.detach()


def _pose_net(sd, device):
    from centerpose_amd import synth
    from centerpose_amd.pose_net import PoseNet
    from tests import pose_net_ref as R

    net = PoseNet(synth.HEADS_POSE, head_conv=R.HEAD_CONV, opt=None)
    net.load_state_dict(sd, strict=True)
    return net.to(device).train()


def _pose_worker(rank, world, port, q, backend):
    device = _init(rank, world, port, backend)
    from centerpose_amd import distributed as d
    from centerpose_amd.data_parallel import DataParallel
    from tests import pose_net_ref as R

    hip.set_default_precision("f32")
    hip.set_deterministic(True)
    sd, x, lin = _pose_case()
    x, lin = x.to(device), {h: v.to(device) for h, v in lin.items()}
    mine = d.shard_batch(dict(lin, x=x), rank, world)
    start = copy.deepcopy(sd)
    if rank == 1:   # rank 1 starts from other values: construction gives it rank 0's
        for k, v in start.items():
            if v.is_floating_point():
                v.mul_(0.5)
    net = DataParallel(_pose_net(start, device))
    opt = Adam(net.parameters(), lr=1.25e-4, max_grad_norm=100.0)
    opt.zero_grad(set_to_none=True)
    _pose_backward(net, mine.pop("x"), mine)
    net.reduce_gradients()
    opt.step()
    params = list(net.parameters())
    names = [k for k, _ in net.module.named_parameters()]
    out = {"ranks_equal": _same_as_rank0(_state_vector(params, opt)), "differ": bool(net.active_sets_differ),
           "comm_path": net.comm_path, "skipped": bool(opt.last_step_skipped), "grad_norm": float(opt.last_grad_norm)}
    none = [k for k, p in zip(names, params) if p.grad is None]
    out["project_has_no_grad"] = len(none) > 0 and all(R.unused(k) for k in none) and all(
        p.grad is None for k, p in zip(names, params) if R.unused(k))
    stats = torch.cat([b.detach().reshape(-1).to(torch.float32) for b in net.module.buffers()])
    out["buffers_own_before_sync"] = _same_as_rank0(stats) == (rank == 0)
    net.sync_buffers()
    out["buffers_equal_after_sync"] = _same_as_rank0(torch.cat([b.detach().reshape(-1).to(torch.float32) for b in net.module.buffers()]))
    if rank == 0:
        nets = [_pose_net(sd, device), _pose_net(sd, device)]
        emu = Adam(nets[0].parameters(), lr=1.25e-4, max_grad_norm=100.0)
        _emulate(nets, emu, [x], [lin], world, _pose_backward)
        out["emulation_equal"] = _bits_equal(_state_vector(params, opt, net.module.buffers()),
                                             _state_vector(list(nets[0].parameters()), emu, nets[0].buffers()))
        out["first_difference"] = next((k for k, p, e in zip(names, params, nets[0].parameters()) if not torch.equal(p, e)), None)
    torch.cuda.synchronize()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
    q.put((rank, out))


def test_pose_net_two_ranks(device):
    res = _run_ranks(_pose_worker, 2, "gloo")
    print("data_parallel PoseNet: %s" % (res,))
    for out in res:
        assert out["ranks_equal"] and not out["differ"] and not out["skipped"] and out["grad_norm"] > 0
        assert out["project_has_no_grad"] and out["buffers_own_before_sync"] and out["buffers_equal_after_sync"]
    assert res[0]["emulation_equal"], res[0]["first_difference"]


# ---- ranks that disagree ----

def _mismatch_worker(rank, world, port, q, backend):
    device = _init(rank, world, port, backend)
    from centerpose_amd.data_parallel import DataParallel

    xs, lins = _toy_data(1, 4, device)
    net = DataParallel(_toy(100, device))
    if rank == 1:
        net.module.conv2.bias.requires_grad_(False)   # on this rank alone the graph leaves one more parameter out
    _backward(net, xs[0][2 * rank:2 * rank + 2], lins[0][2 * rank:2 * rank + 2])
    out = {"has_grad": net.module.conv2.bias.grad is not None}
    try:
        net.reduce_gradients()
        out["raised"] = None
    except RuntimeError as e:
        out["raised"] = str(e)
    out["differ"] = bool(net.active_sets_differ)
    torch.cuda.synchronize()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
    q.put((rank, out))


def test_ranks_that_disagree_raise_on_both(device):
    res = _run_ranks(_mismatch_worker, 2, "gloo")
    assert [out["has_grad"] for out in res] == [True, False]
    for out in res:
        assert out["differ"] and out["raised"] is not None, out
        assert "conv2.bias (on 1 of 2 ranks)" in out["raised"] and "never_used" not in out["raised"], out["raised"]
