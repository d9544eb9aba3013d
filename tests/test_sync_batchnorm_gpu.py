"""SyncBatchNorm on the device (pytest -m gpu): cp_batchnorm_sync_* through ``hip.sync_norm``, ``sync_norm.SyncBatchNorm`` and
``DataParallel(sync_batchnorm=True)``.

The kernels are tested with no process group: tests/sync_batchnorm_ref.py's driver runs the ranks' phases on the one GPU and
concatenates their records by hand; the reference is float64 ``F.batch_norm`` on the WHOLE batch (tests/batchnorm_ref.py) at
its TOL = 1e-4 x max |reference| per output.  What the ranks share is compared bit for bit.

The collectives are tested with two ranks on the one GPU of the test box over gloo (two RCCL ranks cannot share a device;
tests/test_data_parallel_gpu.py does the same).  Children (tests/sync_batchnorm_ref.py: run_ranks): fresh processes, joined
under one 120 s limit, terminated then, and the test fails at once when a child ends with anything but exit code 0; with
the parent, three processes hold the GPU.
"""
import copy
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from centerpose_amd import hip, norm, sync_norm
from tests import batchnorm_ref as R
from tests import sync_batchnorm_ref as SR

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
pytestmark = pytest.mark.gpu
GRID = [(residual, act) for residual in (False, True) for act in (0, 1)]
SHARED = ("save_mean", "save_invstd", "save_count", "running_mean", "running_var")


def _ranks_share_bits(ranks):
    for r in ranks[1:]:
        for k in SHARED:
            assert torch.equal(r[k], ranks[0][k]), k


@pytest.mark.parametrize("cs", SR.SHARDED, ids=SR.sharded_id)
def test_sharded_against_the_whole_batch(device, cs):
    c, shards = cs
    inp = R.inputs(sum(c), c)
    for residual, act in GRID:
        whole, ranks = SR.check_sharded(device, inp, shards, residual, act, "%s res=%d act=%d" % (SR.sharded_id(cs), residual, act))
        _ranks_share_bits(ranks)
        assert float(ranks[0]["save_count"]) == c.B * c.H * c.W
        if residual and not act:   # nothing gates: grad_residual is grad_out itself
            assert torch.equal(whole["grad_residual"], inp.go)


@pytest.mark.parametrize("cs", SR.LARGE_MEAN_SHARDED, ids=SR.sharded_id)
def test_sharded_large_mean(device, cs):
    """x = 1000 + N(0, 1): the rank merge must not form E[x^2] - mean^2 either."""
    c, shards = cs
    inp = R.inputs(sum(c), c, mean=1000.0)
    for residual, act in GRID:
        _, ranks = SR.check_sharded(device, inp, shards, residual, act, "mean 1000 %s res=%d act=%d" % (SR.sharded_id(cs), residual, act))
        _ranks_share_bits(ranks)


def test_global_count_of_two_forward(device):
    """One value per channel on each of two ranks.  (grad_x at n = 2 is ill-conditioned: tests/sync_batchnorm_ref.py.)"""
    c, shards = SR.N2_SHARDED
    inp = R.inputs(sum(c), c)
    for residual, act in GRID:
        _, ranks = SR.check_sharded(device, inp, shards, residual, act, "n=2 res=%d act=%d" % (residual, act), backward=False)
        _ranks_share_bits(ranks)
        assert float(ranks[0]["save_count"]) == 2.0


def test_record_layout(device):
    """mean[C] | M2[C] | the count as an int32 bit pattern, the rest of its 16-byte slot zero."""
    c = R.CASES[3]
    inp = R.inputs(4, c)
    x = R.nhwc(inp.x).to(device)
    rec = hip.sync_norm.stats(x).cpu()
    assert rec.numel() == hip.sync_norm.record_floats(c.C) == 2 * c.C + 4
    assert rec[2 * c.C:].view(torch.int32).tolist() == [c.B * c.H * c.W, 0, 0, 0]
    xd = inp.x.double()
    mean = xd.mean((0, 2, 3))
    M2 = ((xd - mean.view(1, -1, 1, 1)) ** 2).sum((0, 2, 3))
    R.check(dict(mean=rec[:c.C], M2=rec[c.C:2 * c.C]), dict(mean=mean, M2=M2), "record")


@pytest.mark.parametrize("c", SR.WORLD1_CASES, ids=R.case_id)
def test_world1_is_the_plain_operator_bitwise(device, c):
    inp = R.inputs(sum(c) + 2, c)
    for residual, act in GRID:
        fwd = R.device_forward(device, inp, residual, act)
        bwd = R.device_backward(device, inp, fwd, residual, act)
        whole, ranks = SR.run_sharded(device, inp, (c.B,), residual, act)
        for name, t in fwd[0].items():
            assert torch.equal(whole[name], t), (name, residual, act)
        r = ranks[0]
        assert torch.equal(r["y"], fwd[1]) and torch.equal(r["save_mean"], fwd[2]) and torch.equal(r["save_invstd"], fwd[3])
        assert torch.equal(whole["grad_x"], bwd["grad_x"])
        assert torch.equal(r["grad_gamma"].cpu(), bwd["grad_gamma"]) and torch.equal(r["grad_beta"].cpu(), bwd["grad_beta"])
        if residual:
            assert torch.equal(whole["grad_residual"], bwd["grad_residual"])


@pytest.mark.parametrize("cs", [SR.SHARDED[2], SR.SHARDED[4], SR.SHARDED[6]], ids=SR.sharded_id)
def test_two_calls_are_bit_identical(device, cs):
    c, shards = cs
    inp = R.inputs(5, c)
    a, b = SR.run_sharded(device, inp, shards, True, 1), SR.run_sharded(device, inp, shards, True, 1)
    for name in a[0]:
        assert torch.equal(a[0][name], b[0][name]), name
    for p, q in zip(a[1], b[1]):
        for name in p:
            assert torch.equal(p[name], q[name]), name


@pytest.mark.parametrize("cs", [SR.SHARDED[2], SR.SHARDED[5]], ids=SR.sharded_id)
def test_null_outputs_and_guard_bands(device, cs):
    c, shards = cs
    inp = R.inputs(6, c)
    full, franks = SR.run_sharded(device, inp, shards, True, 1)
    # the outputs that are asked for do not depend on the ones that are not
    for need_x, need_g, need_b in ((False, True, True), (True, False, False), (True, True, False)):
        part, pranks = SR.run_sharded(device, inp, shards, True, 1, need_x=need_x, need_gamma=need_g, need_beta=need_b)
        assert (part["grad_x"] is None) == (not need_x) and (part["grad_gamma"] is None) == (not need_g)
        assert (part["grad_beta"] is None) == (not need_b)
        for name in ("grad_x", "grad_residual", "grad_gamma", "grad_beta"):
            assert part[name] is None or torch.equal(part[name], full[name]), name
        for p, q in zip(pranks, franks):
            assert torch.equal(p["sums"], q["sums"])
    # through the C ABI with the record, the sums and every other output inside canary buffers, for the first shard
    L = hip.lib()
    b0, G = shards[0], 1024
    geo = (b0, c.H, c.W, c.C)
    n, rec, world = b0 * c.H * c.W * c.C, hip.sync_norm.record_floats(c.C), len(shards)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, res, go = (R.nhwc(t)[:b0].contiguous().to(device) for t in (inp.x, inp.res, inp.go))
    gamma, beta = inp.gamma.to(device), inp.beta.to(device)
    nbytes = L.cp_batchnorm_workspace_bytes(*geo)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    canary = lambda m: torch.full((m + 2 * G,), 7.25, device=device)
    big = [canary(n) for _ in range(3)]          # y, grad_x, grad_residual
    small = [canary(c.C) for _ in range(4)]      # save_mean, save_invstd, grad_gamma, grad_beta
    record, sums, count = canary(rec), canary(2 * c.C), canary(4)
    assert L.cp_batchnorm_sync_stats_nhwc(stream, p(x), p(record, G), *geo, p(ws), nbytes) == 0, L.cp_last_error()
    records = torch.stack([record[G:-G]] + [r["record"] for r in franks[1:]]).contiguous()
    rc = L.cp_batchnorm_sync_forward_nhwc(stream, p(x), p(gamma), p(beta), p(res), None, None, p(big[0], G), p(small[0], G),
                                          p(small[1], G), p(count, G), p(records), world, *geo, R.MOMENTUM, R.EPS, 1, p(ws), nbytes)
    assert rc == 0, L.cp_last_error()
    rc = L.cp_batchnorm_sync_backward_reduce_nhwc(stream, p(x), p(big[0], G), p(go), p(small[0], G), p(small[1], G), p(sums, G),
                                                  p(small[2], G), p(small[3], G), *geo, p(ws), nbytes)
    assert rc == 0, L.cp_last_error()
    sums_all = torch.stack([sums[G:-G]] + [r["sums"] for r in franks[1:]]).contiguous()
    rc = L.cp_batchnorm_sync_backward_apply_nhwc(stream, p(x), p(big[0], G), p(go), p(gamma), p(small[0], G), p(small[1], G),
                                                 p(sums_all), world, p(count, G), p(big[1], G), p(big[2], G), *geo, p(ws), nbytes)
    assert rc == 0, L.cp_last_error()
    torch.cuda.synchronize()
    for t in big + small + [record, sums, count]:
        assert bool((t[:G] == 7.25).all()) and bool((t[-G:] == 7.25).all())
    assert float(count[G]) == c.B * c.H * c.W and bool((count[G + 1:-G] == 7.25).all())   # one float, no more
    r0 = franks[0]
    assert torch.equal(record[G:-G], r0["record"]) and torch.equal(sums[G:-G], r0["sums"])
    assert torch.equal(big[0][G:-G].view(geo), r0["y"]) and torch.equal(big[1][G:-G].view(geo), r0["grad_x"])
    assert torch.equal(big[2][G:-G].view(geo), r0["grad_residual"])
    assert torch.equal(small[0][G:-G], r0["save_mean"]) and torch.equal(small[1][G:-G], r0["save_invstd"])
    assert torch.equal(small[2][G:-G], r0["grad_gamma"]) and torch.equal(small[3][G:-G], r0["grad_beta"])
    assert torch.equal(small[0][G:-G].cpu(), full["save_mean"])   # (running statistics NULL here, given there)


def test_eval_and_no_process_group_are_batchnorm2d_bitwise(device):
    """Without an initialised process group the module takes BatchNorm2d's path, training or not."""
    assert not torch.distributed.is_initialized()
    c = R.CASES[2]
    inp = R.inputs(9, c)
    for relu, residual in GRID:
        plain = norm.BatchNorm2d(c.C).to(device)
        with torch.no_grad():
            plain.weight.copy_(inp.gamma), plain.bias.copy_(inp.beta)
        plain.relu = bool(relu)
        ours = copy.deepcopy(plain)
        assert sync_norm.use_hip_sync_norms(ours) == ([""], {}) and type(ours) is sync_norm.SyncBatchNorm and ours.relu == bool(relu)
        for mode in ("train", "eval"):
            outs = []
            for m in (plain, ours):
                getattr(m, mode)()
                x = inp.x.to(device).requires_grad_(True)
                res = inp.res.to(device).requires_grad_(True) if residual else None
                y = m(x, res)
                y.backward(inp.go.to(device))
                outs.append([y.detach(), x.grad, m.weight.grad.clone(), m.bias.grad.clone(), m.running_mean.clone(), m.running_var.clone(),
                             m.num_batches_tracked.clone()] + ([res.grad] if residual else []))
                m.zero_grad(set_to_none=True)
            for a, b in zip(*outs):
                assert torch.equal(a, b), (mode, relu, residual)


# ---- two ranks on the one GPU over gloo ----

def _init(rank, world, port):
    sys.path.insert(0, REPO)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from centerpose_amd import distributed as d

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    assert d.init_from_env("gloo") == (rank, world)
    return device


def _np(t):
    """What a child puts on the queue: an array travels by value (a tensor would travel as a handle of the child's memory)."""
    return t.detach().cpu().numpy()


def _t(a):
    return torch.from_numpy(a)


def _finish(q, rank, out):
    torch.cuda.synchronize()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
    q.put((rank, out))


BN_CASE = R.Case(5, 6, 7, 20)   # 5 images over 2 ranks: 3 + 2; five lanes per row


class BnNet(nn.Module):
    """BatchNorm + ReLU, a per-channel scale in torch, BatchNorm + the input as residual + ReLU."""

    def __init__(self, C):
        super().__init__()
        self.bn1, self.bn2 = norm.BatchNorm2d(C), norm.BatchNorm2d(C)
        self.bn1.relu = self.bn2.relu = True
        self.scale = nn.Parameter(torch.ones(C))

    def forward(self, x):
        self.h = self.bn1(x)
        return self.bn2(self.h * self.scale.view(1, -1, 1, 1), x)


def _bn_case():
    """x, lin [5,20,6,7] and the parameters' values: {name: tensor}."""
    c = BN_CASE
    inp, other = R.inputs(31, c), R.inputs(32, c)
    values = {"bn1.weight": inp.gamma, "bn1.bias": inp.beta, "bn2.weight": other.gamma, "bn2.bias": 0.5 * other.beta,
              "scale": 1 + 0.25 * other.rmean}
    return inp.x, inp.go, values


def _bn_worker(rank, world, port, q, stage):
    device = _init(rank, world, port)
    from centerpose_amd import distributed as d
    from centerpose_amd.data_parallel import DataParallel

    x, lin, values = _bn_case()
    model = BnNet(BN_CASE.C)
    if rank == 0:   # rank 1 keeps its initial values: construction gives it rank 0's
        with torch.no_grad():
            for k, p in model.named_parameters():
                p.copy_(values[k])
    net = DataParallel(model.to(device).train(), stage_on_host=stage, sync_batchnorm=True)
    mine = d.shard_batch({"x": x.to(device), "lin": lin.to(device)}, rank, world)
    xr = mine["x"].clone().requires_grad_(True)
    out = net(xr)
    loss = (out * mine["lin"]).sum() / xr.shape[0]   # L_rank: the mean over this rank's images
    loss.backward()
    net.reduce_gradients()
    res = {"converted": net.sync_batchnorm_converted, "skipped": net.sync_batchnorm_skipped, "comm_path": net.comm_path,
           "types": [type(m).__name__ for m in (model.bn1, model.bn2)], "shard": xr.shape[0],
           "grad_x": _np(xr.grad), "y1": _np(model.h), "y2": _np(out),
           "grads": {k: _np(p.grad) for k, p in model.named_parameters()},
           "buffers": {k: _np(b) for k, b in model.named_buffers()}}
    _finish(q, rank, res)


def _bn_reference(y1, y2):
    """float64 autograd of (L_0 + L_1) / 2 on the concatenated batch, BatchNorm over all of it; the ReLUs take the device's
    gates y1 > 0, y2 > 0 (tests/batchnorm_ref.py says why).  Returns (grad_x, {name: grad}, {buffer name: value})."""
    x, lin, values = _bn_case()
    x = x.double().requires_grad_(True)
    v = {k: t.double().requires_grad_(True) for k, t in values.items()}
    C = BN_CASE.C
    rm = [torch.zeros(C, dtype=torch.float64) for _ in range(2)]
    rv = [torch.ones(C, dtype=torch.float64) for _ in range(2)]
    h = F.batch_norm(x, rm[0], rv[0], v["bn1.weight"], v["bn1.bias"], True, 0.1, 1e-5) * (y1 > 0).double()
    out = (F.batch_norm(h * v["scale"].view(1, -1, 1, 1), rm[1], rv[1], v["bn2.weight"], v["bn2.bias"], True, 0.1, 1e-5) + x) * (y2 > 0).double()
    per_image = (out * lin.double()).sum((1, 2, 3))
    loss = (per_image[:3].sum() / 3 + per_image[3:].sum() / 2) / 2
    names = list(v)
    grads = torch.autograd.grad(loss, [x] + [v[k] for k in names])
    buffers = {"bn1.running_mean": rm[0], "bn1.running_var": rv[0], "bn2.running_mean": rm[1], "bn2.running_var": rv[1]}
    return grads[0], dict(zip(names, grads[1:])), buffers, out.detach()


@pytest.mark.parametrize("stage", [None, True], ids=["device_tensors", "pinned_host"])
def test_two_ranks_equal_the_whole_batch(device, stage):
    res = SR.run_ranks(_bn_worker, stage)
    for r in res:
        r.update({k: _t(r[k]) for k in ("grad_x", "y1", "y2")}, grads={k: _t(v) for k, v in r["grads"].items()},
                 buffers={k: _t(v) for k, v in r["buffers"].items()})
    y1, y2 = (torch.cat([r[k] for r in res]) for k in ("y1", "y2"))
    grad_x, grads, buffers, out = _bn_reference(y1, y2)
    assert [r["shard"] for r in res] == [3, 2]
    for rank, r in enumerate(res):
        assert r["converted"] == ["bn1", "bn2"] and r["skipped"] == {} and r["types"] == ["SyncBatchNorm"] * 2
        assert r["comm_path"] == ("pinned host" if stage else "device")
        # a rank's grad_x is the gradient of L_0 + L_1: twice that of the mean of the rank losses
        s = slice(0, 3) if rank == 0 else slice(3, 5)
        R.check({"grad_x": r["grad_x"] / 2, "y": r["y2"]}, {"grad_x": grad_x[s], "y": out[s]}, "rank %d" % rank)
        R.check(r["grads"], grads, "rank %d reduced" % rank)
        R.check(r["buffers"], buffers, "rank %d running" % rank)
    for k in res[0]["buffers"]:   # before any sync_buffers()
        assert torch.equal(res[0]["buffers"][k], res[1]["buffers"][k]), k
    for k in res[0]["grads"]:
        assert torch.equal(res[0]["grads"][k], res[1]["grads"][k]), k


# ---- PoseNet, two ranks ----

def _pose_worker(rank, world, port, q):
    device = _init(rank, world, port)
    from centerpose_amd import distributed as d
    from centerpose_amd.data_parallel import DataParallel
    from tests.test_data_parallel_gpu import _pose_backward, _pose_case, _pose_net

    hip.set_default_precision("f32")
    hip.set_deterministic(True)
    sd, x, lin = _pose_case()
    x, lin = x.to(device), {h: v.to(device) for h, v in lin.items()}
    mine = d.shard_batch(dict(lin, x=x), rank, world)
    model = _pose_net(copy.deepcopy(sd), device)
    keys = list(model.state_dict())
    before = [k for k, m in model.named_modules() if isinstance(m, norm.BatchNorm2d)]
    net = DataParallel(model, sync_batchnorm=True)
    layers = [(k, m) for k, m in model.named_modules() if isinstance(m, sync_norm.SyncBatchNorm)]
    tracked = [int(m.num_batches_tracked) for _, m in layers]
    loss = _pose_backward(net, mine.pop("x"), mine)
    net.reduce_gradients()
    ran = [(k, m) for (k, m), n in zip(layers, tracked) if int(m.num_batches_tracked) == n + 1]
    out = {"before": before, "converted": net.sync_batchnorm_converted, "skipped": net.sync_batchnorm_skipped,
           "left": [k for k, m in model.named_modules() if isinstance(m, nn.modules.batchnorm._BatchNorm) and type(m) is not sync_norm.SyncBatchNorm],
           "keys_unchanged": list(model.state_dict()) == keys, "ran": [k for k, _ in ran],
           "stats": _np(torch.cat([t.detach().reshape(-1) for _, m in ran for t in (m.running_mean, m.running_var)])),
           "differ": bool(net.active_sets_differ), "loss": float(loss)}
    _finish(q, rank, out)


def test_pose_net_two_ranks_sync_batchnorm(device):
    res = SR.run_ranks(_pose_worker)
    for out in res:
        assert len(out["before"]) > 50 and out["converted"] == out["before"] and out["skipped"] == {} and out["left"] == []
        assert out["keys_unchanged"] and not out["differ"] and out["loss"] == out["loss"] and abs(out["loss"]) < float("inf")
        assert len(out["ran"]) > 50 and out["ran"] == res[0]["ran"]
    assert torch.equal(_t(res[0]["stats"]), _t(res[1]["stats"]))   # before any sync_buffers()
