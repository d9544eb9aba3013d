"""CPU tests (no GPU) of SyncBatchNorm: the C ABI's declarations and refusals (cp_batchnorm_sync_*), the
sync_norm.SyncBatchNorm module, use_hip_sync_norms, DataParallel's switch and distributed.all_gather_flat on two gloo ranks."""
import ctypes
import os
import re
import sys

import pytest
import torch
from torch import nn

import __graft_entry__ as ge
from centerpose_amd import distributed as cpd
from centerpose_amd import hip, norm, sync_norm
from tests import sync_batchnorm_ref as SR

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_batchnorm_sync_record_floats", "cp_batchnorm_sync_stats_nhwc", "cp_batchnorm_sync_forward_nhwc",
       "cp_batchnorm_sync_backward_reduce_nhwc", "cp_batchnorm_sync_backward_apply_nhwc")


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def test_symbols_declared_exported_and_listed(built):
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    testing = open(os.path.join(REPO, "include", "centerpose_hip_testing.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and hasattr(built, name) and name in hip.exported_symbols(), name
        assert name in hip._abi.SIGNATURES and name not in testing
    assert int(re.search(r"#define\s+CP_ABI_VERSION\s+(\d+)", header).group(1)) == 7 == built.cp_abi_version() == hip.ABI_VERSION
    # the wrappers are a module of the binding, not new flat names
    assert hip.sync_norm.__name__ == "centerpose_amd.hip.sync_norm"
    for name in ("record_floats", "stats", "forward", "backward_reduce", "backward_apply"):
        assert callable(getattr(hip.sync_norm, name)) and not hasattr(hip, "sync_norm_" + name)
    assert not hasattr(hip, "stats") and not hasattr(hip, "backward_reduce")


def test_record_floats(built):
    q = built.cp_batchnorm_sync_record_floats
    for C in (4, 16, 20, 136, 512, 4096):
        assert q(C) == 2 * C + 4 and q(C) % 4 == 0
    for C in (0, 2, 6, -4, 4100):
        assert q(C) == 0 and b"multiple of 4 in 4..4096" in built.cp_last_error(), C


def test_refusals_without_a_device(built):
    """Every refusal comes before any launch: no device is touched and the pointers are never dereferenced."""
    p, other = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
    odd = ctypes.c_void_p(0x1004)
    ok = (2, 8, 8, 16)
    need = built.cp_batchnorm_workspace_bytes(*ok)
    assert need > 0

    def st(x=p, record=p, geo=ok, ws=p, nbytes=need):
        return built.cp_batchnorm_sync_stats_nhwc(None, x, record, *geo, ws, nbytes)

    def f(x=p, gamma=p, beta=p, res=p, rm=p, rv=p, y=other, mean=p, invstd=p, count=p, records=p, world=2, geo=ok, momentum=0.1,
          eps=1e-5, act=1, ws=p, nbytes=need):
        return built.cp_batchnorm_sync_forward_nhwc(None, x, gamma, beta, res, rm, rv, y, mean, invstd, count, records, world, *geo,
                                                    momentum, eps, act, ws, nbytes)

    def br(x=p, y=p, go=p, mean=p, invstd=p, sums=p, gg=p, gb=p, geo=ok, ws=p, nbytes=need):
        return built.cp_batchnorm_sync_backward_reduce_nhwc(None, x, y, go, mean, invstd, sums, gg, gb, *geo, ws, nbytes)

    def ba(x=p, y=p, go=p, gamma=p, mean=p, invstd=p, sums_all=p, world=2, count=p, gx=p, gr=p, geo=ok, ws=p, nbytes=need):
        return built.cp_batchnorm_sync_backward_apply_nhwc(None, x, y, go, gamma, mean, invstd, sums_all, world, count, gx, gr, *geo,
                                                           ws, nbytes)

    def refused(rc, text):
        assert rc == hip.CP_ERR_INVALID == -1 and text in built.cp_last_error(), (rc, built.cp_last_error())

    nulls = {st: ("x", "record", "ws"), f: ("x", "y", "mean", "invstd", "count", "records", "ws"),
             br: ("x", "go", "mean", "invstd", "sums", "ws"), ba: ("x", "go", "mean", "invstd", "sums_all", "count", "ws")}
    for call, names in nulls.items():
        for name in names:
            refused(call(**{name: None}), b"null argument")
        refused(call(nbytes=need - 1), b"workspace too small")
        refused(call(geo=(0, 8, 8, 16)), b"at least 1")
        refused(call(geo=(2, 8, 0, 16)), b"at least 1")
        refused(call(geo=(2, 8, 8, 6)), b"multiple of 4")
        refused(call(geo=(2, 8, 8, 8192)), b"4..4096")
        refused(call(geo=(64, 1024, 1024, 32)), b"2^31 elements")
        refused(call(x=odd), b"16-byte aligned")
    refused(st(record=odd), b"16-byte aligned")
    refused(f(records=odd), b"16-byte aligned")
    refused(br(sums=odd), b"16-byte aligned")
    refused(ba(sums_all=odd), b"16-byte aligned")
    for call in (f, ba):
        for world in (0, -1, 1025):
            refused(call(world=world), b"world must be in 1..1024")
    # a global count below 2: all the host can know of it is a single rank with a single value per channel
    refused(f(world=1, geo=(1, 1, 1, 16)), b"global count >= 2")
    for act in (-1, 2):
        refused(f(act=act), b"act must be")
    refused(f(eps=-1e-5), b"eps must not be negative")
    refused(f(eps=float("nan")), b"eps must not be negative")
    refused(f(y=p), b"must not alias")


class _Derived(nn.BatchNorm2d):
    pass


class _Tree(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(8, 16, 3, padding=1, bias=False)
        self.ours = norm.BatchNorm2d(16)
        self.ours.relu = True
        self.block = nn.Sequential(nn.Conv2d(16, 16, 1), nn.BatchNorm2d(16, affine=False), nn.ReLU(), nn.BatchNorm2d(6))
        self.sync = nn.SyncBatchNorm(16)
        self.bn1d = nn.BatchNorm1d(16)
        self.gn = nn.GroupNorm(4, 16)
        self.f64 = nn.BatchNorm2d(16).double()
        self.plain = nn.BatchNorm2d(32, momentum=None, track_running_stats=False)
        self.derived = _Derived(16)
        self.already = sync_norm.SyncBatchNorm(8)


def test_use_hip_sync_norms_reclasses_in_place():
    torch.manual_seed(0)
    tree = _Tree()
    params, buffers, keys = dict(tree.named_parameters()), dict(tree.named_buffers()), list(tree.state_dict())
    group = object()   # (only stored)
    tree.already.process_group = "its own"
    converted, skipped = sync_norm.use_hip_sync_norms(tree, group)
    assert converted == ["ours", "block.1", "sync", "plain"]
    assert sorted(skipped) == ["block.3", "derived", "f64"]
    assert "multiple of 4" in skipped["block.3"] and "float64" in skipped["f64"]
    assert skipped["derived"] == "subclass _Derived keeps its own forward"
    for m in (tree.ours, tree.block[1], tree.sync, tree.plain):
        assert type(m) is sync_norm.SyncBatchNorm and m.process_group is group and isinstance(m, norm.BatchNorm2d)
    assert tree.ours.relu is True and tree.sync.relu is False and tree.plain.relu is False
    assert tree.already.process_group == "its own"
    assert type(tree.block[3]) is nn.BatchNorm2d and type(tree.f64) is nn.BatchNorm2d and type(tree.derived) is _Derived
    assert type(tree.bn1d) is nn.BatchNorm1d and type(tree.gn) is nn.GroupNorm and type(tree.conv1) is nn.Conv2d
    after, after_b = dict(tree.named_parameters()), dict(tree.named_buffers())
    assert list(after) == list(params) and all(after[k] is params[k] for k in params)
    assert list(after_b) == list(buffers) and all(after_b[k] is buffers[k] for k in buffers)
    assert list(tree.state_dict()) == keys
    assert sync_norm.use_hip_sync_norms(tree, group) == ([], skipped)
    # the default group: an nn.SyncBatchNorm keeps its own, everything else gets None
    own = nn.SyncBatchNorm(8, process_group="mine")
    lone = nn.BatchNorm2d(4)
    assert sync_norm.use_hip_sync_norms(own) == ([""], {}) and own.process_group == "mine"
    assert sync_norm.use_hip_sync_norms(lone) == ([""], {}) and lone.process_group is None
    # use_hip_norms leaves the converted layers alone
    assert norm.use_hip_norms(tree)[0] == [] and type(tree.ours) is sync_norm.SyncBatchNorm


def test_module_is_nn_batchnorm2d_but_for_forward():
    for args, kwargs in (((16,), {}), ((8,), dict(momentum=None)), ((12,), dict(affine=False)), ((4,), dict(track_running_stats=False)),
                         ((64,), dict(eps=1e-3, momentum=0.01))):
        torch.manual_seed(3)
        ours = sync_norm.SyncBatchNorm(*args, **kwargs)
        torch.manual_seed(3)
        theirs = nn.BatchNorm2d(*args, **kwargs)
        a, b = ours.state_dict(), theirs.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        assert [n for n, _ in ours.named_parameters()] == [n for n, _ in theirs.named_parameters()]
        assert [n for n, _ in ours.named_buffers()] == [n for n, _ in theirs.named_buffers()]
        assert isinstance(ours, norm.BatchNorm2d) and ours.relu is False and ours.process_group is None
    assert {n for n in vars(sync_norm.SyncBatchNorm) if not n.startswith("__")} == {"forward", "process_group"}


def test_zero_images_and_no_cpu_path():
    m = sync_norm.SyncBatchNorm(8)
    for mode in (m.train, m.eval):
        mode()
        with pytest.raises(RuntimeError, match="at least one"):
            m(torch.zeros(0, 8, 4, 4))
    assert int(m.num_batches_tracked) == 0   # raised before any bookkeeping
    with pytest.raises(RuntimeError, match="HIP device"):
        m.train()(torch.zeros(2, 8, 4, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        sync_norm.sync_batch_norm(torch.zeros(2, 8, 4, 4), None, None, None, None, True, 0.1, 1e-5)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.sync_norm.stats(torch.zeros(2, 4, 4, 8))


def test_data_parallel_switch_converts_before_anything_else():
    from centerpose_amd.data_parallel import DataParallel

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(4, 8, 1)
            self.bn = norm.BatchNorm2d(8)
            self.odd = nn.BatchNorm2d(6)

    a, b = DataParallel(Net()), DataParallel(Net(), sync_batchnorm=True)
    assert type(a.module.bn) is norm.BatchNorm2d and a.sync_batchnorm_converted == [] and a.sync_batchnorm_skipped == {}
    assert type(b.module.bn) is sync_norm.SyncBatchNorm and b.sync_batchnorm_converted == ["bn"] and list(b.sync_batchnorm_skipped) == ["odd"]
    assert list(a.state_dict()) == list(b.state_dict())


# ---- all_gather_flat on two gloo ranks ----

def _gather_worker(rank, world, port, q):
    sys.path.insert(0, REPO)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from centerpose_amd import distributed as d

    assert d.init_from_env("gloo") == (rank, world)
    t = torch.arange(6, dtype=torch.float32) + 10 * rank
    t[5] = torch.tensor([12345678 + rank], dtype=torch.int32).view(torch.float32)[0]   # a count's bits: a denormal as a float
    out = d.all_gather_flat(t)
    bad = None
    try:
        d.all_gather_flat(torch.zeros(2, 3))
    except ValueError as e:
        bad = str(e)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
    q.put((rank, (out.numpy(), t.numpy(), bad)))   # (arrays travel by value; tensors would travel as handles of this process)


def test_all_gather_flat_is_rank_order_and_moves_bits():
    t = torch.arange(5, dtype=torch.float32)
    alone = cpd.all_gather_flat(t)   # no process group
    assert alone.shape == (1, 5) and torch.equal(alone[0], t) and alone.data_ptr() != t.data_ptr()
    world = 2
    res = SR.run_ranks(_gather_worker)
    for rank in range(world):
        out, bad = torch.from_numpy(res[rank][0]), res[rank][2]
        assert out.shape == (2, 6) and "1-D" in bad
        for r in range(world):
            assert torch.equal(out[r].view(torch.int32), torch.from_numpy(res[r][1]).view(torch.int32)), (rank, r)
        assert out[:, 5].contiguous().view(torch.int32).tolist() == [12345678, 12345679]
