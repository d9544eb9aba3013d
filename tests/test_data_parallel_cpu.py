"""CPU tests (no GPU) of data-parallel training: the flat gradient layout and the pack table of cp_grad_* (host functions of
csrc/grad_pack.hip), their refusals, and -- world size 2 over gloo on CPU tensors, the pattern of tests/test_distributed_cpu.py
-- ``distributed.shard_batch``, ``DataParallel.reduce_stats`` and the coalesced broadcasts behind ``DataParallel``'s
construction and ``sync_buffers``.  The pack itself has no CPU path (tests/test_data_parallel_gpu.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import __graft_entry__ as ge
from centerpose_amd import hip

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LENGTHS = [0, 1, 3, 4, 5, 4095, 4096, 4097, 8193]
NEW = ("cp_grad_flat_elems", "cp_grad_flat_offsets", "cp_grad_pack_table_bytes", "cp_grad_pack_table_build", "cp_grad_pack")


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def _i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def test_symbols_and_constants(built):
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    for name in NEW:
        assert hasattr(built, name) and name in hip.exported_symbols() and name in header.split("#define CP_ABI_VERSION")[0], name
    assert built.cp_abi_version() == 7 == hip.ABI_VERSION
    for name, value in (("TENSOR_BYTES", hip.optim.GRAD_TENSOR_BYTES), ("CHUNK_BYTES", hip.optim.GRAD_CHUNK_BYTES),
                        ("VEC", hip.optim.GRAD_VEC), ("ZERO", hip.optim.GRAD_ZERO)):
        assert "#define CP_GRAD_%s %d\n" % (name, value) in header, name
    assert not hasattr(hip, "grad_pack")   # the recorded surface of `hip` stays as it is: callers use hip.optim.grad_pack


def test_layout(built):
    offsets, total = hip.optim.grad_flat_layout(LENGTHS)
    n = len(LENGTHS)
    assert len(offsets) == n + 1 and offsets[0] == 0
    for i, length in enumerate(LENGTHS):
        assert offsets[i] % 4 == 0
        assert offsets[i + 1] >= offsets[i] + length            # ascending, no overlap
        assert offsets[i + 1] - (offsets[i] + length) < 4       # no more padding than alignment asks for
    assert offsets[1] == offsets[0]                              # the zero-length tensor takes no space
    assert offsets[n] % 4 == 0 and total == offsets[n] + (n + 3) // 4 * 4   # the tail: n floats, padded to a multiple of 4
    assert total == built.cp_grad_flat_elems(n, _i64(LENGTHS))
    # no pointer goes into it: the same lengths give the same layout whatever the table is later built from
    a, b = hip.optim.GradPackArrays(LENGTHS), hip.optim.GradPackArrays(LENGTHS)
    for i in range(n):
        a.src[i] = 0x7f0000000000 + 0x10000 * i + 4
    assert list(a.offsets) == list(b.offsets) == offsets and a.flat_elems == b.flat_elems == total
    assert hip.optim.grad_flat_layout([7]) == ([0, 8], 12) and hip.optim.grad_flat_layout([0]) == ([0, 0], 4)


def test_layout_refusals(built):
    for n, lengths, text in ((0, [5], b"n_tensors must be >= 1"), (2, [5, -1], b"length -1"),
                             (2, [(1 << 31) - 8, 8], b"2^31 - 1 elements"), (1, [1 << 31], b"2^31 - 1 elements")):
        arr = _i64(lengths)
        assert built.cp_grad_flat_elems(n, arr) == 0 and text in built.cp_last_error(), lengths
        off = _i64([0] * (len(lengths) + 1))
        assert built.cp_grad_flat_offsets(n, arr, off) == hip.CP_ERR_INVALID and text in built.cp_last_error()
        nc = ctypes.c_int(0)
        assert built.cp_grad_pack_table_bytes(n, arr, ctypes.byref(nc)) == 0 and text in built.cp_last_error()
    for lengths in ([], [5, -1], [1 << 31]):
        with pytest.raises(ValueError):
            hip.optim.grad_flat_layout(lengths)
    # the largest accepted: tensors, padding and flags together are 2^31 - 1 - 3 floats (a multiple of 4)
    assert hip.optim.grad_flat_layout([(1 << 31) - 8])[1] == (1 << 31) - 4
    assert built.cp_grad_flat_elems(1, None) == 0 and b"null" in built.cp_last_error()


def _parse(buf, n, n_chunks):
    raw = buf.numpy()
    tensors = raw[:16 * (n + 1)].view(np.int64).reshape(n + 1, 2)
    chunks = raw[16 * (n + 1):16 * (n + 1) + 16 * n_chunks].view(np.int32).reshape(n_chunks, 4)
    return tensors, chunks


def test_host_table(built):
    n = len(LENGTHS)
    a = hip.optim.GradPackArrays(LENGTHS)
    absent, odd = LENGTHS.index(4097), LENGTHS.index(8193)
    addresses = [0x100000 * (i + 1) for i in range(n)]
    addresses[absent] = 0            # NULL: no gradient
    addresses[odd] += 4              # 4-byte aligned only
    for i in range(n):
        a.src[i] = addresses[i] or None
    nbytes, n_chunks = hip.optim.grad_pack_table_bytes(a)
    assert n_chunks == sum((length + 4095) // 4096 for length in LENGTHS) and nbytes == 16 * (n + 1) + 16 * n_chunks
    buf = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8)
    assert hip.optim.grad_pack_table_build(buf[:nbytes], a) == n_chunks
    assert bool((buf[nbytes:] == 0xAB).all())   # nothing written past the table
    tensors, chunks = _parse(buf, n, n_chunks)
    for i in range(n):
        assert tensors[i, 0] == addresses[i] and tensors[i, 1] == a.offsets[i], i
    assert tensors[n, 0] == 0 and tensors[n, 1] == a.offsets[n]   # where the flags go
    covered = [np.zeros(length, dtype=np.int32) for length in LENGTHS]
    last = (-1, -1)
    for t, start, count, flags in chunks:
        start = int(np.uint32(start))
        assert 0 <= t < n and 1 <= count <= hip.optim.ADAM_CHUNK and start % hip.optim.ADAM_CHUNK == 0
        assert start + count <= LENGTHS[t]                        # no chunk straddles two tensors
        assert (t, start) > last
        last = (t, start)
        want = hip.optim.GRAD_ZERO if t == absent else 0 if t == odd else hip.optim.GRAD_VEC
        assert flags == want, (t, flags)
        covered[t][start:start + count] += 1
    for i in range(n):
        assert bool((covered[i] == 1).all()), i                   # every element once, with a source or without
    # refusals
    with pytest.raises(ValueError, match="table buffer too small"):
        hip.optim.grad_pack_table_build(buf[:nbytes - 1], a)
    a.src[3] = 0x100002
    with pytest.raises(ValueError, match="misaligned"):
        hip.optim.grad_pack_table_build(buf[:nbytes], a)
    a.src[3] = 0x100000
    a.offsets[2] += 4
    with pytest.raises(ValueError, match="not the layout's"):
        hip.optim.grad_pack_table_build(buf[:nbytes], a)
    a.offsets[2] -= 4
    nc = ctypes.c_int(0)
    args = (ctypes.c_void_p(buf.data_ptr()), nbytes, n, a.src, a.lengths, a.offsets, ctypes.byref(nc))
    for i in (0, 3, 4, 5, 6):
        bad = list(args)
        bad[i] = None
        assert built.cp_grad_pack_table_build(*bad) == hip.CP_ERR_INVALID and b"null" in built.cp_last_error(), i


def test_pack_refusals_without_a_device(built):
    p = ctypes.c_void_p(0x1000)

    def pack(table=p, n_tensors=3, n_chunks=5, flat=p, flat_elems=1 << 20, scale=0.5):
        return built.cp_grad_pack(None, table, n_tensors, n_chunks, flat, flat_elems, scale)

    def refused(text, **kw):
        assert pack(**kw) == hip.CP_ERR_INVALID and text in built.cp_last_error(), (kw, built.cp_last_error())

    refused(b"null argument", table=None)
    refused(b"null argument", flat=None)
    refused(b"n_tensors must be >= 1", n_tensors=0)
    refused(b"n_chunks must be >= 0", n_chunks=-1)
    refused(b"16-byte aligned", flat=ctypes.c_void_p(0x1008))
    refused(b"8-byte aligned", table=ctypes.c_void_p(0x1004))
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(b"non-finite scale", scale=bad)
    refused(b"flat_elems is below", flat_elems=3)                                 # three flags alone take 4 floats
    refused(b"flat_elems is below", flat_elems=2 * 4096 + 3, n_chunks=5)          # 5 chunks of 3 tensors: more than 2 whole ones


def test_no_cpu_path(built):
    from centerpose_amd.data_parallel import DataParallel

    t = torch.zeros(256, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.optim.grad_pack(t, 1, 1, torch.zeros(64))
    net = DataParallel(torch.nn.Linear(4, 3))
    assert net.world == 1 and net.flat.device.type == "cpu" and not bool(net.flat.any())
    net(torch.ones(2, 4)).sum().backward()
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.reduce_gradients()
    assert net.module.weight.grad is not None and net.module.weight.grad.data_ptr() != net.flat.data_ptr()
    for dtype in (torch.float64, torch.float16):
        with pytest.raises(NotImplementedError, match="centerpose_amd.optim.Adam: float32 strided parameters only"):
            DataParallel(torch.nn.Linear(4, 3).to(dtype))


def _net(seed):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Conv2d(4, 2, 1))
    with torch.no_grad():
        net[1].running_mean.normal_()
        net[1].running_var.uniform_(0.5, 2.0)
        net[1].num_batches_tracked.fill_(10 + seed)
        net[0].weight.data = net[0].weight.data.contiguous(memory_format=torch.channels_last)
    return net


def _worker(rank, world, port, q):
    sys.path.insert(0, REPO)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from centerpose_amd import distributed as d
    from centerpose_amd.data_parallel import DataParallel

    assert d.init_from_env("gloo") == (rank, world)
    # shard_batch: 5 images over 2 ranks are 3 + 2; non-tensors pass through
    batch = {"input": torch.arange(5 * 6, dtype=torch.float32).view(5, 2, 3), "ind": torch.arange(5), "meta": {"id": 7}, "n": 5}
    mine = d.shard_batch(batch, rank, world)
    s, e = (0, 3) if rank == 0 else (3, 5)
    ok_shard = (torch.equal(mine["input"], batch["input"][s:e]) and torch.equal(mine["ind"], batch["ind"][s:e])
                and mine["meta"] is batch["meta"] and mine["n"] == 5)
    # construction: rank 1, seeded differently, ends with rank 0's parameters and buffers (an int64 one among them)
    want = _net(0)
    net = DataParallel(_net(rank))
    sd, sw = net.module.state_dict(), want.state_dict()
    ok_bcast = list(sd) == list(sw) and all(torch.equal(sd[k], sw[k]) and sd[k].dtype == sw[k].dtype for k in sw)
    ok_bcast = ok_bcast and int(sd["1.num_batches_tracked"]) == 10 and sd["1.num_batches_tracked"].dtype == torch.int64
    ok_bcast = ok_bcast and net.module[0].weight.is_contiguous(memory_format=torch.channels_last)
    # sync_buffers: buffers that drifted apart are rank 0's again; parameters are not touched
    with torch.no_grad():
        net.module[1].running_mean.add_(rank + 1.0)
        net.module[1].num_batches_tracked.add_(rank + 1)
        net.module[2].bias.add_(rank + 1.0)
    net.sync_buffers()
    ok_sync = (torch.equal(net.module[1].running_mean, want[1].running_mean + 1.0) and int(net.module[1].num_batches_tracked) == 11
               and torch.equal(net.module[2].bias, want[2].bias + (rank + 1.0)))
    # reduce_stats: the means over the ranks
    out = net.reduce_stats({"loss": torch.tensor(1.0 + 2.0 * rank), "hm_loss": 0.25 * (rank + 1), "n": 4})
    ok_stats = list(out) == ["loss", "hm_loss", "n"] and [float(out[k]) for k in out] == [2.0, 0.375, 4.0] and out["loss"].dim() == 0
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
    q.put((rank, ok_shard, ok_bcast, ok_sync, ok_stats))


def test_world2_gloo(built):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 30500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=120) for _ in procs]
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    assert sorted(res) == [(0, True, True, True, True), (1, True, True, True, True)]
