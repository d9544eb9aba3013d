"""Times the pieces data-parallel training adds to a step, on dla_34's real parameter set (the tensors of
synth.make_state_dict("dla_34", synth.HEADS_POSE, head_conv=256): about 250 tensors, 20.25 M floats) with random gradients.

On one GPU (the default):

  pack          hip.optim.grad_pack over a table that is already on the device                (csrc/grad_pack.hip: 1 launch)
  cat           torch.cat([g.reshape(-1) for g in grads])                                     (the baseline: one copy kernel per
                                                                                                tensor group, plus an allocation)
  reduce        DataParallel.reduce_gradients() at world size 1: table build + upload + pack + the views
  adam_fresh    optim.Adam.step() over gradients whose addresses change every step (two sets, alternating: the table is
                rebuilt and uploaded every step)
  adam_views    optim.Adam.step() over DataParallel's views (stable addresses: one upload in all)

After a warm-up of each route the routes alternate round by round and every round is reported.  A round times --steps calls
between two HIP events twice: on an idle device (ms: the larger of the host's time to queue a call and the device's to run
it) and behind a plug of matrix products that keeps the device busy until the host has queued the whole window (device_ms:
the device time alone).  GB/s is over the 8 bytes per element a pack has to move (4 read, 4 written), per device_ms.  One
JSON line per measurement, then a summary line per route (medians) with the ratio to `cat`.

With --gpus N (N > 1) it starts one process per GPU ($CP_BENCH_BACKEND, default nccl = RCCL; gloo with every rank on device
0 is a plumbing rehearsal on a one-GPU box) and times, per rank, the all-reduce of the flat buffer alone and a whole
reduce_gradients() + Adam.step(); the summary is the MAX over ranks of the per-rank median.

  python tools/data_parallel_bench.py [--gpus 1] [--rounds 7] [--steps 50] [--warmup 5] [--out profiles/data_parallel_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from centerpose_amd import hip, synth  # noqa: E402
from centerpose_amd.data_parallel import DataParallel  # noqa: E402
from centerpose_amd.optim import Adam  # noqa: E402

MAX_NORM = 100.0
LR = 1.25e-4


class _Params(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])


def _host_tensors():
    sd = synth.make_state_dict("dla_34", synth.HEADS_POSE, head_conv=256)
    return [v.float() for k, v in sd.items() if v.is_floating_point() and "running_" not in k]


def _grad_sets(host, dev, sets=2):
    gen = torch.Generator().manual_seed(5)
    return [[(1e-3 * torch.randn(t.shape, generator=gen)).to(dev) for t in host] for _ in range(sets)]


class _Plug(object):
    """Matrix products queued ahead of a timed window keep the device busy while the host queues the window's calls."""

    def __init__(self, dev):
        self.a = torch.randn(4096, 4096, device=dev)
        self.c = torch.empty_like(self.a)
        for i in range(4):
            if i == 1:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
            torch.mm(self.a, self.a, out=self.c)
        ev[1].record()
        torch.cuda.synchronize()
        self.unit_ms = ev[0].elapsed_time(ev[1]) / 3

    def window(self, fn, steps, plug_ms):
        """(device-side ms per call, host ms per call) of ``steps`` calls of ``fn`` behind ``plug_ms`` of plug"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(int(plug_ms / self.unit_ms) + 1 if plug_ms else 0):
            torch.mm(self.a, self.a, out=self.c)
        t0 = time.perf_counter()
        ev[0].record()
        for _ in range(steps):
            fn()
        ev[1].record()
        host_ms = (time.perf_counter() - t0) * 1e3 / steps
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / steps, host_ms


def _measure(routes, a, emit, model_bytes, baseline=None, extra=None):
    plug = _Plug(torch.device("cuda", torch.cuda.current_device()))
    for fn in routes.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times, device_times = {k: [] for k in routes}, {k: [] for k in routes}
    for r in range(a.rounds):
        for name, fn in routes.items():
            ms, host_ms = plug.window(fn, a.steps, 0)
            dev_ms, _ = plug.window(fn, a.steps, 1.5 * host_ms * a.steps + 5)
            times[name].append(ms)
            device_times[name].append(dev_ms)
            emit(dict(route=name, round=r, ms=round(ms, 4), host_ms=round(host_ms, 4), device_ms=round(dev_ms, 4),
                      model_gb_per_s=round(model_bytes / dev_ms / 1e6, 1)))
    summary = {}
    for name in routes:
        med, dmed = statistics.median(times[name]), statistics.median(device_times[name])
        rec = dict(route=name, summary="median of %d rounds" % a.rounds, ms=round(med, 4), min_ms=round(min(times[name]), 4),
                   max_ms=round(max(times[name]), 4), device_ms=round(dmed, 4), min_device_ms=round(min(device_times[name]), 4),
                   max_device_ms=round(max(device_times[name]), 4), model_gb_per_s=round(model_bytes / dmed / 1e6, 1))
        if baseline in routes:
            rec.update(time_vs_baseline=round(med / statistics.median(times[baseline]), 3),
                       device_time_vs_baseline=round(dmed / statistics.median(device_times[baseline]), 3), baseline=baseline)
        if extra:
            rec.update(extra(name))
        summary[name] = rec
    return summary


def single(a, emit):
    dev = torch.device("cuda:0")
    host = _host_tensors()
    n = sum(t.numel() for t in host)
    grad_sets = _grad_sets(host, dev)
    emit(dict(what="data_parallel_bench", device=torch.cuda.get_device_name(0), torch=torch.__version__, tensors=len(host), elements=n,
              small_tensors=sum(t.numel() <= 1024 for t in host), rounds=a.rounds, steps=a.steps, warmup=a.warmup))

    # pack alone: the table of gradient set 0, uploaded once
    arrays = hip.optim.GradPackArrays([g.numel() for g in grad_sets[0]])
    for i, g in enumerate(grad_sets[0]):
        arrays.src[i] = g.data_ptr()
    nbytes, n_chunks = hip.optim.grad_pack_table_bytes(arrays)
    table_host = torch.empty(nbytes, dtype=torch.uint8)
    hip.optim.grad_pack_table_build(table_host, arrays)
    table = table_host.to(dev)
    flat = torch.zeros(arrays.flat_elems, dtype=torch.float32, device=dev)

    net = DataParallel(_Params([t.to(dev) for t in host]))
    count = [0, 0]

    def reduce():
        for p, g in zip(net.module.ps, grad_sets[count[0] % 2]):
            p.grad = g
        count[0] += 1
        net.reduce_gradients()

    fresh = [torch.nn.Parameter(t.to(dev)) for t in host]
    opt_fresh = Adam(fresh, LR, max_grad_norm=MAX_NORM)

    def adam_fresh():
        for p, g in zip(fresh, grad_sets[count[1] % 2]):
            p.grad = g
        count[1] += 1
        opt_fresh.step()

    reduce()   # the views exist from here on; adam_views steps over them as they are
    opt_views = Adam(net.parameters(), LR, max_grad_norm=MAX_NORM)
    routes = {"pack": lambda: hip.optim.grad_pack(table, arrays.n, n_chunks, flat, 0.5),
              "cat": lambda: torch.cat([g.reshape(-1) for g in grad_sets[0]]),
              "reduce": reduce, "adam_fresh": adam_fresh, "adam_views": opt_views.step}
    uploads = {"adam_fresh": lambda: opt_fresh.table_uploads, "adam_views": lambda: opt_views.table_uploads,
               "reduce": lambda: net.pack_table_uploads}
    summary = _measure(routes, a, emit, 8 * n, baseline="cat",
                       extra=lambda name: {"table_uploads": uploads[name]()} if name in uploads else {})
    for name in ("adam_fresh", "adam_views"):   # their own comparison; the 8 bytes-per-element model is the pack's
        for k in ("time_vs_baseline", "device_time_vs_baseline", "baseline", "model_gb_per_s"):
            summary[name].pop(k)
    summary["adam_views"].update(time_vs_adam_fresh=round(summary["adam_views"]["ms"] / summary["adam_fresh"]["ms"], 3),
                                 device_time_vs_adam_fresh=round(summary["adam_views"]["device_ms"] / summary["adam_fresh"]["device_ms"], 3))
    for rec in summary.values():
        emit(rec)


def _rank(rank, world, port, backend, a, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from centerpose_amd import distributed as cpd

    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    cpd.init_from_env(backend)
    host = _host_tensors()
    n = sum(t.numel() for t in host)
    grad_sets = _grad_sets(host, dev)
    net = DataParallel(_Params([t.to(dev) for t in host]))
    opt = Adam(net.parameters(), LR, max_grad_norm=MAX_NORM)
    count = [0]

    def step():
        for p, g in zip(net.module.ps, grad_sets[count[0] % 2]):
            p.grad = g
        count[0] += 1
        net.reduce_gradients()
        opt.step()

    lines = []
    routes = {"all_reduce": lambda: cpd.all_reduce_sum(net.flat, net.group), "reduce_and_step": step}
    summary = _measure(routes, a, lines.append, 8 * n)
    for rec in summary.values():
        rec.update(rank=rank, comm_path=net.comm_path, flat_mb=round(4 * net.flat_elems / 1e6, 1))
        rec.pop("model_gb_per_s")
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, [r for r in lines if "summary" not in r], list(summary.values())))


def multi(a, emit):
    import torch.multiprocessing as mp

    backend = os.environ.get("CP_BENCH_BACKEND", "nccl")
    if backend == "nccl":
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = int(os.environ.get("CP_BENCH_PORT", 36000 + os.getpid() % 2000))
    procs = [ctx.Process(target=_rank, args=(r, a.gpus, port, backend, a, q)) for r in range(a.gpus)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=900) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    emit(dict(what="data_parallel_bench", gpus=a.gpus, backend=backend, device=torch.cuda.get_device_name(0), torch=torch.__version__,
              rounds=a.rounds, steps=a.steps, warmup=a.warmup))
    for rank, lines, summary in res:
        for rec in lines:
            emit(dict(rec, rank=rank))
        for rec in summary:
            emit(rec)
    for route in ("all_reduce", "reduce_and_step"):
        recs = [rec for _, _, summary in res for rec in summary if rec["route"] == route]
        emit(dict(route=route, summary="MAX over %d ranks of the per-rank medians" % a.gpus, ms=max(r["ms"] for r in recs),
                  device_ms=max(r["device_ms"] for r in recs), comm_path=recs[0]["comm_path"], flat_mb=recs[0]["flat_mb"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    (single if a.gpus == 1 else multi)(a, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
