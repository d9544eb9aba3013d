"""Cases, the single-process driver and the two-rank process helper of the SyncBatchNorm tests
(tests/test_sync_batchnorm_{cpu,gpu}.py).

A shard list (b_0, b_1, ...) splits a case's batch by images, one shard per rank.  The driver stands for the ranks on one GPU
with no process group: phase A per shard, the records concatenated by hand (what the all-gather delivers), phase B per shard;
the same for the backward.  The reference is tests/batchnorm_ref.py's float64 ``reference_forward`` / ``reference_backward``
on the WHOLE batch, the tolerance its ``TOL`` = 1e-4 x max |reference| per output.

A float32 emulation of the rank merge (numpy, every operation rounded to float32 in the kernels' order) stays below 6e-6 of
max |reference| on save_mean, save_invstd and grad_x on every case below, and gives 6.6e-4 on grad_x at a global n = 2 --
the ill-conditioned output that tests/test_batchnorm_gpu.py's header explains -- so n = 2 is tested in the forward only.

Measured on an MI355X, the outputs closest to TOL: grad_gamma of the x = 1000 + N(0, 1) cases, 7.5e-5 at (2,8,8,32) and
3.4e-5 at (4,33,31,128) -- save_mean is a float32 (half an ulp at 1000 is 3e-5 of the standard deviation), and that error
times sum g enters sum g (x - mean), in the plain operator as here; every other output of these cases is below 2e-5.
"""
import os
import time

import torch
import torch.multiprocessing as mp

from tests import batchnorm_ref as R

Case = R.Case
# (3,1,1,4): one value per channel on a rank, global n = 3; (5,7,9,512): two channel passes; (4,14,14,256): 2 and 5 reduction
# slabs per shard (batchnorm.hip: plan), so the ranks' local merges differ in depth
SHARDED = [(Case(3, 1, 1, 4), (1, 1, 1)), (Case(3, 1, 1, 4), (2, 1)), (Case(2, 3, 5, 20), (1, 1)), (Case(3, 9, 11, 64), (2, 1)),
           (Case(3, 37, 45, 32), (1, 1, 1)), (Case(5, 7, 9, 512), (3, 2)), (Case(4, 14, 14, 256), (1, 3))]
LARGE_MEAN_SHARDED = [(Case(2, 8, 8, 32), (1, 1)), (Case(4, 33, 31, 128), (2, 1, 1))]   # x = 1000 + N(0, 1)
N2_SHARDED = (Case(2, 1, 1, 4), (1, 1))   # global n = 2: forward only
WORLD1_CASES = [R.CASES[5], R.CASES[7], R.CASES[10]]   # (1,7,9,512), (2,128,128,16), (1,16,18,256)


def sharded_id(cs):
    return "%s_shards_%s" % (R.case_id(cs[0]), "_".join(str(b) for b in cs[1]))


def _split(t, shards):
    return list(torch.split(t, list(shards), 0))


def run_sharded(device, inp, shards, residual, act, backward=True, need_x=True, need_gamma=True, need_beta=True):
    """The ranks' calls on one device.  Returns ``(whole, per_rank)``: ``whole`` is a dict shaped like reference_forward's +
    reference_backward's on the CPU (y / grad_x / grad_residual concatenated over the shards, the statistics rank 0's,
    grad_gamma / grad_beta the SUM over the shards of the local ones); ``per_rank`` lists, per shard, the device tensors
    save_mean, save_invstd, save_count, running_mean, running_var, record, y, sums, grad_x, grad_residual, grad_gamma,
    grad_beta."""
    from centerpose_amd import hip

    S = hip.sync_norm
    dev = lambda t: t.to(device)
    xs, gos = _split(dev(R.nhwc(inp.x)), shards), _split(dev(R.nhwc(inp.go)), shards)
    rs = _split(dev(R.nhwc(inp.res)), shards) if residual else [None] * len(shards)
    gamma, beta = dev(inp.gamma), dev(inp.beta)
    ranks = [dict(record=S.stats(x)) for x in xs]
    records = torch.stack([r["record"] for r in ranks])   # the all-gather, by hand
    for r, x, res in zip(ranks, xs, rs):
        r["running_mean"], r["running_var"] = dev(inp.rmean), dev(inp.rvar)
        r["y"], r["save_mean"], r["save_invstd"], r["save_count"] = S.forward(x, records, gamma, beta, res, r["running_mean"],
                                                                              r["running_var"], R.MOMENTUM, R.EPS, act)
    whole = dict(y=R.nchw(torch.cat([r["y"] for r in ranks])).cpu())
    for k in ("save_mean", "save_invstd", "running_mean", "running_var"):
        whole[k] = ranks[0][k].cpu()
    if not backward:
        return whole, ranks
    for r, x, go in zip(ranks, xs, gos):
        r["sums"], r["grad_gamma"], r["grad_beta"] = S.backward_reduce(x, go, r["save_mean"], r["save_invstd"], y=r["y"] if act else None,
                                                                       need_gamma_grad=need_gamma, need_beta_grad=need_beta)
    sums_all = torch.stack([r["sums"] for r in ranks])
    for r, x, go in zip(ranks, xs, gos):
        r["grad_x"], r["grad_residual"] = S.backward_apply(x, go, r["save_mean"], r["save_invstd"], r["save_count"], sums_all, gamma=gamma,
                                                           y=r["y"] if act else None, need_x_grad=need_x, need_residual_grad=residual)
    cat = lambda k: R.nchw(torch.cat([r[k] for r in ranks])).cpu() if ranks[0][k] is not None else None
    tot = lambda k: sum(r[k].double() for r in ranks).cpu() if ranks[0][k] is not None else None
    whole.update(grad_x=cat("grad_x"), grad_residual=cat("grad_residual"), grad_gamma=tot("grad_gamma"), grad_beta=tot("grad_beta"))
    return whole, ranks


def check_sharded(device, inp, shards, residual, act, what, backward=True):
    """One configuration against the whole-batch reference at TOL; returns run_sharded's result."""
    whole, ranks = run_sharded(device, inp, shards, residual, act, backward)
    R.check(whole, R.reference_forward(inp, residual, act), what)
    if backward:
        R.check(whole, R.reference_backward(inp, residual, whole["y"] if act else None), what)
    return whole, ranks


# ---- two ranks ----

def run_ranks(target, *args):
    """Start ``target(rank, 2, port, queue, *args)`` in two fresh processes and return what they put on the queue, by rank
    (plain Python values and numpy arrays: they travel by value, where a tensor would travel as a handle of the child's
    memory).  One 120 s limit for both children; whatever is left then is terminated, and a child that ends with anything
    but exit code 0 fails the test at once."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37000 + (os.getpid() % 2000)
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
