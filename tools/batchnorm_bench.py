"""The backbones' BatchNorm -> residual add -> ReLU chains under training: norm.batch_norm(x, ..., residual, relu=True)
(cp_batchnorm_forward_nhwc + cp_batchnorm_backward_nhwc) next to torch.relu(F.batch_norm(x, ...) + residual) under torch
autograd, channels_last float32 tensors on the same device, in one process (GPU).

    python tools/batchnorm_bench.py [--batch 16] [--iters 10] [--rounds 3] [--out profiles/batchnorm_bench.txt]

Shapes: every distinct (C, H, W) a BatchNorm of dla_34 sees at a 512 x 512 input: the base layer and levels 0-5, and the
projection / node layers of DLAUp and IDAUp.  Per shape one JSON line: milliseconds of the forward alone and of forward +
backward for both sides (HIP events around `iters` steps, `rounds` rounds alternating library / torch after a warm-up of
both; the median round and all rounds), their ratios, and the achieved bytes/s of a byte model against the 6.3 TB/s streaming
ceiling.  Byte model, in units of the activation's bytes T = B*C*H*W*4 -- a model, not a measurement of traffic:
    forward    library 4 T (x twice, residual once, y once)          torch 8 T (BN 3 T incl. its statistics pass, add 3 T, ReLU 2 T)
    backward   library 8 T (reduce: x, grad_out, y; apply: the same  torch 8 T (ReLU 3 T, BN backward 5 T; the add's backward
               three in, grad_x and grad_residual out)                      moves nothing)
There is no speed gate: the reference time is torch's on the same device in the same run.

    python tools/batchnorm_bench.py --sync [--out profiles/sync_batchnorm_bench.txt]

SyncBatchNorm's four device phases (hip.sync_norm: stats, forward, backward_reduce, backward_apply) next to the plain operator
(hip.batch_norm_forward + hip.batch_norm_backward) on the same shapes, one GPU, NO collective: the records and sums of 1 and
of 8 ranks are built by hand, this rank's own repeated.  Same timing scheme, the three sides alternating.  What it shows is
the device cost the phases add to a step (the merge launches); what the two all-gathers per layer cost is not in it.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CEILING_TBS = 6.3
FWD_T = {"library": 4, "torch": 8}
STEP_T = {"library": 12, "torch": 16}

# (where, C, H = W) at a 512 x 512 input
DLA34_512 = [("base / level0", 16, 512), ("level1", 32, 256), ("level2, ida node", 64, 128), ("level3, dla_up node", 128, 64),
             ("level4, dla_up node", 256, 32), ("level5", 512, 16), ("dla_up proj", 256, 16), ("dla_up proj", 128, 32),
             ("dla_up / ida proj", 64, 64), ("ida proj", 64, 32)]


def _timed(fn, iters):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _write(out, lines):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def sync_main(a, dev):
    """--sync: one training step of the layer (forward + backward, residual and ReLU) at the binding's level, NHWC."""
    import torch

    from centerpose_amd import hip

    S, B, lines = hip.sync_norm, a.batch, []
    for where, C, R in DLA34_512:
        g = torch.Generator(device=dev).manual_seed(1)
        x, res, go = (torch.randn(B, R, R, C, device=dev, generator=g) for _ in range(3))
        w, b = 1 + 0.5 * torch.randn(C, device=dev, generator=g), torch.randn(C, device=dev, generator=g)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)

        def plain():
            y, mean, invstd = hip.batch_norm_forward(x, w, b, res, rm, rv, True, 0.1, 1e-5, 1)
            return hip.batch_norm_backward(x, go, mean, invstd, gamma=w, y=y, need_residual_grad=True)

        def sync(world):
            records = S.stats(x).repeat(world, 1)   # the all-gather's output, by hand
            y, mean, invstd, count = S.forward(x, records, w, b, res, rm, rv, 0.1, 1e-5, 1)
            sums, gg, gb = S.backward_reduce(x, go, mean, invstd, y=y)
            return S.backward_apply(x, go, mean, invstd, count, sums.repeat(world, 1), gamma=w, y=y, need_residual_grad=True) + (gg, gb)

        sides = {"plain": plain, "sync_world1": lambda: sync(1), "sync_world8": lambda: sync(8)}
        for fn in sides.values():   # warm-up of all before anything is timed
            for _ in range(2):
                fn()
        ms = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, fn in sides.items():   # alternating
                ms[s].append(_timed(fn, a.iters))
        same = all(torch.equal(p, q) for p, q in zip(plain(), sync(1)))
        med = {s: statistics.median(v) for s, v in ms.items()}
        line = {"where": where, "B": B, "C": C, "HxW": R, "step_ms": {s: round(med[s], 4) for s in sides},
                "sync_world1_over_plain": round(med["sync_world1"] / med["plain"], 2),
                "sync_world8_over_plain": round(med["sync_world8"] / med["plain"], 2),
                "extra_us_world1": round(1e3 * (med["sync_world1"] - med["plain"]), 1),
                "extra_us_world8": round(1e3 * (med["sync_world8"] - med["plain"]), 1),
                "step_ms_rounds": {s: [round(v, 4) for v in ms[s]] for s in sides}, "world1_bitwise_plain": same}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        del x, res, go
        torch.cuda.empty_cache()
    _write(a.out, lines)


def main():
    import torch
    import torch.nn.functional as F

    from centerpose_amd import norm

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sync", action="store_true", help="time SyncBatchNorm's four phases against the plain operator")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batchnorm_bench: no HIP device (there is nothing to measure on the CPU)")
    dev = torch.device("cuda:0")
    if a.sync:
        return sync_main(a, dev)
    B = a.batch
    timed = lambda fn: _timed(fn, a.iters)
    lines = []
    for where, C, R in DLA34_512:
        g = torch.Generator(device=dev).manual_seed(1)
        cl = lambda t: t.contiguous(memory_format=torch.channels_last)
        x = cl(torch.randn(B, C, R, R, device=dev, generator=g)).requires_grad_(True)
        res = cl(torch.randn(B, C, R, R, device=dev, generator=g)).requires_grad_(True)
        go = cl(torch.randn(B, C, R, R, device=dev, generator=g))
        w = (1 + 0.5 * torch.randn(C, device=dev, generator=g)).requires_grad_(True)
        b = torch.randn(C, device=dev, generator=g).requires_grad_(True)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        sides = {"library": lambda: norm.batch_norm(x, w, b, rm, rv, True, 0.1, 1e-5, residual=res, relu=True),
                 "torch": lambda: torch.relu(F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5) + res)}

        def forward(side):
            with torch.no_grad():
                sides[side]()

        def step(side):
            x.grad = res.grad = w.grad = b.grad = None
            sides[side]().backward(go)

        for side in sides:  # warm-up of both before anything is timed
            for _ in range(2):
                forward(side)
                step(side)
        fwd, full = {s: [] for s in sides}, {s: [] for s in sides}
        for _ in range(a.rounds):
            for side in sides:  # alternating
                fwd[side].append(timed(lambda: forward(side)))
                full[side].append(timed(lambda: step(side)))
        # the two sides' gradients, compared where their ReLU gates agree (a pre-activation within rounding of zero may fall
        # on either side, and one such element moves grad_x there by its whole value); the disagreements are counted
        step("library")
        gl = [t.grad.clone() for t in (x, res, w, b)]
        step("torch")
        with torch.no_grad():
            agree = (sides["library"]() > 0) == (sides["torch"]() > 0)
        diff = max(float(((p - t.grad) * (agree if p.dim() == 4 else 1)).abs().max() / t.grad.abs().max())
                   for p, t in zip(gl, (x, res, w, b)))
        T = B * C * R * R * 4
        mf = {s: statistics.median(v) for s, v in fwd.items()}
        ms = {s: statistics.median(v) for s, v in full.items()}
        tbs = lambda units, t_ms: round(units * T / (t_ms * 1e-3) / 1e12, 2)
        line = {"where": where, "B": B, "C": C, "HxW": R, "T_MiB": round(T / 2 ** 20, 1),
                "forward_ms": {s: round(mf[s], 4) for s in sides}, "forward_library_over_torch": round(mf["library"] / mf["torch"], 2),
                "step_ms": {s: round(ms[s], 4) for s in sides}, "step_library_over_torch": round(ms["library"] / ms["torch"], 2),
                "forward_model_TBps": {s: tbs(FWD_T[s], mf[s]) for s in sides},
                "step_model_TBps": {s: tbs(STEP_T[s], ms[s]) for s in sides},
                "forward_library_frac_ceiling": round(tbs(FWD_T["library"], mf["library"]) / CEILING_TBS, 3),
                "step_library_frac_ceiling": round(tbs(STEP_T["library"], ms["library"]) / CEILING_TBS, 3),
                "forward_ms_rounds": {s: [round(v, 4) for v in fwd[s]] for s in sides},
                "step_ms_rounds": {s: [round(v, 4) for v in full[s]] for s in sides}, "max_rel_grad_diff": diff,
                "gate_disagreements": int((~agree).sum())}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        del x, res, go, w, b, sides
        torch.cuda.empty_cache()
    _write(a.out, lines)


if __name__ == "__main__":
    main()
