"""Times the optimizer step of a training step on dla_34's real parameter set (the tensors of
synth.make_state_dict("dla_34", synth.HEADS_POSE, head_conv=256): about 250 tensors, 20.25 M floats) with random gradients:

  library      centerpose_amd.optim.Adam(max_grad_norm=100.).step()                       (csrc/optim.hip: <= 3 launches)
  torch        clip_grad_norm_(params, 100.) + torch.optim.Adam(params).step()            (torch's default implementation)
  torch_fused  the same with torch.optim.Adam(params, fused=True)

each with clipping and without.  Every route owns a copy of the parameters and steps over two sets of gradients, assigned
alternately before every step (new .grad addresses each step, as after zero_grad(set_to_none=True): the library rebuilds and
uploads its table every time).  After a warm-up of each route the routes alternate round by round, and every round is
reported.  A round times --steps steps between two HIP events twice: on an idle device (ms_per_step: what a loop of nothing
but optimizer steps takes, the larger of the host's time to queue a step, host_ms_per_step, and the device's to run it), and
behind a plug of matrix products that keeps the device busy until the host has queued the whole window
(device_ms_per_step: the device time alone, which is what a training step pays when the host runs ahead of the backward).
GB/s is over the bytes the algorithm needs, 8 x 4 x N with clipping (g twice; p, m, v read and written) and 7 x 4 x N
without, whatever a route actually moves, per device_ms_per_step.  One JSON line per measurement, then one summary line
per route (medians).

  python tools/optim_bench.py [--rounds 7] [--steps 50] [--warmup 5] [--routes library,torch_fused] [--out profiles/optim_bench.txt]
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

from centerpose_amd import synth  # noqa: E402
from centerpose_amd.optim import Adam  # noqa: E402

MAX_NORM = 100.0
LR = 1.25e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--routes", default="library,torch,torch_fused", help="comma-separated subset, library first")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = synth.make_state_dict("dla_34", synth.HEADS_POSE, head_conv=256)
    host = [v.float() for k, v in sd.items() if v.is_floating_point() and "running_" not in k]
    n = sum(t.numel() for t in host)
    gen = torch.Generator().manual_seed(5)
    grad_sets = [[(1e-3 * torch.randn(t.shape, generator=gen)).to(dev) for t in host] for _ in range(2)]
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    emit(dict(what="optim_bench", device=torch.cuda.get_device_name(0), torch=torch.__version__, tensors=len(host), elements=n,
              small_tensors=sum(t.numel() <= 1024 for t in host), rounds=a.rounds, steps=a.steps, warmup=a.warmup, max_norm=MAX_NORM))

    # the plug: matrix products queued ahead of a timed window keep the device busy while the host queues the window's steps
    plug_a = torch.randn(4096, 4096, device=dev)
    plug_c = torch.empty_like(plug_a)
    for i in range(4):
        if i == 1:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
        torch.mm(plug_a, plug_a, out=plug_c)
    ev[1].record()
    torch.cuda.synchronize()
    plug_unit_ms = ev[0].elapsed_time(ev[1]) / 3

    for clip in (True, False):
        routes = {}
        for name in a.routes.split(","):
            params = [torch.nn.Parameter(t.to(dev)) for t in host]
            if name == "library":
                opt = Adam(params, LR, max_grad_norm=MAX_NORM if clip else None)
            else:
                opt = torch.optim.Adam(params, LR, fused=(name == "torch_fused"))
            routes[name] = (params, opt)
        # clip_grad_norm_ scales .grad in place: the torch routes get gradient sets of their own (scaled again at every step,
        # which changes their values and not the work), so that no route changes another's input
        grads = {name: grad_sets if name == "library" or not clip else [[g.clone() for g in gs] for gs in grad_sets] for name in routes}
        count = {name: 0 for name in routes}

        def run_route(name, steps):
            params, opt = routes[name]
            for _ in range(steps):
                for p, g in zip(params, grads[name][count[name] % 2]):
                    p.grad = g
                count[name] += 1
                if clip and name != "library":
                    torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                opt.step()

        for name in routes:
            run_route(name, a.warmup)
        torch.cuda.synchronize()
        model_bytes = (8 if clip else 7) * 4 * n
        times, device_times = {name: [] for name in routes}, {name: [] for name in routes}

        def window(name, plug_ms):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for _ in range(int(plug_ms / plug_unit_ms) + 1 if plug_ms else 0):
                torch.mm(plug_a, plug_a, out=plug_c)
            t0 = time.perf_counter()
            ev[0].record()
            run_route(name, a.steps)
            ev[1].record()
            host_ms = (time.perf_counter() - t0) * 1e3 / a.steps
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) / a.steps, host_ms

        for r in range(a.rounds):
            for name in routes:
                ms, host_ms = window(name, 0)
                dev_ms, _ = window(name, 1.5 * host_ms * a.steps + 5)
                times[name].append(ms)
                device_times[name].append(dev_ms)
                emit(dict(route=name, clip=clip, round=r, ms_per_step=round(ms, 4), host_ms_per_step=round(host_ms, 4),
                          device_ms_per_step=round(dev_ms, 4), model_gb_per_s=round(model_bytes / dev_ms / 1e6, 1)))
        for name in routes:
            med, dmed = statistics.median(times[name]), statistics.median(device_times[name])
            rec = dict(route=name, clip=clip, summary="median of %d rounds" % a.rounds, ms_per_step=round(med, 4),
                       min_ms=round(min(times[name]), 4), max_ms=round(max(times[name]), 4), device_ms_per_step=round(dmed, 4),
                       min_device_ms=round(min(device_times[name]), 4), max_device_ms=round(max(device_times[name]), 4),
                       model_gb_per_s=round(model_bytes / dmed / 1e6, 1))
            if "library" in routes:
                rec.update(time_vs_library=round(med / statistics.median(times["library"]), 2),
                           device_time_vs_library=round(dmed / statistics.median(device_times["library"]), 2))
            if name == "library":
                rec["layout_copies"] = routes[name][1].layout_copies
            emit(rec)
        del routes, grads
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
