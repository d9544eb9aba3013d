"""Training the stacked hourglass on the library: the two pieces it added (the kp_module merge, the 3 -> 128 stem's weight
gradient) next to torch's own operators, and one step of centerpose_amd.pose_net_hourglass.PoseNetHourglass, in one process (GPU).

    python tools/pose_net_hourglass_bench.py [--batch 8] [--size 512] [--iters 3] [--rounds 3] [--skip-step] [--out profiles/pose_net_hourglass_bench.txt]

1. ``merge``: forward + backward of ``up1 + Upsample(scale_factor=2)(low)`` on the network's five merge shapes at ``size`` x
   ``size``.  ``library``: upsample.upsample2_add (cp_upsample2_add_nhwc / _backward_nhwc).  ``torch``: ``up1 +
   F.interpolate(low, scale_factor=2)`` under autograd, channels_last on both sides.  The two kernels are also timed alone.
   ``*_ms`` is a loop of nothing but the operator (host-bound at the small shapes: a few tens of microseconds of device work
   per call); ``device_*_ms`` is the same loop queued behind a plug of matrix products, i.e. what a training step pays, where
   the host runs ahead of the device.
   Byte model per call, with [B,H,W,C] the shape of ``low``: forward 4 B C (4 H W + H W + 4 H W) (up1 and low read, out
   written), backward 4 B C (4 H W + H W) (grad_out read once, grad_low written; the gradient of up1 is grad_out itself).
2. ``stem``: forward + backward of Conv2d(3, 128, 7, stride 2, padding 3) on the image batch (weight gradient only: the input is
   an image).  ``library``: stem.stem_conv2d.  ``torch``: F.conv2d on the planes.  ``conv2d_4planes``: conv.conv2d on the image
   padded to four planes, the only route before (its weight gradient falls to the generic kernel).
3. ``step``: forward + backward of PoseNetHourglass (random linear loss on both stacks' head maps) at ``size`` x ``size``, with the
   time split per operator family (every library call of the step bracketed by HIP events; what is left of the step's wall time
   is torch glue), next to the same graph on torch's own operators in float32 (tests/hourglass_net_ref.py on the device,
   channels_last).

HIP events around ``iters`` calls, ``rounds`` rounds alternating the routes after a warm-up of each; the median round and all
rounds are reported, one JSON line per measurement.  There is no speed gate: the baselines are torch's operators, measured in
the same run.
"""
import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# function -> (module attribute it is reached through, family)
FAMILIES = {"conv2d_nhwc": "conv fwd", "conv2d_stem_backward": "stem bwd",
            "batch_norm_forward": "bn fwd", "batch_norm_backward": "bn bwd", "pose_heads_forward": "heads fwd"}
# reached through hip.ops: the two backwards with a precision argument (the layers call these; hip.conv2d_backward and
# hip.pose_heads_backward go through them too) and the merge
MERGE = {"upsample2_add_forward": "merge fwd", "upsample2_add_backward": "merge bwd", "conv2d_backward_prec": "conv bwd",
         "pose_heads_backward_prec": "heads bwd"}


def main():
    import torch
    import torch.nn.functional as F

    from centerpose_amd import conv, hip, pose_heads, stem, synth, upsample
    from centerpose_amd.hip import ops
    from centerpose_amd.pose_net_hourglass import PoseNetHourglass

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true", help="only the merge and stem measurements")
    ap.add_argument("--backward-precision", default="f32", choices=["f32", "f16x3", "both"],
                    help="of the step's conv.Conv2d layers (conv.set_backward_precision); both: the two modes alternating "
                         "(library = f32, library_f16x3), the traced step in f16x3")
    ap.add_argument("--heads-backward-precision", default="f32", choices=["f32", "f16x3"],
                    help="of the heads' backward (pose_heads.set_backward_precision) in every step but the f32 side of "
                         "--backward-precision both, which stays the all-float32 step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_net_hourglass_bench: no HIP device (there is nothing to measure on the CPU)")
    dev = torch.device("cuda:0")
    hip.set_default_precision("f32")
    B, S = a.batch, a.size
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(json.dumps(d))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    plug_a = torch.randn(8192, 8192, device=dev)

    def timed_behind_plug(fn):
        """Device time of `iters` calls: a plug of matrix products keeps the device busy while the host queues the whole window,
        so the events bracket the kernels back to back and not the host's launch rate."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        for _ in range(2):
            plug_a @ plug_a
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    def compare(sides, timer=None):
        """Warm-up of every route, then `rounds` alternating rounds -> {route: (median ms, [rounds])}"""
        timer = timer or timed
        for fn in sides.values():
            fn()
            fn()
        res = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, fn in sides.items():
                res[s].append(timer(fn))
        return {s: (statistics.median(v), v) for s, v in res.items()}

    def report(d, r):
        for s, (med, rounds) in r.items():
            d[s + "_ms"] = round(med, 4)
            d[s + "_ms_rounds"] = [round(v, 4) for v in rounds]
        for s in r:
            if s != "library":
                d[s + "_over_library"] = round(r[s][0] / r["library"][0], 2)
        emit(d)

    cl = lambda t: t.contiguous(memory_format=torch.channels_last)

    # ---- 1. the merge: the five kp_module levels (the output of level i is [B, dims[i], S / 4 / 2^i, ...]) ----
    for level, C in enumerate(synth.HG_DIMS[:5]):
        H = S // 4 // 2 ** (level + 1)
        g = torch.Generator(device=dev).manual_seed(1 + level)
        up1 = cl(torch.randn(B, C, 2 * H, 2 * H, device=dev, generator=g)).requires_grad_(True)
        low = cl(torch.randn(B, C, H, H, device=dev, generator=g)).requires_grad_(True)
        go = cl(torch.randn(B, C, 2 * H, 2 * H, device=dev, generator=g))

        def run(fn):
            up1.grad = low.grad = None
            fn().backward(go)

        sides = OrderedDict([("library", lambda: run(lambda: upsample.upsample2_add(up1, low))),
                             ("torch", lambda: run(lambda: up1 + F.interpolate(low, scale_factor=2)))])
        r = compare(sides)
        rd = compare(sides, timed_behind_plug)
        sides["library"]()
        gl = low.grad.clone()
        sides["torch"]()
        diff = float((gl - low.grad).abs().max() / low.grad.abs().max())
        un, ln, gn = (t.detach().permute(0, 2, 3, 1) for t in (up1, low, go))
        fwd = statistics.median([timed(lambda: ops.upsample2_add_forward(un, ln)) for _ in range(a.rounds)])
        bwd = statistics.median([timed(lambda: ops.upsample2_add_backward(gn, tuple(ln.shape))) for _ in range(a.rounds)])
        bf, bb = 4.0 * B * C * 9 * H * H, 4.0 * B * C * 5 * H * H
        report({"what": "merge", "low_BHWC": [B, H, H, C], "forward_kernel_ms": round(fwd, 4), "backward_kernel_ms": round(bwd, 4),
                "forward_model_bytes": bf, "backward_model_bytes": bb, "forward_tb_per_s": round(bf / fwd / 1e9, 3),
                "backward_tb_per_s": round(bb / bwd / 1e9, 3), "max_rel_grad_low_diff_vs_torch": diff,
                "device_library_ms": round(rd["library"][0], 4), "device_torch_ms": round(rd["torch"][0], 4),
                "device_library_ms_rounds": [round(v, 4) for v in rd["library"][1]],
                "device_torch_ms_rounds": [round(v, 4) for v in rd["torch"][1]],
                "device_torch_over_library": round(rd["torch"][0] / rd["library"][0], 2)}, r)
        del up1, low, go, gl, sides
        torch.cuda.empty_cache()

    # ---- 2. the stem ----
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(B, 3, S, S, device=dev, generator=g)
    x4 = torch.cat([x, x.new_zeros(B, 1, S, S)], 1)
    w = (torch.randn(128, 3, 7, 7, device=dev, generator=g) * 0.08).requires_grad_(True)
    w4 = torch.cat([w.detach(), w.new_zeros(128, 1, 7, 7)], 1).requires_grad_(True)
    go = cl(torch.randn(B, 128, S // 2, S // 2, device=dev, generator=g))

    def run(fn, leaf):
        leaf.grad = None
        fn().backward(go)

    sides = OrderedDict([("library", lambda: run(lambda: stem.stem_conv2d(x, w, None, 2), w)),
                         ("torch", lambda: run(lambda: F.conv2d(x, w, None, 2, 3), w)),
                         ("conv2d_4planes", lambda: run(lambda: conv.conv2d(x4, w4, None, 2, 3), w4))])
    r = compare(sides)
    sides["library"]()
    gl = w.grad.clone()
    sides["torch"]()
    diff = float((gl - w.grad).abs().max() / w.grad.abs().max())
    gon = go.permute(0, 2, 3, 1)
    bwd = statistics.median([timed(lambda: hip.conv2d_stem_backward(x, gon, stride=2, need_bias_grad=False)) for _ in range(a.rounds)])
    report({"what": "stem", "B": B, "HxW": S, "Cout": 128, "stride": 2, "backward_kernel_ms": round(bwd, 4),
            "max_rel_grad_w_diff_vs_torch": diff}, r)
    del x, x4, w, w4, go, gl, sides
    torch.cuda.empty_cache()

    # ---- 3. the whole step ----
    if not a.skip_step:
        from tests import hourglass_net_ref as ref

        heads = synth.HEADS_POSE
        sd = synth.make_state_dict("hourglass", heads)
        net = PoseNetHourglass(heads)
        net.load_state_dict(sd)
        net = net.to(dev).train()
        x = synth.frames(B, h=S, w=S).to(dev)
        g = torch.Generator(device=dev).manual_seed(3)
        lin = [{h: torch.randn(B, c, S // 4, S // 4, device=dev, generator=g) for h, c in heads.items()} for _ in range(2)]

        def step():
            net.zero_grad(set_to_none=True)
            zs = net(x)
            sum((z[h] * lin[k][h]).sum() for k, z in enumerate(zs) for h in z).backward()

        # the same graph on torch's own operators, float32, channels_last
        tsd = OrderedDict()
        for k, v in sd.items():
            v = v.to(dev)
            tsd[k] = (cl(v) if v.dim() == 4 else v).requires_grad_(True) if v.is_floating_point() and "running_" not in k else v
        leaves = [v for v in tsd.values() if v.requires_grad]
        xc = cl(x)

        def torch_step():
            for v in leaves:
                v.grad = None
            zs = ref.forward(tsd, xc, heads, True)
            sum((z[h] * lin[k][h]).sum() for k, z in enumerate(zs) for h in z).backward()

        modes = ["f32", "f16x3"] if a.backward_precision == "both" else [a.backward_precision]
        current = [None]

        def step_in(mode):
            def run_step():
                if current[0] != mode:
                    current[0] = mode
                    conv.set_backward_precision(net, mode)
                    heads_mode = "f32" if len(modes) == 2 and mode == "f32" else a.heads_backward_precision
                    assert pose_heads.set_backward_precision(net, heads_mode) == 1
                step()
            return run_step

        routes = OrderedDict([("library", step_in(modes[0]))])
        if len(modes) == 2:
            routes["library_f16x3"] = step_in(modes[1])
        routes["torch"] = torch_step
        r = compare(routes)
        del tsd, leaves
        step_in(modes[-1])()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        # one more step with every operator call bracketed by events (no empty_cache() ahead of it: the allocator's blocks stay,
        # so the brackets hold device work and not the host's allocations)
        events, originals = [], []

        def wrap(fam_of, fname, fn):
            def inner(*args, **kw):
                fam = fam_of[fname]
                if fname == "conv2d_nhwc" and args[0].shape[3] == 4 and args[1].shape[2] == 7:
                    fam = "stem fwd"
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(*args, **kw)
                e1.record()
                events.append((fam, e0, e1))
                return out
            return inner

        for module, table in ((hip, FAMILIES), (ops, MERGE)):
            for fname in table:
                originals.append((module, fname, getattr(module, fname)))
                setattr(module, fname, wrap(table, fname, getattr(module, fname)))
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            step()
            e1.record()
            torch.cuda.synchronize()
        finally:
            for module, fname, fn in originals:
                setattr(module, fname, fn)
        split, calls = OrderedDict(), OrderedDict()
        for fam, s0, s1 in events:
            split[fam] = split.get(fam, 0.0) + s0.elapsed_time(s1)
            calls[fam] = calls.get(fam, 0) + 1
        traced = e0.elapsed_time(e1)
        split["torch glue and launch gaps"] = traced - sum(split.values())
        report({"what": "step", "arch": "hourglass", "backward_precision": a.backward_precision, "traced_backward_precision": modes[-1],
                "heads_backward_precision": a.heads_backward_precision,
                "B": B, "HxW": S, "images_per_s": round(B / r["library"][0] * 1e3, 1),
                "traced_step_ms": round(traced, 2), "family_ms": {k: round(v, 2) for k, v in split.items()}, "family_calls": calls,
                "peak_memory_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}, r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
