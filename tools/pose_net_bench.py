"""Training the whole dla_34 network on the library: one step of centerpose_amd.pose_net.PoseNet, and the two layer families it
added (the image stems, the max-pools) next to their baselines, in one process (GPU).

    python tools/pose_net_bench.py [--batch 16] [--size 512] [--iters 3] [--rounds 3] [--skip-step] [--only-step] [--deterministic]
                                   [--backward-precision P] [--heads-backward-precision P] [--dcn-backward-precision P]
                                   [--out profiles/pose_net_bench.txt]

1. ``step``: forward + backward of PoseNet (random linear loss on the head maps) at ``size`` x ``size``, with the time split per
   layer family: every ``centerpose_amd.hip`` operator call of the step is bracketed by HIP events (stem / conv / bn / pool /
   dcn / up / heads, forward and backward apart); what is left of the step's wall time is torch glue (cat, sigmoid, the offset
   split, layout copies, the loss).  ``--deterministic`` times the step under ``hip.set_deterministic(True)`` as well (the
   DCNv2 input gradient summed in a fixed order: every gradient of the step bitwise reproducible), the two modes alternating
   round by round; the family split is then the deterministic step's.
2. ``stem``: forward + backward of the 3 -> 16 (base_layer, pre_img_layer) and 1 -> 16 (pre_hm_layer) stems, three routes:
   ``library`` (stem.stem_conv2d: 4-channel forward + cp_conv2d_stem_backward), ``torch`` (F.conv2d on the planes, weight gradient
   through torch autograd) and ``padded`` (the only route before this operator: conv.conv2d on the image padded to 4 planes,
   whose weight gradient is wgrad_generic_kernel).  None computes an input gradient.
3. ``pool``: forward + backward of the four max-pooled tensors of dla_34 (the inputs of levels 2 .. 5) on the library and with
   F.max_pool2d, channels_last on both sides.

HIP events around ``iters`` steps, ``rounds`` rounds alternating the routes after a warm-up of each; the median round and all
rounds are reported, one JSON line per measurement.  There is no speed gate: the baselines are measured in the same run.
Models: the stem's weight gradient is 2 B Ho Wo 49 Cin Cout FLOP and reads grad_out (B Ho Wo Cout floats) once; a pool step
reads x twice and grad_out once and writes out and grad_x once.
"""
import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FAMILIES = {"conv2d_nhwc": "conv fwd", "conv2d_stem_backward": "stem bwd",
            "batch_norm_forward": "bn fwd", "batch_norm_backward": "bn bwd", "max_pool2d_forward": "pool fwd",
            "max_pool2d_backward": "pool bwd", "conv_transpose2d_dw": "up fwd",
            "dcn_v2_forward": "dcn fwd", "pose_heads_forward": "heads fwd"}
# the layers reach these four through hip.ops, with a precision argument (hip.conv2d_backward, hip.pose_heads_backward and
# hip.dcn_v2_backward go through them too, so each call is bracketed once)
OPS_FAMILIES = {"conv2d_backward_prec": "conv bwd", "pose_heads_backward_prec": "heads bwd", "dcn_v2_backward": "dcn bwd",
                "conv_transpose2d_backward": "up bwd"}


def main():
    import torch
    import torch.nn.functional as F

    from centerpose_amd import conv, hip, pool, pose_heads, stem, synth
    from centerpose_amd.lib.models.networks.DCNv2 import dcn_v2
    from centerpose_amd.pose_net import PoseNet

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--head-conv", type=int, default=256)
    ap.add_argument("--skip-step", action="store_true", help="only the stem and pool measurements")
    ap.add_argument("--only-step", action="store_true", help="only the whole step")
    ap.add_argument("--deterministic", action="store_true", help="time the step under hip.set_deterministic(True) as well")
    ap.add_argument("--backward-precision", default="f32", choices=["f32", "f16x3", "both"],
                    help="of the step's conv.Conv2d layers (conv.set_backward_precision); both: the two modes alternating, "
                         "the traced step in f16x3")
    ap.add_argument("--heads-backward-precision", default="f32", choices=["f32", "f16x3"],
                    help="of the heads' backward (pose_heads.set_backward_precision) in every step but the f32 side of "
                         "--backward-precision both, which stays the all-float32 step")
    ap.add_argument("--dcn-backward-precision", default="f32", choices=["f32", "f16x3", "both"],
                    help="of the DCN layers' backward (dcn_v2.set_backward_precision); both: the step with the other two switches "
                         "as given is timed with the DCN layers in f32 and in f16x3, alternating, and traced in f16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_net_bench: no HIP device (there is nothing to measure on the CPU)")
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

    def compare(sides):
        """Warm-up of every route, then `rounds` alternating rounds -> {route: (median ms, [rounds])}"""
        for fn in sides.values():
            fn()
            fn()
        res = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, fn in sides.items():
                res[s].append(timed(fn))
        return {s: (statistics.median(v), v) for s, v in res.items()}

    # ---- 2. the stems ----
    for name, cin in () if a.only_step else (("base_layer / pre_img_layer", 3), ("pre_hm_layer", 1)):
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(B, cin, S, S, device=dev, generator=g)
        w = (torch.randn(16, cin, 7, 7, device=dev, generator=g) / (49 * cin) ** 0.5).requires_grad_(True)
        go = torch.randn(B, 16, S, S, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        x4 = F.pad(x, (0, 0, 0, 0, 0, 4 - cin)).contiguous(memory_format=torch.channels_last)
        w4 = F.pad(w.detach(), (0, 0, 0, 0, 0, 4 - cin)).requires_grad_(True)

        def run(fn, wt):
            wt.grad = None
            fn().backward(go)

        sides = OrderedDict([("library", lambda: run(lambda: stem.stem_conv2d(x, w, None, 1), w)),
                             ("torch", lambda: run(lambda: F.conv2d(x, w, None, 1, 3), w)),
                             ("padded", lambda: run(lambda: conv.conv2d(x4, w4, None, 1, 3), w4))])
        r = compare(sides)
        sides["library"]()
        gl = w.grad.clone()
        sides["torch"]()
        diff = float((gl - w.grad).abs().max() / w.grad.abs().max())
        # the backward alone (the new kernel): cp_conv2d_stem_backward on the same tensors
        gon = go.permute(0, 2, 3, 1)
        bwd = statistics.median([timed(lambda: hip.conv2d_stem_backward(x, gon, 1)) for _ in range(a.rounds)])
        fl, byt = 2.0 * B * S * S * 49 * cin * 16, 4.0 * B * S * S * (16 + cin)
        emit({"what": "stem", "layer": name, "B": B, "Cin": cin, "Cout": 16, "HxW": S,
              "library_ms": round(r["library"][0], 3), "torch_ms": round(r["torch"][0], 3), "padded_generic_ms": round(r["padded"][0], 3),
              "library_ms_rounds": [round(v, 3) for v in r["library"][1]], "torch_ms_rounds": [round(v, 3) for v in r["torch"][1]],
              "padded_generic_ms_rounds": [round(v, 3) for v in r["padded"][1]],
              "padded_over_library": round(r["padded"][0] / r["library"][0], 2), "torch_over_library": round(r["torch"][0] / r["library"][0], 2),
              "stem_backward_kernel_ms": round(bwd, 3), "stem_backward_tflops": round(fl / bwd / 1e9, 2),
              "stem_backward_gb_per_s": round(byt / bwd / 1e6, 1), "max_rel_grad_diff_vs_torch": diff})
        del x, w, go, x4, w4, sides
        torch.cuda.empty_cache()

    # ---- 3. the max-pools ----
    for name, C, R in () if a.only_step else (("level2", 32, S // 2), ("level3", 64, S // 4), ("level4", 128, S // 8),
                                              ("level5", 256, S // 16)):
        g = torch.Generator(device=dev).manual_seed(2)
        x = torch.relu(torch.randn(B, C, R, R, device=dev, generator=g)).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        go = torch.randn(B, C, R // 2, R // 2, device=dev, generator=g).contiguous(memory_format=torch.channels_last)

        def run(fn):
            x.grad = None
            fn().backward(go)

        sides = OrderedDict([("library", lambda: run(lambda: pool.max_pool2d(x, 2, 2))), ("torch", lambda: run(lambda: F.max_pool2d(x, 2, 2)))])
        r = compare(sides)
        sides["library"]()
        gl = x.grad.clone()
        sides["torch"]()
        byt = 4.0 * B * C * R * R * (2 + 1) + 4.0 * B * C * (R // 2) ** 2 * 2
        emit({"what": "pool", "layer": name + ".downsample", "B": B, "C": C, "HxW": R, "library_ms": round(r["library"][0], 3),
              "torch_ms": round(r["torch"][0], 3), "library_ms_rounds": [round(v, 3) for v in r["library"][1]],
              "torch_ms_rounds": [round(v, 3) for v in r["torch"][1]], "library_over_torch": round(r["library"][0] / r["torch"][0], 2),
              "library_gb_per_s": round(byt / r["library"][0] / 1e6, 1), "grad_bitwise_equal_torch": bool(torch.equal(gl, x.grad))})
        del x, go, sides
        torch.cuda.empty_cache()

    # ---- 1. the whole step ----
    if not a.skip_step:
        heads = synth.HEADS_POSE
        net = PoseNet(heads, head_conv=a.head_conv)
        net.load_state_dict(synth.make_state_dict("dla_34", heads, head_conv=a.head_conv))
        net = net.to(dev).train()
        x = synth.frames(B, h=S, w=S).to(dev)
        g = torch.Generator(device=dev).manual_seed(3)
        lin = {h: torch.randn(B, c, S // 4, S // 4, device=dev, generator=g) for h, c in heads.items()}

        def step():
            net.zero_grad(set_to_none=True)
            z = net(x)[0]
            sum((z[h] * lin[h]).sum() for h in z).backward()

        precs = ["f32", "f16x3"] if a.backward_precision == "both" else [a.backward_precision]
        modes = [False, True] if a.deterministic else [False]
        modes += ["f16x3"] if len(precs) == 2 else []   # (the deterministic step is timed in the first precision)
        modes += ["dcn16"] if a.dcn_backward_precision == "both" else []
        n_dcn = sum(isinstance(m, dcn_v2.DCNv2) for m in net.modules())

        def enter(m):
            hip.set_deterministic(m is True)
            conv.set_backward_precision(net, "f16x3" if m == "f16x3" else precs[0])
            heads_mode = "f32" if len(precs) == 2 and m != "f16x3" else a.heads_backward_precision
            assert pose_heads.set_backward_precision(net, heads_mode) == 1
            dcn16 = a.dcn_backward_precision == "f16x3" or m == "dcn16"
            assert dcn_v2.set_backward_precision(net, "f16x3" if dcn16 else "f32") == n_dcn > 0

        for m in modes:
            enter(m)
            step()
            step()
        rounds = {m: [] for m in modes}
        for _ in range(a.rounds):
            for m in modes:
                enter(m)
                rounds[m].append(timed(step))
        total = rounds[False]
        det = {"backward_precision": a.backward_precision, "traced_backward_precision": precs[-1],
               "heads_backward_precision": a.heads_backward_precision}
        if len(precs) == 2:
            det.update({"f16x3_step_ms": round(statistics.median(rounds["f16x3"]), 2),
                        "f16x3_step_ms_rounds": [round(v, 2) for v in rounds["f16x3"]],
                        "f16x3_over_f32": round(statistics.median(rounds["f16x3"]) / statistics.median(total), 3)})
        det["dcn_backward_precision"] = a.dcn_backward_precision
        if "dcn16" in rounds:
            det.update({"dcn_f16x3_step_ms": round(statistics.median(rounds["dcn16"]), 2),
                        "dcn_f16x3_step_ms_rounds": [round(v, 2) for v in rounds["dcn16"]],
                        "dcn_f16x3_over_dcn_f32": round(statistics.median(rounds["dcn16"]) / statistics.median(total), 3)})
        enter(True if a.deterministic else modes[-1])  # the traced step below: the deterministic mode if asked for, else the last precision
        if a.deterministic:
            det.update({"deterministic_step_ms": round(statistics.median(rounds[True]), 2),
                        "deterministic_step_ms_rounds": [round(v, 2) for v in rounds[True]],
                        "deterministic_over_default": round(statistics.median(rounds[True]) / statistics.median(total), 3),
                        "family_split_of": "deterministic step", "traced_backward_precision": precs[0]})
        # one more step with every operator call bracketed by events
        events, originals = [], {}

        def wrap(fname, fn):
            def inner(*args, **kw):
                fam = FAMILIES.get(fname) or OPS_FAMILIES[fname]
                if fname == "conv2d_nhwc" and args[0].shape[3] == 4 and args[1].shape[2] == 7:
                    fam = "stem fwd"
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(*args, **kw)
                e1.record()
                events.append((fam, e0, e1))
                return out
            return inner

        for module, table in ((hip, FAMILIES), (hip.ops, OPS_FAMILIES)):
            for fname in table:
                originals[(module, fname)] = getattr(module, fname)
                setattr(module, fname, wrap(fname, originals[(module, fname)]))
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            step()
            e1.record()
            torch.cuda.synchronize()
        finally:
            for (module, fname), fn in originals.items():
                setattr(module, fname, fn)
        split, calls = OrderedDict(), OrderedDict()
        for fam, s0, s1 in events:
            split[fam] = split.get(fam, 0.0) + s0.elapsed_time(s1)
            calls[fam] = calls.get(fam, 0) + 1
        traced = e0.elapsed_time(e1)
        split["torch glue and launch gaps"] = traced - sum(split.values())
        emit({"what": "step", "arch": "dla_34", "B": B, "HxW": S, "head_conv": a.head_conv, "step_ms": round(statistics.median(total), 2),
              "step_ms_rounds": [round(v, 2) for v in total], "images_per_s": round(B / statistics.median(total) * 1e3, 1),
              "traced_step_ms": round(traced, 2), "family_ms": {k: round(v, 2) for k, v in split.items()}, "family_calls": calls,
              "peak_memory_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), **det})
        hip.set_deterministic(False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
