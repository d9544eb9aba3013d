"""The prediction-head block under training: PoseHeads (cp_pose_heads_forward / _backward) next to the same block written as
nn.Sequential modules under torch autograd, on the same device, in one process (GPU).

    python tools/pose_heads_bench.py [--iters 5] [--rounds 3] [--cases dla16 dla32 resdcn32] [--out profiles/pose_heads_bench.txt]
                                     [--backward-precision f32|f16x3|both]

Cases: the dla_34 block (64 -> 256, seven heads, 128 x 128) at B = 16 and 32, the resdcn block (64 -> 64) at B = 32.  Per
case one JSON line: forward and backward milliseconds of both sides (HIP events around `iters` calls, `rounds` rounds
alternating module / torch after a warm-up of both, the median round reported and the spread next to it), the peak
torch.cuda.max_memory_allocated of one training step (forward + backward, gradients for the parameters only: the frozen
backbone) above the bytes held before the step, and the module's achieved fraction of the 157.3 TFLOP/s float32 matrix peak.
FLOP model per image and head: hidden = feat (*) w0, 2 * HW * 9 Cin * hid, once in the forward and, in the backward, again
(recomputed) plus the weight gradient of the same size (the data gradient, a third contraction of that size, only with
--feat-grad); the thin products through `classes` add 2 * HW * hid * classes each (one forward, two backward).
--backward-precision: the arithmetic of the module's backward (PoseHeads.backward_precision); "both" times the two modes as two
sides of the same module, alternating with torch in the same process after the warm-up of all three, and reports the f16x3
mode's figures under module_f16x3_* beside the float32 ones, with each mode's workspace (the library's query).
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/pose_heads_bench.py --cases dla16 --iters 2 --rounds 1`.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from centerpose_amd import hip, synth  # noqa: E402
from centerpose_amd.pose_heads import PoseHeads  # noqa: E402

PEAK_TF = 157.3
CASES = {"dla16": ("dla_34 64->256 x7 @128", 16, 64, 256, 128), "dla32": ("dla_34 64->256 x7 @128", 32, 64, 256, 128),
         "resdcn32": ("resdcn 64->64 x7 @128", 32, 64, 64, 128)}


def flops(B, HW, Cin, hid, classes, feat_grad):
    wide = 2.0 * HW * 9 * Cin * hid
    thin = sum(2.0 * HW * hid * c for c in classes)
    n = len(classes)
    fwd = B * (n * wide + thin)
    bwd = B * (n * wide * (3 if feat_grad else 2) + 2 * thin)
    return fwd, bwd


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=list(CASES))
    ap.add_argument("--feat-grad", action="store_true", help="also ask for the feature map's gradient (trainable backbone)")
    ap.add_argument("--precision", default="f32", choices=sorted(hip.PRECISIONS))
    ap.add_argument("--backward-precision", default="f32", choices=sorted(hip.PRECISIONS) + ["both"],
                    help="arithmetic of the module's backward; both: the two modes alternate in one process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_heads_bench: no HIP device (there is nothing to measure on the CPU)")
    dev = torch.device("cuda:0")
    hip.set_default_precision(a.precision)
    heads = synth.HEADS_POSE
    classes = list(heads.values())
    lines = []
    for key in a.cases:
        name, B, Cin, hid, R = CASES[key]
        torch.manual_seed(0)
        mod = PoseHeads(heads, Cin, hid).to(dev)
        ref = nn.ModuleDict({h: nn.Sequential(nn.Conv2d(Cin, hid, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(hid, c, 1))
                             for h, c in heads.items()}).to(dev)
        ref.load_state_dict(mod.state_dict())
        g = torch.Generator(device=dev).manual_seed(1)
        feat = torch.relu(torch.randn(B, Cin, R, R, device=dev, generator=g)).contiguous(memory_format=torch.channels_last)
        feat.requires_grad_(a.feat_grad)
        gos = [torch.randn(B, c, R, R, device=dev, generator=g) for c in classes]
        # the module's sides: "module" is the float32 backward unless f16x3 alone is asked for; "module_f16x3" exists with `both`
        modes = {"module": "f16x3" if a.backward_precision == "f16x3" else "f32"}
        if a.backward_precision == "both":
            modes["module_f16x3"] = "f16x3"

        def run_module(mode):
            mod.backward_precision = mode  # read at the forward, carried into that graph's backward
            return list(mod(feat).values())

        sides = {k: (lambda m=m: run_module(m)) for k, m in modes.items()}
        sides["torch"] = lambda: [ref[h](feat) for h in heads]
        params = {k: list(mod.parameters()) for k in modes}
        params["torch"] = list(ref.parameters())
        res = {k: {"fwd": [], "bwd": []} for k in sides}
        mem = {}

        def step(side, time_it):
            for p in params[side]:
                p.grad = None
            if feat.grad is not None:
                feat.grad = None
            if not time_it:
                outs = sides[side]()
                torch.autograd.backward(outs, gos)
                return None
            tf = timed(lambda: sides[side](), a.iters)
            outs = sides[side]()
            tb = timed(lambda: torch.autograd.backward(outs, gos, retain_graph=True), a.iters)
            return tf, tb

        for side in sides:  # warm-up of every shape + the memory of one step, before anything is timed
            step(side, False)
            step(side, False)
            for p in params[side]:
                p.grad = None
            feat.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(side, False)
            torch.cuda.synchronize()
            mem[side] = torch.cuda.max_memory_allocated() - base
            for p in params[side]:
                p.grad = None
            feat.grad = None
        for _ in range(a.rounds):
            for side in sides:  # alternating
                tf, tb = step(side, True)
                res[side]["fwd"].append(tf)
                res[side]["bwd"].append(tb)
        with torch.no_grad():  # the two sides compute the same block
            za, zb = sides["module"](), sides["torch"]()  # (the forward does not depend on the backward's mode)
            diff = max(float((x - y).abs().max()) for x, y in zip(za, zb))
        f_fwd, f_bwd = flops(B, R * R, Cin, hid, classes, a.feat_grad)
        med = {s: {k: statistics.median(v) for k, v in r.items()} for s, r in res.items()}
        L = hip.lib()
        cls_arr = (ctypes.c_int * len(classes))(*classes)
        ws_mb = {m: round(L.cp_pose_heads_backward_prec_workspace_bytes(B, R, R, Cin, hid, len(classes), cls_arr, hip.PRECISIONS[m]) / 2 ** 20, 1)
                 for m in set(modes.values())}
        line = {"case": name, "B": B, "precision": a.precision, "backward_precision": a.backward_precision,
                "feat_grad": bool(a.feat_grad), "iters": a.iters, "rounds": a.rounds,
                "module_fwd_ms": round(med["module"]["fwd"], 3), "torch_fwd_ms": round(med["torch"]["fwd"], 3),
                "module_bwd_ms": round(med["module"]["bwd"], 3), "torch_bwd_ms": round(med["torch"]["bwd"], 3),
                "module_bwd_ms_rounds": [round(v, 3) for v in res["module"]["bwd"]],
                "torch_bwd_ms_rounds": [round(v, 3) for v in res["torch"]["bwd"]],
                "module_fwd_ms_rounds": [round(v, 3) for v in res["module"]["fwd"]],
                "torch_fwd_ms_rounds": [round(v, 3) for v in res["torch"]["fwd"]],
                "module_step_peak_mb": round(mem["module"] / 2 ** 20, 1), "torch_step_peak_mb": round(mem["torch"] / 2 ** 20, 1),
                "fwd_gflop": round(f_fwd / 1e9, 1), "bwd_gflop": round(f_bwd / 1e9, 1),
                "module_fwd_frac_f32_peak": round(f_fwd / med["module"]["fwd"] / 1e9 / PEAK_TF, 3),
                "module_bwd_frac_f32_peak": round(f_bwd / med["module"]["bwd"] / 1e9 / PEAK_TF, 3),
                "module_bwd_workspace_mb": ws_mb[modes["module"]],
                "backward_mask": hip.ops.pose_heads_backward_precision_mask(B, R, R, Cin, hid, precision=modes["module"]),
                "max_abs_forward_diff": diff}
        if "module_f16x3" in modes:
            m16 = med["module_f16x3"]
            line.update({"module_f16x3_bwd_ms": round(m16["bwd"], 3), "module_f16x3_fwd_ms": round(m16["fwd"], 3),
                         "module_f16x3_bwd_ms_rounds": [round(v, 3) for v in res["module_f16x3"]["bwd"]],
                         "module_f16x3_step_peak_mb": round(mem["module_f16x3"] / 2 ** 20, 1),
                         "module_f16x3_bwd_workspace_mb": ws_mb["f16x3"],
                         "module_f16x3_backward_mask": hip.ops.pose_heads_backward_precision_mask(B, R, R, Cin, hid),
                         "f16x3_over_f32_bwd": round(m16["bwd"] / med["module"]["bwd"], 3),
                         "module_f16x3_bwd_frac_f32_peak": round(f_bwd / m16["bwd"] / 1e9 / PEAK_TF, 3)})
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        del mod, ref, feat, gos, sides, params
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
