"""The up-sampling layers under training: deconv.conv_transpose2d (cp_conv_transpose2d_dw_nhwc / cp_conv_transpose2d_nhwc +
cp_conv_transpose2d_backward_nhwc) next to F.conv_transpose2d under torch autograd, channels_last float32 tensors on the same
device, in one process (GPU).

    python tools/deconv_backward_bench.py [--batch 16] [--iters 10] [--rounds 3] [--precision f32|both]
                                          [--out profiles/deconv_backward_bench.txt]

Shapes at a 512 x 512 input: the eight depth-wise IDAUp / DLAUp layers of dla_34 (pose_dla_dcn.py:402-417) and the three dense
deconv layers of resdcn_18 (resnet_dcn.py:232-240).  Per shape one JSON line: milliseconds of the forward alone and of forward +
backward for both sides (HIP events around `iters` steps, `rounds` rounds alternating library / torch after a warm-up of both;
the median round and all rounds), their ratios, and the achieved bytes/s of a byte model against the 6.3 TB/s streaming
ceiling.  Byte model -- a model, not a measurement of traffic; the backward's time is step - forward:
    forward    x in + out written
    backward   grad_out once + x in + grad_x out  (the weight gradient's partials and the weights are small beside them)
The dense layers are contractions (16 taps x Cin x Cout per output pixel), so their fraction of the streaming ceiling says how
far they are from being memory-bound, not how good they are.  There is no speed gate: the reference time is torch's on the
same device in the same run.

``--precision both``: only the three dense layers, the operator alone (hip.ops.conv_transpose2d_backward on NHWC tensors, no
autograd, no forward) with precision "f32" and "f16x3" alternating round by round after a warm-up of both: milliseconds of each
(median round and all rounds), their ratio, what the f16x3 mask says runs in f16x3, and both modes' error against a float64
reference of one image on the CPU.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CEILING_TBS = 6.3

# (where, kind, C, H_in = W_in, f) at a 512 x 512 input
SHAPES = [("dla_up ida_0 up_1", "dw", 256, 16, 2),
          ("dla_up ida_1 up_1", "dw", 128, 32, 2), ("dla_up ida_1 up_2", "dw", 128, 32, 2),
          ("dla_up ida_2 up_1", "dw", 64, 64, 2), ("dla_up ida_2 up_2", "dw", 64, 64, 2), ("dla_up ida_2 up_3", "dw", 64, 64, 2),
          ("ida_up up_1", "dw", 64, 64, 2), ("ida_up up_2", "dw", 64, 32, 4),
          ("resdcn_18 deconv 1", "dense", 256, 16, 2), ("resdcn_18 deconv 2", "dense", 128, 32, 2),
          ("resdcn_18 deconv 3", "dense", 64, 64, 2)]


def main():
    import torch
    import torch.nn.functional as F

    from centerpose_amd import deconv

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="f32", choices=["f32", "both"],
                    help="both: the dense layers' backward operator in f32 and f16x3, alternating (nothing else is measured)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deconv_backward_bench: no HIP device (there is nothing to measure on the CPU)")
    dev = torch.device("cuda:0")
    B = a.batch

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    lines = []
    if a.precision == "both":
        from centerpose_amd import hip

        for where, kind, C, R, f in SHAPES:
            if kind != "dense":
                continue
            g = torch.Generator(device=dev).manual_seed(1)
            x = torch.randn(B, R, R, C, device=dev, generator=g)
            w = torch.randn(C, C, 4, 4, device=dev, generator=g)
            go = torch.randn(B, 2 * R, 2 * R, C, device=dev, generator=g)
            sides = {p: (lambda p=p: hip.ops.conv_transpose2d_backward(x, w, go, 2, 1, 1, precision=p)) for p in ("f32", "f16x3")}
            for fn in sides.values():
                fn()
                fn()
            rounds = {p: [] for p in sides}
            for _ in range(a.rounds):
                for p, fn in sides.items():
                    rounds[p].append(timed(fn))
            med = {p: statistics.median(v) for p, v in rounds.items()}
            # both modes against float64 autograd of the first image (grad_w of that image alone)
            x1, go1 = x[:1].permute(0, 3, 1, 2).cpu().double().requires_grad_(True), go[:1].permute(0, 3, 1, 2).cpu().double()
            w1 = w.cpu().double().requires_grad_(True)
            ref = torch.autograd.grad(F.conv_transpose2d(x1, w1, None, 2, 1), (x1, w1), go1)
            err = {}
            for p in sides:
                gx, gw = hip.ops.conv_transpose2d_backward(x[:1].contiguous(), w, go[:1].contiguous(), 2, 1, 1, precision=p)
                err[p] = {"grad_x": float((gx.permute(0, 3, 1, 2).cpu().double() - ref[0]).abs().max() / ref[0].abs().max()),
                          "grad_w": float((gw.cpu().double() - ref[1]).abs().max() / ref[1].abs().max())}
            flop = 2 * 2.0 * B * R * R * 16 * C * C     # the two contractions
            line = {"where": where, "what": "backward operator", "B": B, "C": C, "HxW_in": R,
                    "f16x3_mask": hip.ops.conv_transpose2d_backward_precision_mask(B, R, R, C, C),
                    "backward_ms": {p: round(v, 4) for p, v in med.items()},
                    "backward_ms_rounds": {p: [round(v, 4) for v in r] for p, r in rounds.items()},
                    "f16x3_over_f32": round(med["f16x3"] / med["f32"], 3),
                    "tflops": {p: round(flop / (v * 1e-3) / 1e12, 1) for p, v in med.items()},
                    "max_rel_err_vs_float64_one_image": err}
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
            del x, w, go, sides
            torch.cuda.empty_cache()
    for where, kind, C, R, f in SHAPES if a.precision == "f32" else ():
        g = torch.Generator(device=dev).manual_seed(1)
        cl = lambda t: t.contiguous(memory_format=torch.channels_last)
        groups, k, pad = (C, 2 * f, f // 2) if kind == "dw" else (1, 4, 1)
        x = cl(torch.randn(B, C, R, R, device=dev, generator=g)).requires_grad_(True)
        w = torch.randn(C, C // groups, k, k, device=dev, generator=g).requires_grad_(True)
        go = cl(torch.randn(B, C, f * R, f * R, device=dev, generator=g))
        sides = {"library": lambda: deconv.conv_transpose2d(x, w, f, pad, groups),
                 "torch": lambda: F.conv_transpose2d(x, w, None, f, pad, groups=groups)}

        def forward(side):
            with torch.no_grad():
                sides[side]()

        def step(side):
            x.grad = w.grad = None
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
        step("library")
        gl = [t.grad.clone() for t in (x, w)]
        step("torch")
        diff = max(float((p - t.grad).abs().max() / t.grad.abs().max()) for p, t in zip(gl, (x, w)))
        X, G = B * C * R * R * 4, B * C * f * R * f * R * 4
        mf = {s: statistics.median(v) for s, v in fwd.items()}
        ms = {s: statistics.median(v) for s, v in full.items()}
        tbs = lambda nbytes, t_ms: round(nbytes / (max(t_ms, 1e-6) * 1e-3) / 1e12, 3)
        line = {"where": where, "kind": kind, "B": B, "C": C, "HxW_in": R, "f": f, "x_MiB": round(X / 2 ** 20, 1),
                "grad_out_MiB": round(G / 2 ** 20, 1),
                "forward_ms": {s: round(mf[s], 4) for s in sides}, "forward_library_over_torch": round(mf["library"] / mf["torch"], 2),
                "step_ms": {s: round(ms[s], 4) for s in sides}, "step_library_over_torch": round(ms["library"] / ms["torch"], 2),
                "backward_ms": {s: round(ms[s] - mf[s], 4) for s in sides},
                "backward_library_over_torch": round((ms["library"] - mf["library"]) / max(ms["torch"] - mf["torch"], 1e-6), 2),
                "forward_model_TBps": {s: tbs(X + G, mf[s]) for s in sides},
                "backward_model_TBps": {s: tbs(G + 2 * X, ms[s] - mf[s]) for s in sides},
                "backward_library_frac_ceiling": round(tbs(G + 2 * X, ms["library"] - mf["library"]) / CEILING_TBS, 3),
                "forward_ms_rounds": {s: [round(v, 4) for v in fwd[s]] for s in sides},
                "step_ms_rounds": {s: [round(v, 4) for v in full[s]] for s in sides}, "max_rel_grad_diff": diff}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        del x, w, go, sides
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
