"""The backbones' ordinary convolutions under training: conv.conv2d (cp_conv2d_nhwc + cp_conv2d_backward[_prec]_nhwc) next to
torch.nn.functional.conv2d under torch autograd, channels_last float32 tensors on the same device, in one process (GPU).

    python tools/conv_backward_bench.py [--batch 16] [--iters 5] [--rounds 3] [--nets dla_34 resdcn_18 dla_34_lowc hourglass]
        [--layers level2.] [--precision f32|f16x3|both] [--out profiles/conv_backward_bench.txt]

Shapes: every distinct convolution geometry of dla_34 at a 512 x 512 input (levels 2-5: the BasicBlock 3x3 pairs, the 1x1
projects and Roots; the 3x3 C -> 27 conv_offset_mask of the DLAUp / IDAUp deformable layers) and of resdcn_18 (the residual
3x3s, the 1x1 stride-2 down-samples, the offset convolutions of the three up-sampling stages).  The 3-channel stems are left
out (the stem is outside the operator).  dla_34's 16-channel levels 0-1 (16 -> 16 at 512 x 512 and 16 -> 32, stride 2, from 512 x
512: the operator's low-channel path) are a list of their own, `--nets dla_34_lowc`, and so are the hourglass's wide residual
layers (256 to 512 channels at 128 x 128 down to 4 x 4), `--nets hourglass`; a run without --nets leaves both out.
Per shape one JSON line: forward + backward milliseconds of both sides (HIP events around `iters` steps, `rounds` rounds
alternating library / torch after a warm-up of both; the median round and all rounds), their ratio, and the library's achieved
fraction of the 157.3 TFLOP/s float32 matrix peak.  FLOP model: 2 * B*Ho*Wo * K*K*Cin * Cout per contraction, one in the
forward and two in the backward (weight gradient, data gradient).  There is no speed gate: the reference time is torch's on the
same device in the same run.  Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/conv_backward_bench.py --iters 2
--rounds 1`.

--precision is the backward's (conv.conv2d's backward_precision; --forward-precision the forward's).  With `both` the two modes
alternate in the same rounds, and the line also carries the backward operator alone (hip.ops.conv2d_backward_prec on the same tensors,
ungated, all three gradients) in both modes: bwd_f32_ms, bwd_f16x3_ms, their ratio, which contractions the f16x3 mode takes
(f16x3_mask: bit 0 weight gradient, bit 1 data gradient) and both times as fractions of the 833 TFLOP/s f16x3 ceiling (three
binary16 matrix instructions per product block; two contractions).  The float32 figures of such a run are its baseline.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_TF = 157.3
PEAK_F16X3_TF = 833.0

# (name, Cin, Cout, input H = W, kernel, stride); padding = kernel // 2
DLA34_512 = [
    ("level2.tree1.conv1", 32, 64, 256, 3, 2), ("level2.conv3x3", 64, 64, 128, 3, 1), ("level2.project", 32, 64, 128, 1, 1),
    ("level2.root", 128, 64, 128, 1, 1),
    ("level3.tree1.conv1", 64, 128, 128, 3, 2), ("level3.conv3x3", 128, 128, 64, 3, 1), ("level3.project", 64, 128, 64, 1, 1),
    ("level3.tree1.root", 256, 128, 64, 1, 1), ("level3.tree2.root", 448, 128, 64, 1, 1),
    ("level4.tree1.conv1", 128, 256, 64, 3, 2), ("level4.conv3x3", 256, 256, 32, 3, 1), ("level4.project", 128, 256, 32, 1, 1),
    ("level4.tree1.root", 512, 256, 32, 1, 1), ("level4.tree2.root", 896, 256, 32, 1, 1),
    ("level5.tree1.conv1", 256, 512, 32, 3, 2), ("level5.conv3x3", 512, 512, 16, 3, 1), ("level5.project", 256, 512, 16, 1, 1),
    ("level5.root", 1280, 512, 16, 1, 1),
    ("dcn_offset.c512", 512, 27, 16, 3, 1), ("dcn_offset.c256", 256, 27, 32, 3, 1), ("dcn_offset.c128", 128, 27, 64, 3, 1),
    ("dcn_offset.c64", 64, 27, 128, 3, 1),
]
RESDCN18_512 = [
    ("layer1.conv3x3", 64, 64, 128, 3, 1),
    ("layer2.0.conv1", 64, 128, 128, 3, 2), ("layer2.conv3x3", 128, 128, 64, 3, 1), ("layer2.0.downsample", 64, 128, 128, 1, 2),
    ("layer3.0.conv1", 128, 256, 64, 3, 2), ("layer3.conv3x3", 256, 256, 32, 3, 1), ("layer3.0.downsample", 128, 256, 64, 1, 2),
    ("layer4.0.conv1", 256, 512, 32, 3, 2), ("layer4.conv3x3", 512, 512, 16, 3, 1), ("layer4.0.downsample", 256, 512, 32, 1, 2),
    ("deconv.dcn_offset.c512", 512, 27, 16, 3, 1), ("deconv.dcn_offset.c256", 256, 27, 32, 3, 1),
    ("deconv.dcn_offset.c128", 128, 27, 64, 3, 1),
]
# dla_34's 16-channel levels 0-1: the operator's low-channel path (conv_bwd_lowc.hip); --nets dla_34_lowc
DLA34_LOWC_512 = [("level0.conv3x3", 16, 16, 512, 3, 1), ("level1.conv3x3", 16, 32, 512, 3, 2)]
# the hourglass at a 512 x 512 input (large_hourglass.py: dims 256, 256, 384, 384, 384, 512 on maps of 128 down to 4): the
# Residual 3x3s of every level, the stride-2 entries between the levels with their 1x1 skips, the widening layers of the way up
HOURGLASS_512 = [
    ("hg.l0.conv3x3", 256, 256, 128, 3, 1), ("hg.l1.entry", 256, 256, 128, 3, 2), ("hg.l1.conv3x3", 256, 256, 64, 3, 1),
    ("hg.l2.entry", 256, 384, 64, 3, 2), ("hg.l2.skip", 256, 384, 64, 1, 2), ("hg.l2.conv3x3", 384, 384, 32, 3, 1),
    ("hg.l3.entry", 384, 384, 32, 3, 2), ("hg.l3.conv3x3", 384, 384, 16, 3, 1), ("hg.l4.entry", 384, 384, 16, 3, 2),
    ("hg.l4.conv3x3", 384, 384, 8, 3, 1), ("hg.l5.entry", 384, 512, 8, 3, 2), ("hg.l5.skip", 384, 512, 8, 1, 2),
    ("hg.l5.conv3x3", 512, 512, 4, 3, 1), ("hg.l5.up", 512, 384, 4, 3, 1), ("hg.l5.up.skip", 512, 384, 4, 1, 1),
    ("hg.l2.up", 384, 256, 32, 3, 1), ("hg.l2.up.skip", 384, 256, 32, 1, 1),
]
NETS = {"dla_34": DLA34_512, "resdcn_18": RESDCN18_512, "dla_34_lowc": DLA34_LOWC_512, "hourglass": HOURGLASS_512}
PATHS = {0: "generic", 1: "mfma", 2: "lowc"}   # include/centerpose_hip.h: CP_CONV_BWD_*


def contraction_flops(B, Cin, Cout, R, k, stride):
    Ro = (R + 2 * (k // 2) - k) // stride + 1
    return 2.0 * B * Ro * Ro * k * k * Cin * Cout


def main():
    import torch
    import torch.nn.functional as F

    from centerpose_amd import conv, hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nets", nargs="+", default=["dla_34", "resdcn_18"], choices=sorted(NETS))
    ap.add_argument("--layers", nargs="+", default=None, help="only the layers whose name contains one of these (for kernel traces)")
    ap.add_argument("--precision", default="f32", choices=sorted(hip.PRECISIONS) + ["both"],
                    help="of the backward; both: the two modes alternating, and the backward operator alone in each")
    ap.add_argument("--forward-precision", default="f32", choices=sorted(hip.PRECISIONS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_backward_bench: no HIP device (there is nothing to measure on the CPU)")
    dev = torch.device("cuda:0")
    hip.set_default_precision(a.forward_precision)
    B = a.batch
    both = a.precision == "both"
    modes = ["f32", "f16x3"] if both else [a.precision]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    lines, seen = [], {}
    for net in a.nets:
        for name, Cin, Cout, R, k, stride in NETS[net]:
            if a.layers and not any(t in name for t in a.layers):
                continue
            geo = (Cin, Cout, R, k, stride)
            if geo in seen:  # a geometry both networks have is measured once
                continue
            seen[geo] = name
            pad = k // 2
            path = PATHS[hip.conv2d_backward_path(B, R, R, Cin, Cout, k, k, stride, pad)]
            g = torch.Generator(device=dev).manual_seed(1)
            x = torch.randn(B, Cin, R, R, device=dev, generator=g).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            w = (torch.randn(Cout, Cin, k, k, device=dev, generator=g) / (Cin * k * k) ** 0.5).requires_grad_(True)
            b = torch.randn(Cout, device=dev, generator=g).requires_grad_(True)
            Ro = (R + 2 * pad - k) // stride + 1
            go = torch.randn(B, Cout, Ro, Ro, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
            sides = {"library" if not both else "library_" + m: (lambda m=m: conv.conv2d(x, w, b, stride, pad, backward_precision=m))
                     for m in modes}
            sides["torch"] = lambda: F.conv2d(x, w, b, stride, pad)
            # the backward operator alone, on the same tensors as NHWC views
            xn, gn, wd = x.detach().permute(0, 2, 3, 1), go.permute(0, 2, 3, 1), w.detach()
            if both:
                for m in modes:
                    sides["bwd_" + m] = (lambda m=m: hip.ops.conv2d_backward_prec(xn, wd, gn, stride=stride, pad=pad, precision=m))

            def step(side):
                if side.startswith("bwd_"):
                    sides[side]()
                    return
                x.grad = w.grad = b.grad = None
                sides[side]().backward(go)

            for side in sides:  # warm-up of all before anything is timed
                step(side)
                step(side)
            res = {s: [] for s in sides}
            for _ in range(a.rounds):
                for side in sides:  # alternating
                    res[side].append(timed(lambda: step(side)))
            lib = "library" if not both else "library_" + modes[-1]
            step(lib)
            gl = [t.grad.clone() for t in (x, w, b)]
            step("torch")
            diff = max(float((p - t.grad).abs().max() / t.grad.abs().max()) for p, t in zip(gl, (x, w, b)))
            med = {s: statistics.median(v) for s, v in res.items()}
            fl = 3 * contraction_flops(B, Cin, Cout, R, k, stride)
            line = {"net": net, "layer": name, "B": B, "Cin": Cin, "Cout": Cout, "HxW": R, "k": k, "stride": stride,
                    "path": path, "backward_precision": a.precision}
            for s in sides:
                line[s + "_ms"] = round(med[s], 3)
                line[s + "_ms_rounds"] = [round(v, 3) for v in res[s]]
            if both:
                line["f16x3_mask"] = hip.ops.conv2d_backward_precision_mask(B, R, R, Cin, Cout, k, k, stride, pad)
                line["library_f16x3_over_f32"] = round(med["library_f16x3"] / med["library_f32"], 3)
                line["library_f16x3_over_torch"] = round(med["library_f16x3"] / med["torch"], 2)
                line["library_f32_over_torch"] = round(med["library_f32"] / med["torch"], 2)
                line["bwd_f16x3_over_f32"] = round(med["bwd_f16x3"] / med["bwd_f32"], 3)
                for m in modes:
                    line["bwd_%s_frac_f16x3_peak" % m] = round(fl * 2 / 3 / med["bwd_" + m] / 1e9 / PEAK_F16X3_TF, 4)
            else:
                line["library_over_torch"] = round(med["library"] / med["torch"], 2)
                line["library_frac_f32_peak"] = round(fl / med["library"] / 1e9 / PEAK_TF, 3)
            line["step_gflop"] = round(fl / 1e9, 2)
            line["max_rel_grad_diff"] = diff
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
            del x, w, b, go, sides, xn, gn, wd
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
