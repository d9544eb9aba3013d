"""The backbones' ordinary convolutions under training: conv.conv2d (cp_conv2d_nhwc + cp_conv2d_backward_nhwc) next to
torch.nn.functional.conv2d under torch autograd, channels_last float32 tensors on the same device, in one process (GPU).

    python tools/conv_backward_bench.py [--batch 16] [--iters 5] [--rounds 3] [--nets dla_34 resdcn_18 dla_34_lowc] [--layers level2.] [--out profiles/conv_backward_bench.txt]

Shapes: every distinct convolution geometry of dla_34 at a 512 x 512 input (levels 2-5: the BasicBlock 3x3 pairs, the 1x1
projects and Roots; the 3x3 C -> 27 conv_offset_mask of the DLAUp / IDAUp deformable layers) and of resdcn_18 (the residual
3x3s, the 1x1 stride-2 down-samples, the offset convolutions of the three up-sampling stages).  The 3-channel stems are left
out (the stem is outside the operator).  dla_34's 16-channel levels 0-1 (16 -> 16 at 512 x 512 and 16 -> 32, stride 2, from 512 x
512: the operator's low-channel path) are a list of their own, `--nets dla_34_lowc`, which a run without --nets leaves out.
Per shape one JSON line: forward + backward milliseconds of both sides (HIP events around `iters` steps, `rounds` rounds
alternating library / torch after a warm-up of both; the median round and all rounds), their ratio, and the library's achieved
fraction of the 157.3 TFLOP/s float32 matrix peak.  FLOP model: 2 * B*Ho*Wo * K*K*Cin * Cout per contraction, one in the
forward and two in the backward (weight gradient, data gradient).  There is no speed gate: the reference time is torch's on the
same device in the same run.  Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/conv_backward_bench.py --iters 2
--rounds 1`.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_TF = 157.3

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
NETS = {"dla_34": DLA34_512, "resdcn_18": RESDCN18_512, "dla_34_lowc": DLA34_LOWC_512}
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
    ap.add_argument("--precision", default="f32", choices=sorted(hip.PRECISIONS), help="of the forward (the backward is float32)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_backward_bench: no HIP device (there is nothing to measure on the CPU)")
    dev = torch.device("cuda:0")
    hip.set_default_precision(a.precision)
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
            sides = {"library": lambda: conv.conv2d(x, w, b, stride, pad), "torch": lambda: F.conv2d(x, w, b, stride, pad)}

            def step(side):
                x.grad = w.grad = b.grad = None
                sides[side]().backward(go)

            for side in sides:  # warm-up of both before anything is timed
                step(side)
                step(side)
            res = {s: [] for s in sides}
            for _ in range(a.rounds):
                for side in sides:  # alternating
                    res[side].append(timed(lambda: step(side)))
            step("library")
            gl = [t.grad.clone() for t in (x, w, b)]
            step("torch")
            diff = max(float((p - t.grad).abs().max() / t.grad.abs().max()) for p, t in zip(gl, (x, w, b)))
            med = {s: statistics.median(v) for s, v in res.items()}
            fl = 3 * contraction_flops(B, Cin, Cout, R, k, stride)
            line = {"net": net, "layer": name, "B": B, "Cin": Cin, "Cout": Cout, "HxW": R, "k": k, "stride": stride,
                    "path": path,
                    "library_ms": round(med["library"], 3), "torch_ms": round(med["torch"], 3),
                    "library_over_torch": round(med["library"] / med["torch"], 2),
                    "library_ms_rounds": [round(v, 3) for v in res["library"]], "torch_ms_rounds": [round(v, 3) for v in res["torch"]],
                    "step_gflop": round(fl / 1e9, 2), "library_frac_f32_peak": round(fl / med["library"] / 1e9 / PEAK_TF, 3),
                    "max_rel_grad_diff": diff}
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
            del x, w, b, go, sides
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
