"""Training the dlav1_34 tracking network on the library: the two operators it added (the ConvGRU's gate arithmetic, GroupNorm +
ReLU) next to torch's own operators, and one step of centerpose_amd.pose_net_gru.PoseNetGRU, in one process (GPU).

    python tools/pose_net_gru_bench.py [--batch 16] [--size 512] [--iters 3] [--rounds 3] [--skip-step] [--out profiles/pose_net_gru_bench.txt]

1. ``gate``: forward + backward of the GRU gate at M = batch x (size / 4)^2 rows, Ch = 64, with and without the hidden side
   (step 0).  ``library``: conv_gru.gru_gate (cp_gru_gate_forward / _backward).  ``torch``: the same arithmetic as torch eager
   operators under autograd (sigmoid, tanh, mul, add on channel slices), channels_last on both sides.
   Byte model: forward 4 M 8 Ch, backward 4 M 15 Ch (step 0: 4 Ch and 7 Ch).
2. ``groupnorm``: forward + backward of GroupNorm(32, head_conv) + ReLU at [batch, head_conv, size / 4, size / 4].  ``library``:
   group_norm.group_norm(relu=True).  ``torch``: F.relu(F.group_norm(...)), channels_last input.
   Byte model: forward 3 tensor passes (x by the statistics; x and y by the apply pass), backward 5 (x and grad_out by the
   reduction; x, grad_out and grad_x by the apply pass); the ReLU's gate adds a read of y to both backward passes (7), which the
   model leaves out, so the achieved figure of the fused layer is conservative.
3. ``step``: forward + backward of PoseNetGRU (random linear loss on the head maps) at ``size`` x ``size``, with the time split
   per operator family (every ``centerpose_amd.hip`` call of the step bracketed by HIP events); what is left of the step's wall
   time is torch glue (cat, autograd's adds of grad_x3 across the GRU steps, layout copies, the loss).

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

FAMILIES = {"conv2d_nhwc": "conv fwd", "conv2d_backward": "conv bwd", "conv2d_stem_backward": "stem bwd",
            "batch_norm_forward": "bn fwd", "batch_norm_backward": "bn bwd", "max_pool2d_forward": "pool fwd",
            "max_pool2d_backward": "pool bwd", "conv_transpose2d_dw": "up fwd", "conv_transpose2d_backward": "up bwd",
            "dcn_v2_forward": "dcn fwd", "dcn_v2_backward": "dcn bwd", "group_norm_forward": "gn fwd",
            "group_norm_backward": "gn bwd", "gru_gate_forward": "gate fwd", "gru_gate_backward": "gate bwd"}


def _is_head_conv(w, head_conv):
    """A head's 3x3 (64 -> head_conv) or its final 1x1 (head_conv -> classes, at most 32 with the forward's tile padding)"""
    cout, cin, k = w[0], w[1], w[2]
    return (k == 3 and cin == 64 and cout == head_conv and head_conv > 128) or (k == 1 and cin == head_conv and cout <= 32)


def main():
    import torch
    import torch.nn.functional as F

    from centerpose_amd import conv_gru, group_norm, hip, synth
    from centerpose_amd.pose_net_gru import PoseNetGRU

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--head-conv", type=int, default=256)
    ap.add_argument("--skip-step", action="store_true", help="only the gate and GroupNorm measurements")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_net_gru_bench: no HIP device (there is nothing to measure on the CPU)")
    dev = torch.device("cuda:0")
    hip.set_default_precision("f32")
    B, S = a.batch, a.size
    R = S // 4
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

    cl = lambda t: t.contiguous(memory_format=torch.channels_last)

    # ---- 1. the gate ----
    Ch = 64
    for step0 in (False, True):
        g = torch.Generator(device=dev).manual_seed(1)
        x3 = cl(torch.randn(B, 3 * Ch, R, R, device=dev, generator=g)).requires_grad_(True)
        h3 = None if step0 else cl(torch.randn(B, 3 * Ch, R, R, device=dev, generator=g)).requires_grad_(True)
        hp = None if step0 else cl(torch.randn(B, Ch, R, R, device=dev, generator=g)).requires_grad_(True)
        go = cl(torch.randn(B, Ch, R, R, device=dev, generator=g))
        leaves = [t for t in (x3, h3, hp) if t is not None]

        def eager():
            xr, xz, xn = x3[:, :Ch], x3[:, Ch:2 * Ch], x3[:, 2 * Ch:]
            if step0:
                r, z = torch.sigmoid(xr), torch.sigmoid(xz)
                return (1 - z) * torch.tanh(xn)
            r, z = torch.sigmoid(xr + h3[:, :Ch]), torch.sigmoid(xz + h3[:, Ch:2 * Ch])
            n = torch.tanh(xn + r * h3[:, 2 * Ch:])
            return (1 - z) * n + z * hp

        def run(fn):
            for t in leaves:
                t.grad = None
            fn().backward(go)

        sides = OrderedDict([("library", lambda: run(lambda: conv_gru.gru_gate(x3, h3, hp))), ("torch", lambda: run(eager))])
        r = compare(sides)
        sides["library"]()
        gl = [t.grad.clone() for t in leaves]
        sides["torch"]()
        diff = max(float((p - t.grad).abs().max() / t.grad.abs().max()) for p, t in zip(gl, leaves))
        x3n, h3n, hpn, gon = (None if t is None else t.detach().permute(0, 2, 3, 1) for t in (x3, h3, hp, go))
        fwd = statistics.median([timed(lambda: hip.gru_gate_forward(x3n, h3n, hpn)) for _ in range(a.rounds)])
        bwd = statistics.median([timed(lambda: hip.gru_gate_backward(x3n, h3n, hpn, gon)) for _ in range(a.rounds)])
        M = B * R * R
        bf, bb = 4.0 * M * Ch * (4 if step0 else 8), 4.0 * M * Ch * (7 if step0 else 15)
        emit({"what": "gate", "step0": step0, "M": M, "Ch": Ch, "library_ms": round(r["library"][0], 3), "torch_ms": round(r["torch"][0], 3),
              "library_ms_rounds": [round(v, 3) for v in r["library"][1]], "torch_ms_rounds": [round(v, 3) for v in r["torch"][1]],
              "torch_over_library": round(r["torch"][0] / r["library"][0], 2), "forward_kernel_ms": round(fwd, 4),
              "backward_kernel_ms": round(bwd, 4), "forward_model_bytes": bf, "backward_model_bytes": bb,
              "forward_tb_per_s": round(bf / fwd / 1e9, 3), "backward_tb_per_s": round(bb / bwd / 1e9, 3),
              "max_rel_grad_diff_vs_torch": diff})
        del x3, h3, hp, go, leaves, sides, gl
        torch.cuda.empty_cache()

    # ---- 2. GroupNorm + ReLU ----
    C, G = a.head_conv, 32 if a.head_conv % 32 == 0 else 16
    g = torch.Generator(device=dev).manual_seed(2)
    x = cl(torch.randn(B, C, R, R, device=dev, generator=g)).requires_grad_(True)
    w = (1 + 0.5 * torch.randn(C, device=dev, generator=g)).requires_grad_(True)
    b = torch.randn(C, device=dev, generator=g).requires_grad_(True)
    go = cl(torch.randn(B, C, R, R, device=dev, generator=g))

    def run(fn):
        x.grad = w.grad = b.grad = None
        fn().backward(go)

    sides = OrderedDict([("library", lambda: run(lambda: group_norm.group_norm(x, G, w, b, 1e-5, relu=True))),
                         ("torch", lambda: run(lambda: F.relu(F.group_norm(x, G, w, b, 1e-5))))])
    r = compare(sides)
    sides["library"]()
    gl = [t.grad.clone() for t in (x, w, b)]
    sides["torch"]()
    diff = max(float((p - t.grad).abs().max() / t.grad.abs().max()) for p, t in zip(gl, (x, w, b)))
    xn, gon = x.detach().permute(0, 2, 3, 1), go.permute(0, 2, 3, 1)
    y, mean, invstd = hip.group_norm_forward(xn, G, w.detach(), b.detach(), 1e-5, 1)
    fwd = statistics.median([timed(lambda: hip.group_norm_forward(xn, G, w.detach(), b.detach(), 1e-5, 1)) for _ in range(a.rounds)])
    bwd = statistics.median([timed(lambda: hip.group_norm_backward(xn, gon, G, mean, invstd, gamma=w.detach(), y=y))
                             for _ in range(a.rounds)])
    tensor = 4.0 * B * C * R * R
    emit({"what": "groupnorm", "B": B, "C": C, "G": G, "HxW": R, "library_ms": round(r["library"][0], 3),
          "torch_ms": round(r["torch"][0], 3), "library_ms_rounds": [round(v, 3) for v in r["library"][1]],
          "torch_ms_rounds": [round(v, 3) for v in r["torch"][1]], "torch_over_library": round(r["torch"][0] / r["library"][0], 2),
          "forward_ms": round(fwd, 4), "backward_ms": round(bwd, 4), "forward_model_bytes": 3 * tensor, "backward_model_bytes": 5 * tensor,
          "forward_tb_per_s": round(3 * tensor / fwd / 1e9, 3), "backward_tb_per_s": round(5 * tensor / bwd / 1e9, 3),
          "max_rel_grad_diff_vs_torch": diff})
    del x, w, b, go, y, gl, sides
    torch.cuda.empty_cache()

    # ---- 3. the whole step ----
    if not a.skip_step:
        heads = synth.HEADS_POSE
        net = PoseNetGRU(heads, head_conv=a.head_conv)
        net.load_state_dict(synth.make_state_dict("dlav1_34", heads, head_conv=a.head_conv))
        net = net.to(dev).train()
        x = synth.frames(B, h=S, w=S).to(dev)
        g = torch.Generator(device=dev).manual_seed(3)
        lin = {h: torch.randn(B, c, R, R, device=dev, generator=g) for h, c in heads.items()}

        def step():
            net.zero_grad(set_to_none=True)
            z = net(x)[0]
            sum((z[h] * lin[h]).sum() for h in z).backward()

        step()
        step()
        total = [timed(step) for _ in range(a.rounds)]
        # one more step with every operator call bracketed by events
        events, originals = [], {}

        def wrap(fname, fn):
            def inner(*args, **kw):
                fam = FAMILIES[fname]
                if fname == "conv2d_nhwc" and args[0].shape[3] == 4 and args[1].shape[2] == 7:
                    fam = "stem fwd"
                elif fname in ("conv2d_nhwc", "conv2d_backward") and args[1].shape[0] == 192:
                    fam = "gru " + fam          # the ConvGRU's two fused 64 -> 192 convolutions
                elif fname in ("conv2d_nhwc", "conv2d_backward") and _is_head_conv(tuple(args[1].shape), a.head_conv):
                    fam = "head " + fam
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(*args, **kw)
                e1.record()
                events.append((fam, e0, e1))
                return out
            return inner

        for fname in FAMILIES:
            originals[fname] = getattr(hip, fname)
            setattr(hip, fname, wrap(fname, originals[fname]))
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            step()
            e1.record()
            torch.cuda.synchronize()
        finally:
            for fname, fn in originals.items():
                setattr(hip, fname, fn)
        split, calls = OrderedDict(), OrderedDict()
        for fam, s0, s1 in events:
            split[fam] = split.get(fam, 0.0) + s0.elapsed_time(s1)
            calls[fam] = calls.get(fam, 0) + 1
        traced = e0.elapsed_time(e1)
        split["torch glue and launch gaps"] = traced - sum(split.values())
        emit({"what": "step", "arch": "dlav1_34", "B": B, "HxW": S, "head_conv": a.head_conv, "step_ms": round(statistics.median(total), 2),
              "step_ms_rounds": [round(v, 2) for v in total], "images_per_s": round(B / statistics.median(total) * 1e3, 1),
              "traced_step_ms": round(traced, 2), "family_ms": {k: round(v, 2) for k, v in split.items()}, "family_calls": calls,
              "peak_memory_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
