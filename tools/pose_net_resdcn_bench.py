"""Training the ResNet-DCN family on the library: one step of centerpose_amd.pose_net_resdcn.PoseNetResDCN next to the same
graph on torch's operators, in one process (GPU).

    python tools/pose_net_resdcn_bench.py [--depths 18,50] [--batch 16] [--size 512] [--iters 3] [--rounds 3] [--head-conv 64]
                                          [--out profiles/pose_net_resdcn_bench.txt]

Per depth, forward + backward of a random linear loss on the head maps at ``size`` x ``size``, three sides alternating round by
round after a warm-up of each:
  ``f32``    the library with every backward in float32,
  ``f16x3``  the library with the four backward switches on (conv, deconv, pose_heads, dcn_v2 ``set_backward_precision``),
  ``torch``  the same module tree on torch's own operators: nn.Conv2d / nn.BatchNorm2d + ReLU / nn.MaxPool2d / nn.ConvTranspose2d
             in channels_last, heads as nn.Sequential; the deformable layers stay the library's DCN (torch has none), so the
             comparison is of everything else.
Then one more f16x3 step with every ``centerpose_amd.hip`` operator call bracketed by HIP events: the time per layer family
(stem / conv / bn / pool / dcn / deconv / heads, forward and backward apart); what is left of the step's wall time is torch glue
(the offset split, sigmoid, layout copies, the loss) and launch gaps.  One JSON line per depth; there is no speed gate.
"""
import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FAMILIES = {"conv2d_nhwc": "conv fwd", "conv2d_stem_backward": "stem bwd", "batch_norm_forward": "bn fwd",
            "batch_norm_backward": "bn bwd", "max_pool2d_forward": "pool fwd", "max_pool2d_backward": "pool bwd",
            "conv_transpose2d": "deconv fwd", "dcn_v2_forward": "dcn fwd", "pose_heads_forward": "heads fwd"}
# the layers reach these through hip.ops, with a precision argument
OPS_FAMILIES = {"conv2d_backward_prec": "conv bwd", "pose_heads_backward_prec": "heads bwd", "dcn_v2_backward": "dcn bwd",
                "conv_transpose2d_backward": "deconv bwd"}


def torch_twin(net):
    """The same tree on torch's operators: every library layer but the DCNs replaced by its nn counterpart (a fused ReLU or
    residual add becomes a small wrapper), sharing nothing with ``net``."""
    import copy

    import torch
    from torch import nn

    from centerpose_amd import conv, deconv, norm, pool, stem
    from centerpose_amd.lib.models.networks.DCNv2.dcn_v2 import DCN

    class BnAct(nn.Module):
        def __init__(self, m):
            super().__init__()
            self.bn = nn.BatchNorm2d(m.num_features, eps=m.eps, momentum=m.momentum)
            self.bn.load_state_dict(m.state_dict())
            self.relu = bool(m.relu)

        def forward(self, x, residual=None):
            y = self.bn(x)
            if residual is not None:
                y = y + residual
            return torch.relu(y) if self.relu else y

    twin = copy.deepcopy(net)

    def swap(parent):
        for name, m in list(parent.named_children()):
            if isinstance(m, DCN):
                continue     # (its conv_offset_mask stays the library's too: part of the deformable layer)
            if isinstance(m, norm.BatchNorm2d):
                new = BnAct(m)
            elif isinstance(m, (stem.StemConv2d, conv.Conv2d)):
                new = nn.Conv2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, bias=m.bias is not None)
                new.load_state_dict(m.state_dict())
            elif isinstance(m, deconv.ConvTranspose2d):
                new = nn.ConvTranspose2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, bias=False)
                new.load_state_dict(m.state_dict())
            elif isinstance(m, pool.MaxPool2d):
                new = nn.MaxPool2d(m.kernel_size, m.stride, m.padding)
            else:
                swap(m)
                continue
            setattr(parent, name, new)

    swap(twin)
    twin.to(next(net.parameters()).device)      # (the replacements were built on the CPU)
    heads = OrderedDict()
    for h in net.heads:
        a, b = getattr(getattr(net, h), "0"), getattr(getattr(net, h), "2")
        seq = nn.Sequential(nn.Conv2d(a.weight.shape[1], a.weight.shape[0], 3, padding=1), nn.ReLU(),
                            nn.Conv2d(b.weight.shape[1], b.weight.shape[0], 1))
        with torch.no_grad():
            seq[0].weight.copy_(a.weight), seq[0].bias.copy_(a.bias), seq[2].weight.copy_(b.weight), seq[2].bias.copy_(b.bias)
        heads[h] = seq
    twin.__dict__["_torch_heads"] = nn.ModuleDict(heads).to(next(net.parameters()).device)

    def forward(x):
        x = twin.maxpool(twin.bn1(twin.conv1(x)))
        x = twin.deconv_layers(twin.layer4(twin.layer3(twin.layer2(twin.layer1(x)))))
        return [OrderedDict((h, m(x)) for h, m in twin._torch_heads.items())]

    params = [p for n, p in twin.named_parameters() if n.split(".")[0] not in heads] + list(twin._torch_heads.parameters())
    return forward, params


def main():
    import torch

    from centerpose_amd import conv, deconv, hip, pose_heads, synth
    from centerpose_amd.lib.models.networks.DCNv2 import dcn_v2
    from centerpose_amd.pose_net_resdcn import PoseNetResDCN

    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", default="18,50")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--head-conv", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_net_resdcn_bench: no HIP device (there is nothing to measure on the CPU)")
    dev = torch.device("cuda:0")
    hip.set_default_precision("f32")
    B, S = a.batch, a.size
    lines = []

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for depth in [int(d) for d in a.depths.split(",")]:
        heads = synth.HEADS_POSE
        net = PoseNetResDCN(depth, heads, head_conv=a.head_conv)
        net.load_state_dict(synth.make_state_dict("resdcn_%d" % depth, heads, head_conv=a.head_conv))
        net = net.to(dev).train()
        twin_forward, twin_params = torch_twin(net)
        x = synth.frames(B, h=S, w=S).to(dev)
        xcl = x.contiguous(memory_format=torch.channels_last)
        g = torch.Generator(device=dev).manual_seed(3)
        lin = {h: torch.randn(B, c, S // 4, S // 4, device=dev, generator=g) for h, c in heads.items()}

        def switch(name):
            assert conv.set_backward_precision(net, name) > 0 and deconv.set_backward_precision(net, name) == 3
            assert pose_heads.set_backward_precision(net, name) == 1 and dcn_v2.set_backward_precision(net, name) == 3

        def lib_step():
            net.zero_grad(set_to_none=True)
            z = net(x)[0]
            sum((z[h] * lin[h]).sum() for h in z).backward()

        def torch_step():
            for p in twin_params:
                p.grad = None
            z = twin_forward(xcl)[0]
            sum((z[h] * lin[h]).sum() for h in z).backward()

        sides = OrderedDict([("f32", lambda: (switch("f32"), lib_step())), ("f16x3", lambda: (switch("f16x3"), lib_step())),
                             ("torch", torch_step)])
        for fn in sides.values():
            fn()
            fn()
        rounds = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, fn in sides.items():
                rounds[s].append(timed(fn))
        med = {s: statistics.median(v) for s, v in rounds.items()}
        # one more f16x3 step with every operator call bracketed by events
        switch("f16x3")
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
            lib_step()
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
        line = {"what": "step", "arch": "resdcn_%d" % depth, "B": B, "HxW": S, "head_conv": a.head_conv,
                "step_ms": {s: round(v, 2) for s, v in med.items()},
                "step_ms_rounds": {s: [round(v, 2) for v in r] for s, r in rounds.items()},
                "images_per_s": {s: round(B / v * 1e3, 1) for s, v in med.items()},
                "f16x3_over_f32": round(med["f16x3"] / med["f32"], 3), "f32_over_torch": round(med["f32"] / med["torch"], 3),
                "f16x3_over_torch": round(med["f16x3"] / med["torch"], 3), "traced_backward_precision": "f16x3",
                "traced_step_ms": round(traced, 2), "family_ms": {k: round(v, 2) for k, v in split.items()}, "family_calls": calls,
                "peak_memory_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        del net, twin_forward, twin_params, x, xcl, lin, sides
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
