"""Reference of the PoseNetResDCN tests (test helper, not a test module): a functional torch restatement of the ResNet-DCN graph
(``PoseResNet`` with DCN up-sampling, resnet_dcn.py:134-267) on a state dict, in training or evaluation mode, in any float
dtype, under autograd.  It is built from tests/pose_net_ref.py's pieces (``_conv``, ``_bn``, ``_conv_bn``, the differentiable
``dcn_v2``) and conditions its case by the same recipe.  tests/test_pose_net_resdcn_cpu.py pins its evaluation mode to
``tests.resdcn_ref.torch_resdcn_forward`` and checks that the case the GPU test uses is well conditioned;
tests/test_pose_net_resdcn_gpu.py compares ``centerpose_amd.pose_net_resdcn.PoseNetResDCN`` with its float64 run.
"""
import functools
import zlib
from collections import OrderedDict

import torch
import torch.nn.functional as F

from centerpose_amd import synth
from tests.pose_net_ref import Ctx, Result, _bn, _conv, _conv_bn, companion_weight, dcn_v2

HEAD_CONV = 32
SHAPE = (2, 3, 64, 96)   # B, planes, H, W: layer4 and the first DCN see 2 x 3 maps, the deconvs run 2x3 -> 4x6 -> 8x12 -> 16x24
SEED = 11
DEPTHS = (18, 50)        # BasicBlock, Bottleneck


def block(c, x, p, bottleneck, stride):
    residual = x
    if p + ".downsample.0.weight" in c.sd:
        residual = _conv_bn(c, x, p + ".downsample.0", p + ".downsample.1", stride, 0, relu=False)
    if bottleneck:
        out = _conv_bn(c, x, p + ".conv1", p + ".bn1", 1, 0)
        out = _conv_bn(c, out, p + ".conv2", p + ".bn2", stride, 1)
        return F.relu(_conv_bn(c, out, p + ".conv3", p + ".bn3", 1, 0, relu=False) + residual)
    out = _conv_bn(c, x, p + ".conv1", p + ".bn1", stride, 1)
    return F.relu(_conv_bn(c, out, p + ".conv2", p + ".bn2", 1, 1, relu=False) + residual)


def forward(sd, x, depth, heads, training):
    """The head dict ``z`` (raw maps) of PoseResNet.forward on the state dict ``sd`` (tensors of x's dtype; in training mode the
    running statistics and num_batches_tracked in ``sd`` are updated in place, as nn.BatchNorm2d does)."""
    c = Ctx(sd, training)
    bottleneck, blocks = synth.RESNET_SPEC[depth]
    x = F.max_pool2d(_conv_bn(c, x, "conv1", "bn1", 2, 3), 3, 2, 1)
    for li, n in enumerate(blocks):
        for b in range(n):
            x = block(c, x, "layer%d.%d" % (li + 1, b), bottleneck, 2 if li and b == 0 else 1)
    for i in range(3):
        p = "deconv_layers.%d" % (6 * i)
        om = _conv(c, x, p + ".conv_offset_mask", 1, 1)
        x = dcn_v2(x, sd[p + ".weight"], sd[p + ".bias"], om[:, :18], torch.sigmoid(om[:, 18:27]))
        x = F.relu(_bn(c, x, "deconv_layers.%d" % (6 * i + 1)))
        x = F.conv_transpose2d(x, sd["deconv_layers.%d.weight" % (6 * i + 3)], None, stride=2, padding=1)
        x = F.relu(_bn(c, x, "deconv_layers.%d" % (6 * i + 4)))
    z = OrderedDict()
    for h in heads:
        z[h] = _conv(c, F.relu(_conv(c, x, h + ".0", 1, 1)), h + ".2", 1, 0)
    return z


# ---- the case of the GPU test ----

def _gen(name):
    return torch.Generator().manual_seed(SEED * 1000003 + zlib.crc32(name.encode()))


def case_state_dict(depth):
    """synth's random resdcn state dict, conditioned as tests/pose_net_ref.py's (see case_state_dict there for the reasons):
    conv_offset_mask weights of contribution std ~0.02, offset biases 0.15 .. 0.35 in magnitude with random sign, N(0, 0.5) mask
    logits; +3 on every BatchNorm shift, +4 on the heads' hidden biases."""
    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("resdcn_%d" % depth, heads, seed=SEED, head_conv=HEAD_CONV)
    for k in sd:
        if k.endswith("conv_offset_mask.weight"):
            sd[k] = torch.randn(sd[k].shape, generator=_gen(k)) * (0.02 / (9 * sd[k].shape[1]) ** 0.5)
        elif k.endswith("conv_offset_mask.bias"):
            g = _gen(k)
            b = torch.rand(27, generator=g) * 0.2 + 0.15
            b = b * (torch.randint(0, 2, (27,), generator=g) * 2 - 1)
            b[18:] = torch.randn(9, generator=g) * 0.5
            sd[k] = b
        elif k.endswith(".bias") and k[:-5] + ".running_mean" in sd:
            sd[k] = sd[k] + 3.0
        elif k.split(".")[0] in heads and k.endswith(".0.bias"):
            sd[k] = sd[k] + 4.0
    return sd


def case_inputs():
    B, _, H, W = SHAPE
    x = torch.randn(SHAPE, generator=_gen("x"))
    lin = OrderedDict((h, torch.randn(B, c, H // 4, W // 4, generator=_gen("lin." + h))) for h, c in synth.HEADS_POSE.items())
    return x, lin


def run(sd32, depth, x, lin, dtype):
    """One training-mode forward + backward of loss = sum_h <z[h], lin[h]> in ``dtype`` on the CPU.  Returns the outputs, the
    gradients of the floating-point parameters and the buffers after the step (tests/pose_net_ref.py's Result)."""
    sd = OrderedDict()
    for k, v in sd32.items():
        if not v.is_floating_point() or "running_" in k:
            sd[k] = v.clone() if not v.is_floating_point() else v.to(dtype).clone()
        else:
            sd[k] = v.to(dtype).clone().requires_grad_(True)
    z = forward(sd, x.to(dtype), depth, synth.HEADS_POSE, True)
    loss = sum((z[h] * lin[h].to(dtype)).sum() for h in z)
    params = [k for k, v in sd.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [sd[k] for k in params])
    r = Result()
    r.z = OrderedDict((h, v.detach()) for h, v in z.items())
    r.grads = OrderedDict(zip(params, grads))
    r.buffers = OrderedDict((k, v) for k, v in sd.items() if not v.requires_grad)
    return r


@functools.lru_cache(maxsize=None)
def reference_case(depth, dtype=torch.float64):
    """(state dict, inputs, Result) of the GPU test's case, computed once per process and left unchanged by its users."""
    sd = case_state_dict(depth)
    inp = case_inputs()
    return sd, inp, run(sd, depth, *inp, dtype)


def family(name, ndim):
    """The tensor family a parameter belongs to (the lines the tests print)."""
    if "conv_offset_mask" in name:
        return "offset conv"
    if name.startswith("deconv_layers."):
        i = int(name.split(".")[1]) % 6
        return "dcn" if i == 0 else "deconv" if i == 3 else "bn"
    if name.split(".")[0] in synth.HEADS_POSE:
        return "heads"
    if name == "conv1.weight":
        return "stem"
    return "bn" if ndim == 1 else "conv"


FAMILIES = ("stem", "conv", "bn", "offset conv", "dcn", "deconv", "heads")
F16X3_FAMILIES = ("conv", "offset conv", "dcn", "deconv", "heads")    # the kinds whose weight gradient a backward switch moves


def zero_gradient_biases(ref):
    """The biases whose gradient is mathematically zero because a training BatchNorm removes every per-channel constant that
    reaches it un-gated (the three DCN ``.bias``; in the Bottleneck nets also shifts ahead of a 1x1 convolution and its
    BatchNorm whose ReLU gates nothing), decided from the float64 reference alone: the gradient's maximum is below 1e-6 of the
    same module's weight-gradient maximum.  The tests bound such a bias by that weight gradient's maximum."""
    out = []
    for k, g in ref.grads.items():
        if k.endswith(".bias") and companion_weight(k) in ref.grads:
            if float(g.abs().max()) < 1e-6 * float(ref.grads[companion_weight(k)].abs().max()):
                out.append(k)
    return out


def scales(ref):
    """name -> the magnitude a gradient's error is measured against: its own float64 maximum, or its module's weight gradient's
    for a zero-gradient bias."""
    zero = set(zero_gradient_biases(ref))
    return OrderedDict((k, float(ref.grads[companion_weight(k) if k in zero else k].abs().max())) for k in ref.grads)


def compare(got, ref):
    """Relative errors of a step (a Result, or anything with .z / .grads / .buffers of CPU tensors) against the float64
    ``ref``: (outputs, gradients per family {family: (worst, name)}, running statistics), each error / its scale."""
    out = max(float((got.z[h].double() - ref.z[h]).abs().max()) / float(ref.z[h].abs().max()) for h in ref.z)
    fam = {}
    for k, s in scales(ref).items():
        assert s > 0, k
        e = float((got.grads[k].double() - ref.grads[k]).abs().max()) / s
        f = family(k, ref.grads[k].dim())
        if f not in fam or e > fam[f][0]:
            fam[f] = (e, k)
    stat = max(float((got.buffers[k].double() - v).abs().max()) / float(v.abs().max())
               for k, v in ref.buffers.items() if v.is_floating_point())
    return out, fam, stat
