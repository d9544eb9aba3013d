"""Reference of the PoseNetHourglass tests (test helper, not a test module): a functional torch restatement of the stacked
hourglass's graph (``exkp``, large_hourglass.py:190-287, configured as ``HourglassNet``, :290-309) on a state dict, in training
or evaluation mode, in any float dtype, under autograd: ``F.conv2d``, ``F.batch_norm(training=...)``, ``F.interpolate``.

The structural arguments are ``exkp``'s (``n``, ``dims``, ``modules``, ``nstack``), so the tests run a shallow instance:
``CASE`` is ``exkp(2, 2, [256, 256, 384], [1, 1, 1], heads)`` on a 2 x 3 x 64 x 96 input (maps of 16 x 24, 8 x 12 and 4 x 6).
tests/test_pose_net_hourglass_cpu.py pins the float64 run of that case to tests/golden/hourglass_train_ref.npz (written by
tools/make_hourglass_train_golden.py from the reference's own module) and the evaluation mode at full depth to
tests/golden/backbone_hourglass.npz; tests/test_pose_net_hourglass_gpu.py compares
``centerpose_amd.pose_net_hourglass.PoseNetHourglass`` with the float64 run.
"""
import functools
import zlib
from collections import OrderedDict

import torch
import torch.nn.functional as F

from centerpose_amd import synth

BN_EPS, BN_MOMENTUM = 1e-5, 0.1   # nn.BatchNorm2d's defaults (large_hourglass.py:24, :56, :60, :64)
CASE = dict(n=2, dims=[256, 256, 384], modules=[1, 1, 1], num_stacks=2)
SHAPE = (2, 3, 64, 96)            # B, planes, H, W of the GPU test
SEED = 23
HEADS = synth.HEADS_POSE
GOLDEN_BNS = ("pre.0.bn", "kps.0.low2.low2.0.bn2", "cnvs_.0.1")   # the BatchNorms whose updated statistics the golden file holds


class Ctx:
    def __init__(self, sd, training):
        self.sd, self.training = sd, training


def _conv(c, x, name, stride=1, padding=0):
    return F.conv2d(x, c.sd[name + ".weight"], c.sd.get(name + ".bias"), stride=stride, padding=padding)


def _bn(c, x, name):
    sd = c.sd
    if c.training:
        sd[name + ".num_batches_tracked"] += 1
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                        c.training, BN_MOMENTUM, BN_EPS)


def convolution(c, x, p, k, stride=1):
    """large_hourglass.py:27-31 with BatchNorm"""
    return F.relu(_bn(c, _conv(c, x, p + ".conv", stride, (k - 1) // 2), p + ".bn"))


def residual(c, x, p, stride=1):
    """large_hourglass.py:68-77; the 1x1 skip exists where the state dict has one"""
    out = F.relu(_bn(c, _conv(c, x, p + ".conv1", stride, 1), p + ".bn1"))
    out = _bn(c, _conv(c, out, p + ".conv2", 1, 1), p + ".bn2")
    skip = _bn(c, _conv(c, x, p + ".skip.0", stride, 0), p + ".skip.1") if p + ".skip.0.weight" in c.sd else x
    return F.relu(out + skip)


def layer(c, x, p, count, stride=1):
    """make_layer / make_hg_layer / make_layer_revr (large_hourglass.py:80-92, :290-293): the widths are the state dict's"""
    for i in range(count):
        x = residual(c, x, "%s.%d" % (p, i), stride if i == 0 else 1)
    return x


def kp_module(c, x, p, n, modules):
    """large_hourglass.py:180-187 (max1 is empty, low1 has stride 2)"""
    up1 = layer(c, x, p + ".up1", modules[0])
    low1 = layer(c, x, p + ".low1", modules[0], 2)
    low2 = kp_module(c, low1, p + ".low2", n - 1, modules[1:]) if n > 1 else layer(c, low1, p + ".low2", modules[1])
    low3 = layer(c, low2, p + ".low3", modules[0])
    return up1 + F.interpolate(low3, scale_factor=2)


def forward(sd, x, heads, training, n=5, modules=synth.HG_MODULES, num_stacks=2, dims=None):
    """The list of head dicts (raw maps), one per stack, of exkp.forward (large_hourglass.py:266-287) on the state dict ``sd``
    (tensors of x's dtype; in training mode the running statistics and num_batches_tracked in ``sd`` are updated in place, as
    nn.BatchNorm2d does).  ``dims`` is implied by the state dict and accepted for symmetry with the module's signature."""
    c = Ctx(sd, training)
    inter = residual(c, convolution(c, x, "pre.0", 7, 2), "pre.1", 2)
    outs = []
    for k in range(num_stacks):
        cnv = convolution(c, kp_module(c, inter, "kps.%d" % k, n, list(modules)), "cnvs.%d" % k, 3)
        z = OrderedDict()
        for h in heads:
            z[h] = _conv(c, F.relu(_conv(c, cnv, "%s.%d.0.conv" % (h, k), 1, 1)), "%s.%d.1" % (h, k), 1, 0)
        outs.append(z)
        if k < num_stacks - 1:
            inter = _bn(c, _conv(c, inter, "inters_.%d.0" % k), "inters_.%d.1" % k) + \
                _bn(c, _conv(c, cnv, "cnvs_.%d.0" % k), "cnvs_.%d.1" % k)
            inter = residual(c, F.relu(inter), "inters.%d" % k)
    return outs


# ---- the case of the GPU test ----

def _gen(name):
    return torch.Generator().manual_seed(SEED * 1000003 + zlib.crc32(name.encode()))


def case_spec(heads=HEADS, n=CASE["n"], dims=CASE["dims"], modules=CASE["modules"], num_stacks=CASE["num_stacks"]):
    """name -> shape of ``exkp(n, num_stacks, dims, modules, heads)``'s state dict, in its order (synth.hourglass_param_spec with
    the structural arguments left open)."""
    s = OrderedDict()
    s["pre.0.conv.weight"] = (128, 3, 7, 7)
    synth._bn(s, "pre.0.bn", 128)
    synth._hg_residual(s, "pre.1", 128, 256, 2)
    for k in range(num_stacks):
        synth._hg_kp(s, "kps.%d" % k, n, dims, modules)
    for k in range(num_stacks):
        s["cnvs.%d.conv.weight" % k] = (256, dims[0], 3, 3)
        synth._bn(s, "cnvs.%d.bn" % k, 256)
    for k in range(num_stacks - 1):
        synth._hg_residual(s, "inters.%d" % k, dims[0], dims[0])
    for nm, cin in (("inters_", dims[0]), ("cnvs_", 256)):
        for k in range(num_stacks - 1):
            s["%s.%d.0.weight" % (nm, k)] = (dims[0], cin, 1, 1)
            synth._bn(s, "%s.%d.1" % (nm, k), dims[0])
    for h, classes in heads.items():
        for k in range(num_stacks):
            s["%s.%d.0.conv.weight" % (h, k)] = (dims[0], 256, 3, 3)
            s["%s.%d.0.conv.bias" % (h, k)] = (dims[0],)
            s["%s.%d.1.weight" % (h, k)] = (classes, dims[0], 1, 1)
            s["%s.%d.1.bias" % (h, k)] = (classes,)
    return s


def case_state_dict():
    """A seeded random state dict of the shallow instance: He-normal convolution weights (conv2 of a residual damped to 0.35,
    the heads' final 1x1 to 0.5, as synth does for this architecture), BatchNorm scales in 0.8 .. 1.2, running variances
    likewise, shifts / biases / running means N(0, 0.1).

    The shifts ahead of the ReLUs are then raised: +3 on every BatchNorm shift, +4 on the heads' hidden biases.  The gradient
    is discontinuous where a ReLU's input crosses zero, and with shifts of N(0, 0.1) some of the network's ReLU inputs lie
    inside the float32 forward error: two float32 evaluations then differ by 1e-2 of a gradient's maximum whatever computes
    them.  Raised, a ReLU input in a thousand is still negative, so every gate is exercised."""
    sd, spec = OrderedDict(), case_spec()
    for name, shape in spec.items():
        g = _gen(name)
        leaf = name.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            t = torch.zeros((), dtype=torch.long)
        elif leaf == "running_var" or (len(shape) == 1 and leaf == "weight"):
            t = torch.rand(shape, generator=g) * 0.4 + 0.8
        elif len(shape) == 1:
            t = torch.randn(shape, generator=g) * 0.1
            if name[:-len(".bias")] + ".running_mean" in spec:
                t = t + 3.0
            elif name.endswith(".0.conv.bias"):
                t = t + 4.0
        else:
            t = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
            if name.endswith(".conv2.weight"):
                t = t * 0.35
            elif name.split(".")[0] in HEADS and shape[2] == 1:
                t = t * 0.5
        sd[name] = t
    return sd


def case_inputs():
    B, _, H, W = SHAPE
    x = torch.randn(SHAPE, generator=_gen("x"))
    lin = [OrderedDict((h, torch.randn(B, c, H // 4, W // 4, generator=_gen("lin.%d.%s" % (k, h)))) for h, c in HEADS.items())
           for k in range(CASE["num_stacks"])]
    return x, lin


Result = type("Result", (), {})


def run(sd32, x, lin, dtype, **structure):
    """One training-mode forward + backward of loss = sum over stacks and heads of <z[k][h], lin[k][h]> in ``dtype`` on the CPU.
    Returns the outputs per stack, the gradients of the floating-point parameters and the buffers after the step."""
    structure = structure or CASE
    sd = OrderedDict()
    for k, v in sd32.items():
        if not v.is_floating_point() or "running_" in k:
            sd[k] = v.clone() if not v.is_floating_point() else v.to(dtype).clone()
        else:
            sd[k] = v.to(dtype).clone().requires_grad_(True)
    zs = forward(sd, x.to(dtype), HEADS, True, **structure)
    loss = sum((z[h] * lin[k][h].to(dtype)).sum() for k, z in enumerate(zs) for h in z)
    params = [k for k, v in sd.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [sd[k] for k in params])
    r = Result()
    r.z = [OrderedDict((h, v.detach()) for h, v in z.items()) for z in zs]
    r.grads = OrderedDict(zip(params, grads))
    r.buffers = OrderedDict((k, v) for k, v in sd.items() if not v.requires_grad)
    return r


@functools.lru_cache(maxsize=None)
def reference_case(dtype=torch.float64):
    """(state dict, inputs, Result) of the GPU test's case, computed once per process and left unchanged by its users."""
    sd = case_state_dict()
    inp = case_inputs()
    return sd, inp, run(sd, *inp, dtype)


def family(name, ndim):
    """The tensor family a parameter belongs to (the lines tests/test_pose_net_hourglass_gpu.py prints)."""
    if name.split(".")[0] in HEADS:
        return "heads"
    if name.startswith("pre.0.conv"):
        return "stem"
    return "bn" if ndim == 1 else "conv"


def grad_sample(g):
    """The fixed strided sample of a gradient the golden file holds: at most 64 values of the flattened tensor."""
    flat = g.reshape(-1)
    return flat[::max(1, -(-flat.numel() // 64))][:64]
