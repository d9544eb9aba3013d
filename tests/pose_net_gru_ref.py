"""Reference of the PoseNetGRU tests (test helper, not a test module): ``dlav1_34``'s graph on a state dict, in training or
evaluation mode, in any float dtype, under autograd.  Backbone and up-sampling are tests/pose_net_ref.py's functions
(``dla34_base``, ``dla_up``, ``ida_up``, ``Ctx``); this file adds the ConvGRU (tests/conv_gru_ref.py: six separate convolutions per
step), the GroupNorm heads (pose_dla_dcn.py:491-521, groups by GN.py) and the routing of the heads to the GRU steps, which is
``oracle.backbone.head_routing``'s restatement of pose_dla_dcn.py:545-563.  tests/test_pose_net_gru_cpu.py pins its evaluation
mode to ``oracle.backbone.dlaseg_forward(arch='dlav1')``.
"""
import functools
from collections import OrderedDict

import torch
import torch.nn.functional as F

from centerpose_amd import synth
from oracle.backbone import head_routing
from tests import conv_gru_ref
from tests import pose_net_ref as P

GN_EPS = 1e-5
HEAD_CONV = P.HEAD_CONV   # 64: two channels per group
SHAPE = P.SHAPE
SEED = P.SEED


def heads_of(tracking):
    return synth.HEADS_TRACK if tracking else synth.HEADS_POSE


def gn_groups(c):
    return 32 if c % 32 == 0 else 16   # GN.py:4-9


def forward(sd, x, heads, training, tracking_task=False, pre_img=None, pre_hm=None, pre_hm_hp=None):
    """The head dict ``z`` (raw maps) of DLASeg.forward with the ConvGRU on the state dict ``sd``"""
    c = P.Ctx(sd, training)
    ups = P.dla_up(c, P.dla34_base(c, x, pre_img, pre_hm, pre_hm_hp))
    y = [ups[0], ups[1], ups[2]]
    P.ida_up(c, y, "ida_up", 0, 3, [1, 2, 4])
    gru = conv_gru_ref.conv_gru(sd, y[-1], 4 if tracking_task else 3, prefix="convGRU.cell0.")
    route = head_routing(heads, True, tracking_task)
    z = OrderedDict()
    for h in heads:
        t = P._conv(c, gru[route[h]], h + ".0", 1, 1)
        t = F.group_norm(t, gn_groups(t.shape[1]), sd[h + ".1.weight"], sd[h + ".1.bias"], GN_EPS)
        z[h] = P._conv(c, F.relu(t), h + ".3", 1, 0)
    return z


def case_state_dict(tracking, head_conv=HEAD_CONV):
    """synth's random dlav1_34 state dict with pose_net_ref.case_state_dict's changes (fractional offsets away from the cell
    borders, +3 on the BatchNorm shifts), and +4 on the heads' GroupNorm shifts in place of the heads' hidden biases, which
    the GroupNorm removes: gate flips at a ReLU are a property of the graph, not of the kernels."""
    heads = heads_of(tracking)
    sd = synth.make_state_dict("dlav1_34", heads, tracking=bool(tracking), seed=SEED, head_conv=head_conv)
    for k in sd:
        if k.endswith("conv_offset_mask.weight"):
            sd[k] = torch.randn(sd[k].shape, generator=P._gen(k)) * (0.02 / (9 * sd[k].shape[1]) ** 0.5)
        elif k.endswith("conv_offset_mask.bias"):
            g = P._gen(k)
            b = torch.rand(27, generator=g) * 0.2 + 0.15
            b = b * (torch.randint(0, 2, (27,), generator=g) * 2 - 1)
            b[18:] = torch.randn(9, generator=g) * 0.5
            sd[k] = b
        elif k.endswith(".bias") and k[:-5] + ".running_mean" in sd and not k.endswith("tree2.bn2.bias"):
            sd[k] = sd[k] + 3.0
        elif k.split(".")[0] in heads and k.endswith(".1.bias"):
            sd[k] = sd[k] + 4.0
    return sd


def case_inputs(tracking):
    """x, pre_img, pre_hm, pre_hm_hp (None without tracking) and the loss's linear functional per head"""
    B, _, H, W = SHAPE
    x = torch.randn(SHAPE, generator=P._gen("x"))
    pre_img = torch.randn(SHAPE, generator=P._gen("pre_img")) if tracking else None
    pre_hm = torch.rand(B, 1, H, W, generator=P._gen("pre_hm")) if tracking else None
    pre_hm_hp = torch.rand(B, 8, H, W, generator=P._gen("pre_hm_hp")) if tracking else None
    lin = OrderedDict((h, torch.randn(B, c, H // 4, W // 4, generator=P._gen("lin." + h))) for h, c in heads_of(tracking).items())
    return x, pre_img, pre_hm, pre_hm_hp, lin


def run(sd32, tracking, x, pre_img, pre_hm, pre_hm_hp, lin, dtype):
    """One training-mode forward + backward of loss = sum_h <z[h], lin[h]> in ``dtype`` on the CPU (pose_net_ref.run's result)"""
    sd = OrderedDict()
    for k, v in sd32.items():
        if not v.is_floating_point() or "running_" in k:
            sd[k] = v.clone() if not v.is_floating_point() else v.to(dtype).clone()
        else:
            sd[k] = v.to(dtype).clone().requires_grad_(True)
    cast = lambda t: None if t is None else t.to(dtype)
    z = forward(sd, cast(x), heads_of(tracking), True, bool(tracking), cast(pre_img), cast(pre_hm), cast(pre_hm_hp))
    loss = sum((z[h] * lin[h].to(dtype)).sum() for h in z)
    params = [k for k, v in sd.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [sd[k] for k in params], allow_unused=True)
    r = P.Result()
    r.z = OrderedDict((h, v.detach()) for h, v in z.items())
    r.grads = OrderedDict(zip(params, grads))
    r.buffers = OrderedDict((k, v) for k, v in sd.items() if not v.requires_grad)
    return r


@functools.lru_cache(maxsize=None)
def reference_case(tracking, dtype=torch.float64):
    """(state dict, inputs, Result) of the GPU test's case, computed once per process and left unchanged by its users"""
    sd = case_state_dict(tracking)
    inp = case_inputs(tracking)
    return sd, inp, run(sd, tracking, *inp, dtype)


def family(name, ndim):
    """pose_net_ref.family with the new families: the ConvGRU's parameters, the heads' GroupNorms, the heads' convolutions"""
    if name.startswith("convGRU."):
        return "gru"
    if name.split(".")[0] in synth.HEADS_TRACK:
        return "gn" if name.split(".")[1] == "1" else "heads"
    if name.startswith("base.pre_hm_hp_layer.0"):
        return "conv"
    return P.family(name, ndim)
