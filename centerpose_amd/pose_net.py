"""``PoseNet``: the reference's ``dla_34`` network (``DLASeg``, pose_dla_dcn.py:457-570) as one trainable ``nn.Module`` whose
layers all run on the library, forward and backward.

The module tree repeats the reference's -- ``base`` (``DLA``: ``base_layer``, ``level0`` .. ``level5`` of ``BasicBlock`` / ``Root`` /
``Tree``, the previous-frame stems), ``dla_up`` (``DLAUp`` of ``IDAUp``), ``ida_up`` and one ``Sequential``-shaped module per head --
so ``state_dict()`` has the reference's keys and shapes (``synth.param_spec('dla_34', ...)``) and reference checkpoints load
with ``strict=True``.  It is built from the library's layers with the documented fusions applied:

* ``stem.StemConv2d`` for the 7x7 stems of 1 and 3 planes, ``conv.Conv2d`` everywhere else (``conv_offset_mask`` included),
* ``norm.BatchNorm2d`` with ``relu = True`` and the residual passed in (``BasicBlock``, ``Root``, ``DeformConv``),
* ``pool.MaxPool2d`` for ``Tree.downsample``,
* the mirror's ``DCN`` (``lib/models/networks/DCNv2``) for the deformable layers,
* ``deconv.ConvTranspose2d`` with ``add = layers[i - 1]`` (``IDAUp``),
* ``pose_heads.PoseHeads`` for the heads, its per-head modules registered here under the heads' own names.

Two things differ from running the reference's tree in training mode, neither visible in a trained checkpoint's use: the
``project`` of a two-level ``Tree`` (``base.level3.project``, ``base.level4.project``), whose result the reference computes and
throws away (pose_dla_dcn.py:214-220), is not run at all, so its parameters get no gradient and its running statistics stay
as loaded; and initial convolution weights are ``nn.Conv2d``'s own (the reference starts from an ImageNet checkpoint).

``HipPoseNet.train_module()`` / ``load_module()`` (lib/models/model.py) move a model between this module and the inference
engine.
"""
from collections import OrderedDict

import torch
from torch import nn

from . import synth as _synth
from .conv import Conv2d, use_hip_convs
from .deconv import ConvTranspose2d
from .lib.models.networks.DCNv2.dcn_v2 import DCN
from .norm import BatchNorm2d
from .pool import MaxPool2d
from .pose_heads import PoseHeads
from .stem import StemConv2d

BN_MOMENTUM = 0.1  # pose_dla_dcn.py:19
_CHANNELS = [16, 32, 64, 128, 256, 512]  # dla34, pose_dla_dcn.py:340-343
_LEVELS = [1, 1, 1, 2, 2, 1]


def _bn(c, relu):
    m = BatchNorm2d(c, momentum=BN_MOMENTUM)
    m.relu = relu
    return m


class BasicBlock(nn.Module):
    """pose_dla_dcn.py:40-62: relu(bn1(conv1)) -> relu(bn2(conv2) + residual), each a convolution and one fused layer"""

    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = _bn(planes, True)
        self.conv2 = Conv2d(planes, planes, 3, stride=1, padding=1, bias=False)
        self.bn2 = _bn(planes, True)

    def forward(self, x, residual=None):
        out = self.bn1(self.conv1(x))
        return self.bn2(self.conv2(out), x if residual is None else residual)


class Root(nn.Module):
    """pose_dla_dcn.py:150-168 (dla34: residual_root = False)"""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = Conv2d(in_channels, out_channels, 1, stride=1, bias=False, padding=0)
        self.bn = _bn(out_channels, True)

    def forward(self, *x):
        return self.bn(self.conv(torch.cat(x, 1)))


class Tree(nn.Module):
    """pose_dla_dcn.py:171-224"""

    def __init__(self, levels, in_channels, out_channels, stride=1, level_root=False, root_dim=0):
        super().__init__()
        if root_dim == 0:
            root_dim = 2 * out_channels
        if level_root:
            root_dim += in_channels
        if levels == 1:
            self.tree1 = BasicBlock(in_channels, out_channels, stride)
            self.tree2 = BasicBlock(out_channels, out_channels, 1)
            self.root = Root(root_dim, out_channels)
        else:
            self.tree1 = Tree(levels - 1, in_channels, out_channels, stride, root_dim=0)
            self.tree2 = Tree(levels - 1, out_channels, out_channels, root_dim=root_dim + out_channels)
        self.level_root, self.levels = level_root, levels
        self.downsample = MaxPool2d(stride, stride=stride) if stride > 1 else None
        self.project = None
        if in_channels != out_channels:
            self.project = nn.Sequential(Conv2d(in_channels, out_channels, 1, stride=1, bias=False), _bn(out_channels, False))

    def forward(self, x, children=None):
        children = [] if children is None else children
        bottom = self.downsample(x) if self.downsample is not None else x
        if self.level_root:
            children.append(bottom)
        if self.levels == 1:
            residual = self.project(bottom) if self.project is not None else bottom
            x1 = self.tree1(x, residual)
            x2 = self.tree2(x1)
            return self.root(x2, x1, *children)
        # two levels: the inner tree recomputes its own residual (pose_dla_dcn.py:214), this level's project is never used
        x1 = self.tree1(x)
        children.append(x1)
        return self.tree2(x1, children=children)


def _conv_level(inplanes, planes, stride, stem=None):
    """conv -> BatchNorm -> ReLU under the reference's Sequential indices 0 and 1 (the ReLU runs inside the BatchNorm)"""
    if stem is None:
        conv = Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
    else:
        conv = stem(inplanes, planes, 7, stride=1, padding=3, bias=False)
    return nn.Sequential(conv, _bn(planes, True))


class DLA(nn.Module):
    """pose_dla_dcn.py:227-322 for dla34; ``tracking`` = which of (pre_img, pre_hm, pre_hm_hp) stems exist"""

    def __init__(self, tracking):
        super().__init__()
        ch = _CHANNELS
        self.base_layer = _conv_level(3, ch[0], 1, StemConv2d)
        self.level0 = _conv_level(ch[0], ch[0], 1)
        self.level1 = _conv_level(ch[0], ch[1], 2)
        self.level2 = Tree(_LEVELS[2], ch[1], ch[2], 2, level_root=False)
        self.level3 = Tree(_LEVELS[3], ch[2], ch[3], 2, level_root=True)
        self.level4 = Tree(_LEVELS[4], ch[3], ch[4], 2, level_root=True)
        self.level5 = Tree(_LEVELS[5], ch[4], ch[5], 2, level_root=True)
        if tracking[0]:
            self.pre_img_layer = _conv_level(3, ch[0], 1, StemConv2d)
        if tracking[1]:
            self.pre_hm_layer = _conv_level(1, ch[0], 1, StemConv2d)
        if tracking[2]:
            self.pre_hm_hp_layer = _conv_level(8, ch[0], 1, Conv2d)  # 8 planes: an ordinary convolution

    def forward(self, x, pre_img=None, pre_hm=None, pre_hm_hp=None):
        y = []
        x = self.base_layer(x)
        # sums of ReLUs (pose_dla_dcn.py:312-318): torch adds, not the fused relu(bn + residual)
        for name, t in (("pre_img", pre_img), ("pre_hm", pre_hm), ("pre_hm_hp", pre_hm_hp)):
            if t is not None:
                layer = getattr(self, name + "_layer", None)
                if layer is None:
                    raise RuntimeError("PoseNet: %s was passed but the model was built without opt.%s" % (name, name))
                x = x + layer(t)
        for i in range(6):
            x = getattr(self, "level%d" % i)(x)
            y.append(x)
        return y


class DeformConv(nn.Module):
    """pose_dla_dcn.py:377-389: DCN -> BatchNorm -> ReLU, the last two as one layer"""

    def __init__(self, chi, cho):
        super().__init__()
        self.actf = nn.Sequential(_bn(cho, True))
        self.conv = DCN(chi, cho, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1)
        use_hip_convs(self.conv.conv_offset_mask)

    def forward(self, x):
        return self.actf[0](self.conv(x))


def fill_up_weights(up):
    """pose_dla_dcn.py:365-374"""
    with torch.no_grad():
        up.weight.copy_(_synth._bilinear_up(tuple(up.weight.shape)))


class IDAUp(nn.Module):
    """pose_dla_dcn.py:392-417"""

    def __init__(self, o, channels, up_f):
        super().__init__()
        for i in range(1, len(channels)):
            f = int(up_f[i])
            setattr(self, "proj_%d" % i, DeformConv(channels[i], o))
            up = ConvTranspose2d(o, o, f * 2, stride=f, padding=f // 2, output_padding=0, groups=o, bias=False)
            fill_up_weights(up)
            setattr(self, "up_%d" % i, up)
            setattr(self, "node_%d" % i, DeformConv(o, o))

    def forward(self, layers, startp, endp):
        for i in range(startp + 1, endp):
            k = i - startp
            up = getattr(self, "up_%d" % k)(getattr(self, "proj_%d" % k)(layers[i]), layers[i - 1])  # + layers[i - 1] in the kernel
            layers[i] = getattr(self, "node_%d" % k)(up)


class DLAUp(nn.Module):
    """pose_dla_dcn.py:420-443"""

    def __init__(self, startp, channels, scales):
        super().__init__()
        self.startp = startp
        channels, in_channels, scales = list(channels), list(channels), list(scales)
        for i in range(len(channels) - 1):
            j = -i - 2
            setattr(self, "ida_%d" % i, IDAUp(channels[j], in_channels[j:], [s // scales[j] for s in scales[j:]]))
            scales[j + 1:] = [scales[j]] * len(scales[j + 1:])
            in_channels[j + 1:] = [channels[j]] * len(channels[j + 1:])

    def forward(self, layers):
        layers = list(layers)
        out = [layers[-1]]
        for i in range(len(layers) - self.startp - 1):
            getattr(self, "ida_%d" % i)(layers, len(layers) - i - 2, len(layers))
            out.insert(0, layers[-1])
        return out


_MISSING = {
    "dlav1": "its ConvGRU and GroupNorm heads are composed by centerpose_amd.pose_net_gru.PoseNetGRU (build one with "
             "PoseNetGRU.from_model(model) and hand it back with model.load_module(net))",
    "hourglass": "the two-stack hourglass is composed by centerpose_amd.pose_net_hourglass.PoseNetHourglass, which returns one "
                 "head dict per stack (build one with PoseNetHourglass.from_model(model) and hand it back with "
                 "model.load_module(net))",
    "resdcn": "the ResNet-DCN family is composed by centerpose_amd.pose_net_resdcn.PoseNetResDCN (build one with "
              "PoseNetResDCN.from_model(model) and hand it back with model.load_module(net))",
}


def compose_backbone(net, opt):
    """Registers DLASeg's ``base``, ``dla_up`` and ``ida_up`` (pose_dla_dcn.py:473-489, down_ratio 4) on ``net``, in the reference's
    order; ``opt`` says which previous-frame stems exist.  Shared by ``PoseNet`` and ``pose_net_gru.PoseNetGRU``."""
    net.pre_stems = tuple(bool(opt is not None and getattr(opt, f, False)) for f in ("pre_img", "pre_hm", "pre_hm_hp"))
    net.first_level, net.last_level = 2, 5  # down_ratio 4
    net.base = DLA(net.pre_stems)
    ch = _CHANNELS
    scales = [2 ** i for i in range(len(ch[net.first_level:]))]
    net.dla_up = DLAUp(net.first_level, ch[net.first_level:], scales)
    net.ida_up = IDAUp(ch[net.first_level], ch[net.first_level:net.last_level],
                       [2 ** i for i in range(net.last_level - net.first_level)])


def run_backbone(net, x, pre_img=None, pre_hm=None, pre_hm_hp=None):
    """DLASeg.forward up to the feature map the heads (or the ConvGRU) read: [B,64,H/4,W/4]"""
    y = net.dla_up(net.base(x, pre_img, pre_hm, pre_hm_hp))
    y = y[:net.last_level - net.first_level]
    net.ida_up(y, 0, len(y))
    return y[-1]


class PoseNet(nn.Module):
    """``PoseNet(heads, head_conv=256, opt=None)``: ``dla_34``.  ``heads`` maps head name -> classes (``opt.heads``); ``opt`` may
    set ``pre_img`` / ``pre_hm`` / ``pre_hm_hp`` (which previous-frame stems exist), as for ``create_model``.
    ``forward(x, pre_img=None, pre_hm=None, pre_hm_hp=None)`` takes NCHW images on the device and returns ``[z]``, ``z`` the
    dict of raw head maps, like ``DLASeg``.  ``eval()`` runs the same layers on the running statistics."""

    def __init__(self, heads, head_conv=256, opt=None, arch="dla_34"):
        super().__init__()
        family = arch.split("_")[0]
        if family in _MISSING:
            raise NotImplementedError("PoseNet: %s is not built: %s" % (arch, _MISSING[family]))
        if arch != "dla_34":
            raise NotImplementedError("PoseNet: only dla_34 is built, got %r" % (arch,))
        self.arch = arch
        self.heads = OrderedDict(heads)
        self.head_conv = int(head_conv)
        compose_backbone(self, opt)
        ch = _CHANNELS
        # the heads: one PoseHeads (one autograd function over all of them), its per-head modules registered under this
        # module so that the state-dict keys are the reference's `hm.0.weight`, ... without a prefix
        block = PoseHeads(self.heads, ch[self.first_level], self.head_conv)
        for name in self.heads:
            if name in self._modules or hasattr(self, name):
                raise ValueError("PoseNet: head name %r collides with an attribute of the module" % name)
            self.add_module(name, getattr(block, name))
        self.__dict__["_head_block"] = block  # (not a sub-module: its parameters are registered above)

    def forward(self, x, pre_img=None, pre_hm=None, pre_hm_hp=None):
        return [self._head_block(run_backbone(self, x, pre_img, pre_hm, pre_hm_hp))]
