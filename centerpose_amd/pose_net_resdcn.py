"""``PoseNetResDCN``: the reference's ResNet-DCN family (``PoseResNet`` with DCN up-sampling, resnet_dcn.py:134-267;
``resdcn_18|34|50|101|152``) as one trainable ``nn.Module`` whose layers all run on the library, forward and backward.

The module tree repeats the reference's -- ``conv1``, ``bn1``, ``maxpool``, ``layer1`` .. ``layer4`` of ``BasicBlock`` or
``Bottleneck``, the ``deconv_layers`` Sequential of three (DCN, BatchNorm, ReLU, ConvTranspose2d, BatchNorm, ReLU) stages and one
``Sequential``-shaped module per head -- so ``state_dict()`` has the reference's keys, shapes and order
(``synth.param_spec('resdcn_N', ...)``) and reference checkpoints load with ``strict=True``.  It is built from the library's
layers with the documented fusions applied:

* ``stem.StemConv2d`` for the 7x7 / stride-2 ``conv1``, ``pool.MaxPool2d(3, 2, 1)``, ``conv.Conv2d`` for every 1x1 and 3x3,
* ``norm.BatchNorm2d`` with ``relu = True`` wherever a ReLU follows, and the residual passed in at a block's last one, so the
  ``out += residual; relu`` of a block is part of that layer (the ReLU slots 2, 5, ... of ``deconv_layers`` hold an
  ``nn.Identity``: the keys keep the reference's indices and the ReLUs run inside the BatchNorms),
* the mirror's ``DCN`` (``lib/models/networks/DCNv2``) with its ``conv_offset_mask`` on ``conv.Conv2d``,
* ``deconv.ConvTranspose2d`` for the three dense ``ConvTranspose2d(planes, planes, 4, 2, 1, bias=False)``,
* ``pose_heads.PoseHeads`` for the heads, its per-head modules registered here under the heads' own names.

Initial weights are the layers' own (the reference starts from an ImageNet checkpoint); the deconvs start from the reference's
bilinear ``fill_up_weights``.

``PoseNet(arch="resdcn_N")`` and ``HipPoseNet.train_module()`` keep refusing the family; this class is reached as
``PoseNetGRU`` and ``PoseNetHourglass`` are: ``PoseNetResDCN.from_model(model)``, then ``model.load_module(net)``.
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

BN_MOMENTUM = 0.1  # resnet_dcn.py:20
_DECONV_PLANES = (256, 128, 64)


def _bn(c, relu):
    m = BatchNorm2d(c, momentum=BN_MOMENTUM)
    m.relu = relu
    return m


def _downsample(inplanes, outplanes, stride):
    """resnet_dcn.py:185-190: the 1x1 projection of a stage's first block; no ReLU -- its output is the block's residual"""
    return nn.Sequential(Conv2d(inplanes, outplanes, 1, stride=stride, bias=False), _bn(outplanes, False))


class BasicBlock(nn.Module):
    """resnet_dcn.py:39-68: relu(bn1(conv1)) -> relu(bn2(conv2) + residual), each a convolution and one fused layer"""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = _bn(planes, True)
        self.conv2 = Conv2d(planes, planes, 3, stride=1, padding=1, bias=False)
        self.bn2 = _bn(planes, True)
        self.downsample = downsample

    def forward(self, x):
        residual = x if self.downsample is None else self.downsample(x)
        out = self.bn1(self.conv1(x))
        return self.bn2(self.conv2(out), residual)


class Bottleneck(nn.Module):
    """resnet_dcn.py:71-109: 1x1 -> 3x3 (carries the stride) -> 1x1 to 4 x planes, the add and last ReLU inside bn3"""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = _bn(planes, True)
        self.conv2 = Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = _bn(planes, True)
        self.conv3 = Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = _bn(planes * self.expansion, True)
        self.downsample = downsample

    def forward(self, x):
        residual = x if self.downsample is None else self.downsample(x)
        out = self.bn1(self.conv1(x))
        out = self.bn2(self.conv2(out))
        return self.bn3(self.conv3(out), residual)


def fill_up_weights(up):
    """resnet_dcn.py:112-121: the bilinear kernel in [c, 0] of every input channel c, the layer's other entries as they are"""
    with torch.no_grad():
        k = _synth._bilinear_up((1, 1) + tuple(up.weight.shape[2:]))[0, 0]
        up.weight[:, 0] = k.to(up.weight)


class PoseNetResDCN(nn.Module):
    """``PoseNetResDCN(depth, heads, head_conv=64)``: ``resdcn_<depth>``, depth one of ``synth.RESNET_SPEC``.  ``heads`` maps head
    name -> classes (``opt.heads``).  ``forward(x)`` takes an NCHW image batch on the device, H and W multiples of 32, and returns
    ``[z]``, ``z`` the dict of raw head maps in ``heads`` order, like ``PoseResNet``.  ``eval()`` runs the same layers on the
    running statistics."""
    arch = "resdcn_%d"

    def __init__(self, depth, heads, head_conv=64):
        super().__init__()
        if depth not in _synth.RESNET_SPEC:
            raise NotImplementedError("PoseNetResDCN: depth must be one of %s (synth.RESNET_SPEC), got %r"
                                      % (sorted(_synth.RESNET_SPEC), depth))
        head_conv = int(head_conv)
        if head_conv < 32 or head_conv % 32:
            raise NotImplementedError("PoseNetResDCN: head_conv must be a positive multiple of 32 (the heads' hidden width on "
                                      "the matrix cores), got %d" % head_conv)
        self.depth = int(depth)
        self.arch = type(self).arch % self.depth
        self.heads = OrderedDict(heads)
        self.head_conv = head_conv
        bottleneck, blocks = _synth.RESNET_SPEC[self.depth]
        block = Bottleneck if bottleneck else BasicBlock
        self.conv1 = StemConv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = _bn(64, True)
        self.maxpool = MaxPool2d(3, stride=2, padding=1)
        inplanes = 64
        for i, n in enumerate(blocks):
            planes, stride = 64 << i, (2 if i else 1)
            down = None
            if stride != 1 or inplanes != planes * block.expansion:
                down = _downsample(inplanes, planes * block.expansion, stride)
            stage = [block(inplanes, planes, stride, down)]
            inplanes = planes * block.expansion
            stage += [block(inplanes, planes) for _ in range(1, n)]
            setattr(self, "layer%d" % (i + 1), nn.Sequential(*stage))
        # resnet_dcn.py:213-250; the reference's nn.ReLU slots hold an Identity (no parameters either way)
        stages = []
        for planes in _DECONV_PLANES:
            fc = DCN(inplanes, planes, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1)
            use_hip_convs(fc.conv_offset_mask)
            up = ConvTranspose2d(planes, planes, 4, stride=2, padding=1, output_padding=0, bias=False)
            fill_up_weights(up)
            stages += [fc, _bn(planes, True), nn.Identity(), up, _bn(planes, True), nn.Identity()]
            inplanes = planes
        self.deconv_layers = nn.Sequential(*stages)
        # the heads: one PoseHeads (one autograd function over all of them), its per-head modules registered under this
        # module so that the state-dict keys are the reference's `hm.0.weight`, ... without a prefix
        head_block = PoseHeads(self.heads, inplanes, self.head_conv)
        for name in self.heads:
            if name in self._modules or hasattr(self, name):
                raise ValueError("PoseNetResDCN: head name %r collides with an attribute of the module" % name)
            self.add_module(name, getattr(head_block, name))
        self.__dict__["_head_block"] = head_block  # (not a sub-module: its parameters are registered above)

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError("PoseNetResDCN: x must be [B,3,H,W], got %s" % (tuple(x.shape),))
        if x.shape[2] % 32 or x.shape[3] % 32:
            raise NotImplementedError("PoseNetResDCN: H and W must be multiples of 32 (five halvings down to layer4, as the "
                                      "engine requires), got %d x %d" % (x.shape[2], x.shape[3]))
        x = self.maxpool(self.bn1(self.conv1(x)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return [self._head_block(self.deconv_layers(x))]

    @classmethod
    def from_model(cls, model):
        """A ``PoseNetResDCN`` holding copies of a ``HipPoseNet``'s current parameters and buffers (train it, then
        ``model.load_module(net)``)."""
        arch = getattr(model, "arch", None)
        depth = arch[len("resdcn_"):] if isinstance(arch, str) and arch.startswith("resdcn_") else ""
        if not depth.isdigit():
            raise NotImplementedError("PoseNetResDCN.from_model: the model is %r, not resdcn_N" % (arch,))
        net = cls(int(depth), model.heads, model.head_conv)
        net.load_state_dict(model.state_dict(), strict=True)
        return net
