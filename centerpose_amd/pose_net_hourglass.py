"""``PoseNetHourglass``: the reference's two-stack hourglass (``exkp`` / ``HourglassNet``, large_hourglass.py:190-309) as one
trainable ``nn.Module`` whose layers all run on the library, forward and backward.

The module tree, its registration order and ``state_dict()`` are the reference's -- ``pre`` (the 7x7 stride-2 stem and a
stride-2 ``residual``), ``kps`` (one recursive ``kp_module`` per stack: ``up1`` | ``low1`` (stride 2) | ``low2`` | ``low3``),
``cnvs``, ``inters``, ``inters_``, ``cnvs_`` and one list of per-stack heads per head name (``synth.param_spec('hourglass',
...)``) -- so reference checkpoints load with ``strict=True``.  It is built from the library's layers with the documented fusions:

* ``stem.StemConv2d`` for ``pre.0.conv`` (3 -> 128, stride 2), ``conv.Conv2d`` for every other convolution,
* ``norm.BatchNorm2d`` with ``relu = True`` after a convolution, and with the skip passed in as the residual at the end of a
  ``residual`` block and where two stacks join (``relu(inters_(inter) + cnvs_(cnv))``, large_hourglass.py:284-285),
* ``upsample.UpsampleAdd`` for ``up2`` + ``merge`` of a ``kp_module`` (``max1`` is empty in the reference and stays empty),
* one ``pose_heads._PoseHeadsFn`` per stack over all of that stack's heads: conv3x3 + bias -> ReLU -> conv1x1 on the
  256-channel map, the parameters held by this module under the reference's names (``hm.0.0.conv.weight``, ``hm.0.1.weight``).

``forward(x)`` returns one head dict per stack, as the reference does in training; ``pose_loss.ObjectPoseLoss`` with
``opt.num_stacks = 2`` consumes that list.  ``PoseNetHourglass.from_model(model)`` builds one from a ``HipPoseNet`` of arch
``hourglass`` and ``model.load_module(net)`` takes it back (the engine keeps returning the last stack only).  Initial
convolution weights are ``nn.Conv2d``'s own.
"""
from collections import OrderedDict

from torch import nn

from . import synth as _synth
from ._layers import _precision_name
from .conv import Conv2d
from .norm import BatchNorm2d
from .pose_heads import _PoseHeadsFn, _Slot
from .stem import StemConv2d
from .upsample import UpsampleAdd

CNV_DIM = 256  # large_hourglass.py:192, :308


def _bn(c, relu):
    m = BatchNorm2d(c)  # nn.BatchNorm2d's defaults, as the reference builds them
    m.relu = relu
    return m


class Convolution(nn.Module):
    """large_hourglass.py:18-31 with BatchNorm: conv -> BatchNorm -> ReLU, the last two as one layer"""

    def __init__(self, k, inp_dim, out_dim, stride=1):
        super().__init__()
        if inp_dim == 3:
            self.conv = StemConv2d(inp_dim, out_dim, k, stride=stride, padding=(k - 1) // 2, bias=False)
        else:
            self.conv = Conv2d(inp_dim, out_dim, k, stride=stride, padding=(k - 1) // 2, bias=False)
        self.bn = _bn(out_dim, True)

    def forward(self, x):
        return self.bn(self.conv(x))


class Residual(nn.Module):
    """large_hourglass.py:51-77: relu(bn1(conv1)) -> relu(bn2(conv2) + skip), each a convolution and one fused layer; ``skip`` is
    the input, or conv1x1 -> BatchNorm where the stride or the width changes"""

    def __init__(self, inp_dim, out_dim, stride=1):
        super().__init__()
        self.conv1 = Conv2d(inp_dim, out_dim, 3, stride=stride, padding=1, bias=False)
        self.bn1 = _bn(out_dim, True)
        self.conv2 = Conv2d(out_dim, out_dim, 3, stride=1, padding=1, bias=False)
        self.bn2 = _bn(out_dim, True)
        self.skip = nn.Sequential()
        if stride != 1 or inp_dim != out_dim:
            self.skip = nn.Sequential(Conv2d(inp_dim, out_dim, 1, stride=stride, padding=0, bias=False), _bn(out_dim, False))

    def forward(self, x):
        out = self.bn1(self.conv1(x))
        return self.bn2(self.conv2(out), self.skip(x))


def _layer(inp_dim, out_dim, modules, stride=1):
    """make_layer (large_hourglass.py:80-84), and make_hg_layer (:290-293) with stride 2"""
    return nn.Sequential(Residual(inp_dim, out_dim, stride), *[Residual(out_dim, out_dim) for _ in range(1, modules)])


def _layer_revr(inp_dim, out_dim, modules):
    """make_layer_revr (large_hourglass.py:87-92)"""
    return nn.Sequential(*[Residual(inp_dim, inp_dim) for _ in range(modules - 1)], Residual(inp_dim, out_dim))


class KpModule(nn.Module):
    """kp_module (large_hourglass.py:130-187) as HourglassNet configures it: no pooling, ``low1`` has stride 2"""

    def __init__(self, n, dims, modules):
        super().__init__()
        curr_dim, next_dim, curr_mod, next_mod = dims[0], dims[1], modules[0], modules[1]
        self.up1 = _layer(curr_dim, curr_dim, curr_mod)
        self.max1 = nn.Sequential()
        self.low1 = _layer(curr_dim, next_dim, curr_mod, stride=2)
        self.low2 = KpModule(n - 1, dims[1:], modules[1:]) if n > 1 else _layer(next_dim, next_dim, next_mod)
        self.low3 = _layer_revr(next_dim, curr_dim, curr_mod)
        self.merge = UpsampleAdd()  # up2 and merge in one pass

    def forward(self, x):
        return self.merge(self.up1(x), self.low3(self.low2(self.low1(x))))


def _head(classes, is_hm):
    """make_kp_layer (large_hourglass.py:115-119) as parameter holders under the reference's indices: ``0.conv`` (3x3 + bias, the
    ReLU behind it) and ``1`` (1x1).  nn.Conv2d's initial weights; the final bias of a heat-map head is -2.19 (:255-256)."""
    c0, c1 = nn.Conv2d(CNV_DIM, CNV_DIM, 3, padding=1), nn.Conv2d(CNV_DIM, int(classes), 1)
    if is_hm:
        nn.init.constant_(c1.bias, -2.19)
    hidden = nn.Module()
    hidden.add_module("conv", _Slot(c0.weight.detach().clone(), c0.bias.detach().clone()))
    seq = nn.Module()
    seq.add_module("0", hidden)
    seq.add_module("1", _Slot(c1.weight.detach().clone(), c1.bias.detach().clone()))
    return seq


class PoseNetHourglass(nn.Module):
    """``PoseNetHourglass(heads, opt=None, n=5, dims=synth.HG_DIMS, modules=synth.HG_MODULES, num_stacks=2)``: ``hourglass``.
    ``heads`` maps head name -> classes (``opt.heads``); the structural arguments are ``exkp``'s own and default to the
    reference network.  ``forward(x)`` takes an NCHW image batch on the device, H and W multiples of ``4 * 2**n``, and returns
    a list of ``num_stacks`` dicts of raw head maps.  ``eval()`` runs the same layers on the running statistics."""
    arch = "hourglass"
    heads_backward_precision = "f32"  # the heads' backward arithmetic (pose_heads.set_backward_precision)

    def __init__(self, heads, opt=None, n=5, dims=_synth.HG_DIMS, modules=_synth.HG_MODULES, num_stacks=2):
        super().__init__()
        dims, modules = list(dims), list(modules)
        if n < 1 or len(dims) != n + 1 or len(modules) != n + 1:
            raise ValueError("PoseNetHourglass: dims and modules must have n + 1 = %d entries, got %d and %d"
                             % (n + 1, len(dims), len(modules)))
        if dims[0] != CNV_DIM:
            raise NotImplementedError("PoseNetHourglass: dims[0] must be %d (the heads' feature map), got %d" % (CNV_DIM, dims[0]))
        if num_stacks < 1:
            raise ValueError("PoseNetHourglass: num_stacks must be at least 1, got %d" % num_stacks)
        self.heads = OrderedDict(heads)
        self.n, self.nstack = int(n), int(num_stacks)
        curr_dim = dims[0]
        self.pre = nn.Sequential(Convolution(7, 3, 128, stride=2), Residual(128, 256, stride=2))
        self.kps = nn.ModuleList([KpModule(n, dims, modules) for _ in range(self.nstack)])
        self.cnvs = nn.ModuleList([Convolution(3, curr_dim, CNV_DIM) for _ in range(self.nstack)])
        self.inters = nn.ModuleList([Residual(curr_dim, curr_dim) for _ in range(self.nstack - 1)])
        self.inters_ = nn.ModuleList([nn.Sequential(Conv2d(curr_dim, curr_dim, 1, bias=False), _bn(curr_dim, False))
                                      for _ in range(self.nstack - 1)])
        # the join's ReLU and add run inside this BatchNorm: relu(cnvs_(cnv) + inters_(inter))
        self.cnvs_ = nn.ModuleList([nn.Sequential(Conv2d(CNV_DIM, curr_dim, 1, bias=False), _bn(curr_dim, True))
                                    for _ in range(self.nstack - 1)])
        for name, classes in self.heads.items():
            if name in self._modules or hasattr(self, name):
                raise ValueError("PoseNetHourglass: head name %r collides with an attribute of the module" % name)
            if not 1 <= int(classes) <= 64:
                raise NotImplementedError("PoseNetHourglass: head %r has %d classes (1..64 are built)" % (name, classes))
            self.add_module(name, nn.ModuleList([_head(classes, "hm" in name) for _ in range(self.nstack)]))

    def _head_params(self, k):
        flat = []
        for name in self.heads:
            seq = getattr(self, name)[k]
            a, b = getattr(seq, "0").conv, getattr(seq, "1")
            flat += [a.weight, a.bias, b.weight, b.bias]
        return flat

    def forward(self, x):
        unit = 4 * 2 ** self.n
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError("PoseNetHourglass: x must be [B,3,H,W], got %s" % (tuple(x.shape),))
        if x.shape[2] % unit or x.shape[3] % unit:
            raise RuntimeError("PoseNetHourglass: H and W must be multiples of %d (4 x 2^n: the stem, pre.1 and %d halvings), got "
                               "%d x %d" % (unit, self.n, x.shape[2], x.shape[3]))
        inter = self.pre(x)
        outs = []
        for k in range(self.nstack):
            cnv = self.cnvs[k](self.kps[k](inter))
            # all heads of the stack in one autograd function (pose_heads.py), on this module's own parameters
            outs.append(OrderedDict(zip(self.heads, _PoseHeadsFn.apply(cnv, _precision_name(self.heads_backward_precision), *self._head_params(k)))))
            if k < self.nstack - 1:
                a, b = self.inters_[k], self.cnvs_[k]
                inter = self.inters[k](b[1](b[0](cnv), a[1](a[0](inter))))
        return outs

    @classmethod
    def from_model(cls, model):
        """A ``PoseNetHourglass`` holding copies of a ``HipPoseNet``'s current parameters and buffers (train it, then
        ``model.load_module(net)``)."""
        if getattr(model, "arch", None) != cls.arch:
            raise NotImplementedError("PoseNetHourglass.from_model: the model is %r, not %s" % (getattr(model, "arch", None), cls.arch))
        net = cls(model.heads, model.opt)
        net.load_state_dict(model.state_dict(), strict=True)
        return net
