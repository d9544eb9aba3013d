"""The reference's ConvGRU (convGRU.py) on the library's kernels, forward and backward: ``gru_gate``, ``ConvGRUCell`` and
``ConvGRU``.

``dlav1_34`` runs a one-layer ConvGRU of 3 steps (4 when tracking) between the backbone's feature map and the heads, and every
step sees the SAME input.  So the three input-side convolutions ``Wir`` / ``Wiz`` / ``Win`` run once per forward as one
64 -> 192 ``conv.conv2d`` on the concatenated weights and biases, the three hidden-side ones ``Whr`` / ``Whz`` / ``Whn`` as one
64 -> 192 convolution per step from step 1 on (the state of step 0 is zero and they have no bias: their result is zero and is
not computed), and the gate arithmetic between them is one kernel each way (``cp_gru_gate_forward`` / ``_backward``), which
keeps no gate tensor: the backward recomputes r, z and n.  ``torch.cat`` of the parameters lets autograd split the weight
gradients back onto the six ``nn.Conv2d``-shaped parameters, whose names are the reference's (``cell0.Wir.weight`` ...).

The reference's ``br`` / ``bz`` / ``bin`` / ``bhn`` tensors are zeros that are no parameters (convGRU.py:42-46) and are not kept.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import hip as _hip
from ._layers import _nhwc, _on_device
from .conv import Conv2d, conv2d


class _GruGateFn(Function):
    @staticmethod
    def forward(ctx, x3, h3, hprev):
        ctx.step0 = h3 is None
        if ctx.step0:
            x3h = _nhwc(x3)
            ctx.save_for_backward(x3h)
            out = _hip.gru_gate_forward(x3h)
        else:
            x3h, h3h, hph = _nhwc(x3), _nhwc(h3), _nhwc(hprev)
            ctx.save_for_backward(x3h, h3h, hph)
            out = _hip.gru_gate_forward(x3h, h3h, hph)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x3 = ctx.saved_tensors[0]
        h3, hprev = (None, None) if ctx.step0 else ctx.saved_tensors[1:]
        need_h3 = not ctx.step0 and ctx.needs_input_grad[1]
        need_hp = not ctx.step0 and ctx.needs_input_grad[2]
        gx3, gh3, ghp = _hip.gru_gate_backward(x3, h3, hprev, _nhwc(grad_out), need_h3_grad=need_h3, need_hprev_grad=need_hp)
        nchw = lambda t: None if t is None else t.permute(0, 3, 1, 2)
        return nchw(gx3) if ctx.needs_input_grad[0] else None, nchw(gh3), nchw(ghp)


def gru_gate(x3, h3=None, hprev=None):
    """The GRU cell behind its convolutions, on the HIP kernels with autograd: ``x3`` = [Wir x | Wiz x | Win x] (biases added)
    and ``h3`` = [Whr h | Whz h | Whn h] as logical [B,3 Ch,H,W] tensors, ``hprev`` [B,Ch,H,W] -> the new state [B,Ch,H,W]
    (channels_last), ``(1 - z) n + z hprev`` with ``r = sigmoid(x3r + h3r)``, ``z = sigmoid(x3z + h3z)``, ``n = tanh(x3n + r h3n)``.
    ``h3 = hprev = None`` is step 0: the state is zero.  ``Ch % 4 == 0``, float32."""
    _on_device(x3)
    if (h3 is None) != (hprev is None):
        raise RuntimeError("gru_gate: h3 and hprev are given together, or neither (step 0)")
    if x3.dim() != 4 or x3.shape[1] % 12:
        raise RuntimeError("gru_gate: x3 must be [B,3 Ch,H,W] with Ch %% 4 == 0, got %s" % (tuple(x3.shape),))
    ch = x3.shape[1] // 3
    if h3 is not None and (h3.shape != x3.shape or tuple(hprev.shape) != (x3.shape[0], ch) + tuple(x3.shape[2:])):
        raise RuntimeError("gru_gate: h3 %s / hprev %s do not match x3 %s" % (tuple(h3.shape), tuple(hprev.shape), tuple(x3.shape)))
    for name, t in (("x3", x3), ("h3", h3), ("hprev", hprev)):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("gru_gate: %s is %s (only float32 is built)" % (name, t.dtype))
    return _GruGateFn.apply(x3, h3, hprev)


class ConvGRUCell(nn.Module):
    """convGRU.py:7-51 with the reference's six convolutions as parameters; ``input3`` / ``forward`` split its forward into the
    part that depends on the input alone and the step."""

    def __init__(self, input_channels, hidden_channels, kernel_size):
        super().__init__()
        assert hidden_channels % 2 == 0
        self.input_channels, self.hidden_channels, self.kernel_size = input_channels, hidden_channels, kernel_size
        self.padding = int((kernel_size - 1) / 2)
        for gate in "rzn":
            setattr(self, "Wi" + gate, Conv2d(input_channels, hidden_channels, kernel_size, 1, self.padding, bias=True))
            setattr(self, "Wh" + gate, Conv2d(hidden_channels, hidden_channels, kernel_size, 1, self.padding, bias=False))

    def input3(self, x):
        """[Wir x + b | Wiz x + b | Win x + b] as one convolution"""
        w = torch.cat([self.Wir.weight, self.Wiz.weight, self.Win.weight])
        b = torch.cat([self.Wir.bias, self.Wiz.bias, self.Win.bias])
        return conv2d(x, w, b, 1, self.padding)

    def forward(self, x3, h=None):
        """One step from ``x3 = input3(x)`` and the state ``h`` (None: zero)"""
        if h is None:
            return gru_gate(x3)
        w = torch.cat([self.Whr.weight, self.Whz.weight, self.Whn.weight])
        return gru_gate(x3, conv2d(h, w, None, 1, self.padding), h)


class ConvGRU(nn.Module):
    """``ConvGRU(input_channels, hidden_channels=[64], kernel_size=3, step=1, effective_step=[1])``, convGRU.py:54-94 with one
    layer, as the reference uses it.  ``forward(input) -> (outputs, last)``: the states of the effective steps and the last
    state."""

    def __init__(self, input_channels, hidden_channels, kernel_size, step=1, effective_step=(1,)):
        super().__init__()
        hidden_channels = list(hidden_channels)
        if len(hidden_channels) != 1:
            raise NotImplementedError("ConvGRU: one layer is built (the reference's use), got hidden_channels = %r" % (hidden_channels,))
        self.input_channels = [input_channels] + hidden_channels
        self.hidden_channels, self.kernel_size, self.num_layers = hidden_channels, kernel_size, 1
        self.step, self.effective_step = int(step), list(effective_step)
        self.cell0 = ConvGRUCell(input_channels, hidden_channels[0], kernel_size)

    def forward(self, input):
        x3 = self.cell0.input3(input)  # the same at every step
        outputs, h = [], None
        for step in range(self.step):
            h = self.cell0(x3, h)
            if step in self.effective_step:
                outputs.append(h)
        return outputs, h
