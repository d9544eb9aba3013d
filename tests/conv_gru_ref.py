"""Reference of the ConvGRU tests (tests/test_conv_gru_{cpu,gpu}.py): the gate arithmetic of convGRU.py:32-39 on
pre-computed convolution outputs, and a functional restatement of ConvGRU.forward (convGRU.py:72-94) with the reference's six
separate convolutions, both in any float dtype under CPU autograd.  The reference's br / bz / bin / bhn are zeros and are left
out."""
import collections

import torch
import torch.nn.functional as F

TOL = 1e-4        # x max |reference| per output: the project's gradient tolerance
TOL_LAYERS = 1e-3  # the multi-layer limit (tests/test_conv_backward_gpu.py's block)
# (M, Ch): one row; a ragged count below a workgroup; 4 x 37 x 45 rows, many workgroups; the narrowest and a wide state
GATE_CASES = [(1, 64), (63, 64), (4 * 37 * 45, 64), (35, 4), (35, 128)]


def gate(x3, h3, hprev):
    """x3, h3 [M, 3 Ch], hprev [M, Ch]; h3 = hprev = None: step 0"""
    ch = x3.shape[-1] // 3
    xr, xz, xn = x3[..., :ch], x3[..., ch:2 * ch], x3[..., 2 * ch:]
    if h3 is None:
        hr = hz = hn = hprev = torch.zeros_like(xr)
    else:
        hr, hz, hn = h3[..., :ch], h3[..., ch:2 * ch], h3[..., 2 * ch:]
    r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
    n = torch.tanh(xn + r * hn)
    return (1 - z) * n + z * hprev


GateInputs = collections.namedtuple("GateInputs", "x3 h3 hprev go")


def gate_inputs(seed, M, Ch):
    g = torch.Generator().manual_seed(seed)
    return GateInputs(torch.randn(M, 3 * Ch, generator=g), torch.randn(M, 3 * Ch, generator=g), torch.randn(M, Ch, generator=g),
                      torch.randn(M, Ch, generator=g))


def gate_reference(inp, step0, dtype=torch.float64):
    """dict of hout, grad_x3, grad_h3, grad_hprev (the last two None at step 0)"""
    x3 = inp.x3.to(dtype).requires_grad_(True)
    h3 = None if step0 else inp.h3.to(dtype).requires_grad_(True)
    hp = None if step0 else inp.hprev.to(dtype).requires_grad_(True)
    out = gate(x3, h3, hp)
    grads = torch.autograd.grad(out, [x3] if step0 else [x3, h3, hp], inp.go.to(dtype))
    return dict(hout=out.detach(), grad_x3=grads[0], grad_h3=None if step0 else grads[1], grad_hprev=None if step0 else grads[2])


def conv_gru(sd, x, steps, prefix="cell0."):
    """ConvGRU.forward with one layer: the list of the states after every step"""
    conv = lambda t, name: F.conv2d(t, sd[prefix + name + ".weight"], sd.get(prefix + name + ".bias"), padding=1)
    h = torch.zeros_like(x[:, :sd[prefix + "Whr.weight"].shape[0]])
    outs = []
    for _ in range(steps):
        r = torch.sigmoid(conv(x, "Wir") + conv(h, "Whr"))
        z = torch.sigmoid(conv(x, "Wiz") + conv(h, "Whz"))
        n = torch.tanh(conv(x, "Win") + r * conv(h, "Whn"))
        h = (1 - z) * n + z * h
        outs.append(h)
    return outs
