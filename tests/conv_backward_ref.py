"""Cases, input generators and the reference of the Conv2d backward tests (tests/test_conv_backward_{cpu,gpu}.py).

Reference: torch.nn.functional.conv2d under autograd, float64, on the CPU -- what the reference project's layers call.  For
the gated form (the layer ended in a ReLU) ``grad_out * (y > 0)`` is fed to it.

Dyadic inputs: x, w, grad_out (and y, bias) are integers in [-2, 2].  Every product is then an integer of magnitude <= 4,
grad_w sums B*Ho*Wo of them, grad_x at most K*K*Cout, grad_bias B*Ho*Wo values of magnitude <= 2: with 4 * B*Ho*Wo < 2^24 and
4 * K*K*Cout < 2^24 every partial sum of every gradient, in any order, is an integer below 2^24 and exact in float32.  The
device's gradients must therefore EQUAL the float64 reference: a tolerance of zero that is a property of the inputs, not a
measurement, and any wrong tap, parity class, halo, pad lane or slab breaks it.
"""
import collections

import torch
import torch.nn.functional as F

Case = collections.namedtuple("Case", "B Cin Cout H W k stride pad")


def _c(B, Cin, Cout, H, W, k, stride, pad=None):
    return Case(B, Cin, Cout, H, W, k, stride, k // 2 if pad is None else pad)


MFMA_CASES = [_c(2, 64, 64, 128, 128, 3, 1), _c(2, 32, 64, 37, 45, 3, 2), _c(2, 64, 128, 64, 64, 3, 2), _c(1, 256, 512, 32, 32, 3, 2),
              _c(2, 512, 512, 16, 16, 3, 1), _c(2, 128, 64, 33, 20, 1, 1), _c(1, 448, 128, 64, 64, 1, 1), _c(1, 64, 128, 31, 31, 1, 2),
              _c(3, 32, 32, 1, 1, 3, 1), _c(1, 32, 32, 2, 3, 3, 2),
              # slab counts around the eight lanes of the two-level slab sum (a lane without a slab, one each, one lane with
              # two); Cout 40 also has pad lanes and an element tail in the 32-wide groups.
              # 1x1: weight-gradient slabs = output rows = 7, 8, 9
              _c(1, 32, 40, 7, 7, 1, 1), _c(1, 32, 40, 8, 8, 1, 1), _c(1, 32, 40, 9, 9, 1, 1),
              # 3x3: stage / bias slabs 7, 8, 9 (Q = 441, 506, 552 output pixels)
              _c(1, 32, 40, 21, 21, 3, 1), _c(1, 32, 40, 22, 23, 3, 1), _c(1, 32, 40, 23, 24, 3, 1)]
PADDED_CASES = [_c(2, 64, 27, 40, 40, 3, 1), _c(1, 128, 27, 64, 64, 3, 1)]
GENERIC_CASES = [_c(2, 16, 32, 50, 50, 3, 2), _c(1, 4, 16, 64, 64, 7, 1), _c(1, 36, 20, 17, 23, 3, 1), _c(1, 8, 8, 29, 31, 5, 3, 2),
                 _c(1, 64, 64, 20, 20, 3, 1, 0)]
CASES = MFMA_CASES + PADDED_CASES + GENERIC_CASES


def case_id(c):
    return "B%d_%dto%d_%dx%d_k%ds%dp%d" % c


def out_size(c):
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def is_mfma(c):
    return c.k in (1, 3) and c.stride in (1, 2) and c.pad == c.k // 2 and c.Cin % 32 == 0


def dla34_shapes(B):
    """dla_34's convolution geometries at a 512 x 512 input (tools/conv_backward_bench.py) as Cases."""
    from tools.conv_backward_bench import DLA34_512

    return [_c(B, cin, cout, r, r, k, s) for _, cin, cout, r, k, s in DLA34_512]


Inputs = collections.namedtuple("Inputs", "x w bias go y")   # logical NCHW float32 tensors; y: a stand-in forward output


def _ints(g, *shape):
    return torch.randint(-2, 3, shape, generator=g).float()


def dyadic_inputs(seed, c):
    """Integer inputs in [-2, 2]; asserts the premise that makes every gradient exact in float32 (module docstring)."""
    Ho, Wo = out_size(c)
    assert Ho >= 1 and Wo >= 1
    assert 4 * c.B * Ho * Wo < 2 ** 24 and 4 * c.k * c.k * c.Cout < 2 ** 24 and 4 * c.k * c.k * c.Cin + 2 < 2 ** 24
    g = torch.Generator().manual_seed(seed)
    inp = Inputs(_ints(g, c.B, c.Cin, c.H, c.W), _ints(g, c.Cout, c.Cin, c.k, c.k), _ints(g, c.Cout),
                 _ints(g, c.B, c.Cout, Ho, Wo), _ints(g, c.B, c.Cout, Ho, Wo))
    for t in inp:
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 2
    assert bool((inp.y == 0).any()) and bool((inp.y < 0).any()) and bool((inp.y > 0).any())
    return inp


def gaussian_inputs(seed, c):
    Ho, Wo = out_size(c)
    g = torch.Generator().manual_seed(seed)
    return Inputs(torch.randn(c.B, c.Cin, c.H, c.W, generator=g), torch.randn(c.Cout, c.Cin, c.k, c.k, generator=g) / (c.Cin * c.k * c.k) ** 0.5,
                  torch.randn(c.Cout, generator=g), torch.randn(c.B, c.Cout, Ho, Wo, generator=g),
                  torch.randn(c.B, c.Cout, Ho, Wo, generator=g))


def reference(x, w, go, stride, pad, y=None, dtype=torch.float64):
    """(grad_x, grad_w, grad_bias) of out = conv2d(x, w) + bias by CPU autograd in ``dtype``; ``y``: gate grad_out by y > 0."""
    x, w = x.to(dtype).requires_grad_(True), w.to(dtype).requires_grad_(True)
    b = torch.zeros(w.shape[0], dtype=dtype, requires_grad=True)
    out = F.conv2d(x, w, b, stride, pad)
    g = go.to(dtype)
    if y is not None:
        g = torch.where(y <= 0, torch.zeros_like(g), g)   # torch's threshold_backward: a NaN y passes the gradient
    return torch.autograd.grad(out, (x, w, b), g)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def device_backward(device, c, inp, gated, need_x_grad=True, need_bias_grad=True):
    """hip.conv2d_backward on the case; returns (grad_x NCHW | None, grad_w, grad_bias | None) on the CPU."""
    from centerpose_amd import hip

    gx, gw, gb = hip.conv2d_backward(nhwc(inp.x).to(device), inp.w.to(device), nhwc(inp.go).to(device), stride=c.stride, pad=c.pad,
                                     y=nhwc(inp.y).to(device) if gated else None, need_x_grad=need_x_grad,
                                     need_bias_grad=need_bias_grad)
    return (gx.permute(0, 3, 1, 2).cpu() if gx is not None else None, gw.cpu(), gb.cpu() if gb is not None else None)
