"""Cases, input generators and the reference of the conv2d geometry sweep (tests/test_conv_geometry_{cpu,gpu}.py): the
operator's accepted domain away from the square, odd, same-padded kernels the other conv tests visit -- KH != KW, even kernels,
stride 3 and 4, pad above k // 2, more than 32 taps, channel counts that leave the aligned loader.

Reference: torch.nn.functional.conv2d (and a ReLU) under autograd, float64, on the CPU.

Dyadic inputs (tests/conv_backward_ref.py, with KH * KW for k * k): x, w, bias, grad_out are integers in [-2, 2].  An output sums
KH*KW*Cin products of magnitude <= 4 and a bias, grad_w sums B*Ho*Wo products, grad_x at most KH*KW*Cout, grad_bias B*Ho*Wo
values: with 4*KH*KW*Cin + 2, 4*B*Ho*Wo and 4*KH*KW*Cout all below 2^24 every partial sum, in any order, is an integer below
2^24 and exact in float32.  The device's output and gradients must therefore EQUAL the float64 reference.
"""
import collections

import torch
import torch.nn.functional as F

from tests.conv_backward_ref import Inputs, _ints, nhwc  # noqa: F401  (nhwc: for the tests)

GeoCase = collections.namedtuple("GeoCase", "B Cin Cout H W KH KW stride pad")

RECT_F16_CASES = [GeoCase(2, 32, 40, 9, 14, 1, 3, 1, 0), GeoCase(2, 32, 40, 14, 9, 3, 1, 1, 0), GeoCase(1, 64, 32, 8, 20, 1, 7, 1, 0),
                  GeoCase(2, 32, 64, 21, 8, 7, 1, 2, 0),
                  GeoCase(2, 32, 64, 11, 13, 3, 5, 1, 1),    # M = 242: two ragged M tiles
                  GeoCase(1, 32, 27, 9, 12, 3, 7, 1, 2),
                  GeoCase(1, 32, 40, 8, 9, 5, 6, 1, 2)]      # 30 taps: the top bits of the 32-bit tap mask
RECT_F32_CASES = [GeoCase(2, 16, 16, 12, 15, 5, 3, 2, 2),    # N tile 16
                  GeoCase(1, 48, 24, 7, 8, 2, 3, 1, 1)]      # three 16-channel K-steps per tap: aligned, never split-f16
SQUARE_CASES = [GeoCase(1, 32, 128, 9, 9, 5, 5, 1, 2),       # 25 taps, the mask loop, N tile 128
                GeoCase(2, 32, 32, 10, 11, 5, 5, 3, 4),      # pad 4 > k // 2, stride 3
                GeoCase(1, 32, 64, 16, 20, 4, 4, 4, 0), GeoCase(2, 64, 64, 7, 9, 4, 4, 2, 1),
                GeoCase(2, 32, 48, 9, 11, 2, 2, 2, 0),       # no window touches the last input row and column: grad_x is 0 there
                GeoCase(1, 32, 32, 6, 6, 2, 2, 1, 1),        # output larger than the input
                GeoCase(2, 32, 64, 5, 7, 3, 3, 1, 2),        # 3x3 with pad 2: not the halo kernel, not the MFMA backward
                GeoCase(1, 32, 64, 10, 13, 3, 3, 3, 0), GeoCase(1, 64, 32, 17, 9, 3, 3, 4, 1), GeoCase(2, 64, 128, 10, 13, 1, 1, 3, 0),
                GeoCase(1, 64, 128, 10, 13, 1, 1, 4, 0)]
UNALIGNED_CASES = [GeoCase(1, 32, 32, 8, 10, 6, 6, 2, 2),    # 36 taps
                   GeoCase(1, 32, 64, 14, 14, 7, 7, 2, 3),   # 49 taps at real channel counts
                   GeoCase(2, 8, 24, 9, 12, 7, 5, 1, 4),     # M = 352
                   GeoCase(1, 12, 20, 9, 11, 3, 3, 1, 1), GeoCase(1, 20, 12, 7, 10, 2, 3, 1, 1), GeoCase(1, 4, 8, 13, 6, 6, 7, 3, 5)]
# the window is the padded input (Ho = Wo = 1): almost every tap lies in the padding
WINDOW_CASES = [GeoCase(3, 32, 32, 1, 1, 5, 5, 1, 2), GeoCase(2, 32, 64, 1, 3, 7, 7, 4, 3)]
CASES = RECT_F16_CASES + RECT_F32_CASES + SQUARE_CASES + UNALIGNED_CASES + WINDOW_CASES
RECT_CASES = [c for c in CASES if c.KH != c.KW]


def case_id(c):
    return "B%d_%dto%d_%dx%d_k%dx%ds%dp%d" % c


def out_size(c):
    return (c.H + 2 * c.pad - c.KH) // c.stride + 1, (c.W + 2 * c.pad - c.KW) // c.stride + 1


def in_domain(c):
    """The operator's accepted domain, written out on its own (not through the code under test)."""
    return (1 <= c.KH <= 7 and 1 <= c.KW <= 7 and 1 <= c.stride <= 4 and 0 <= c.pad < min(c.KH, c.KW) and c.Cin >= 4
            and c.Cin % 4 == 0 and c.Cout >= 1)


def f16x3_eligible(c):
    """cp_conv2d_nhwc takes the split-f16 kernels under the "f16x3" precision for these; everything else stays float32."""
    return c.Cin % 32 == 0 and c.KH * c.KW <= 32 and c.Cout > 16


def aligned(c):
    """The implicit-GEMM forward's aligned loader (tap mask, wave-uniform tap walk); otherwise the per-lane unaligned one."""
    return c.Cin % 16 == 0 and c.KH * c.KW <= 32


def dyadic_inputs(seed, c):
    """Integer inputs in [-2, 2]; asserts the premise that makes the output and every gradient exact in float32."""
    Ho, Wo = out_size(c)
    assert Ho >= 1 and Wo >= 1
    taps = c.KH * c.KW
    assert 4 * taps * c.Cin + 2 < 2 ** 24 and 4 * c.B * Ho * Wo < 2 ** 24 and 4 * taps * c.Cout < 2 ** 24
    g = torch.Generator().manual_seed(seed)
    inp = Inputs(_ints(g, c.B, c.Cin, c.H, c.W), _ints(g, c.Cout, c.Cin, c.KH, c.KW), _ints(g, c.Cout),
                 _ints(g, c.B, c.Cout, Ho, Wo), _ints(g, c.B, c.Cout, Ho, Wo))
    for t in inp:
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 2
    assert float(inp.x.abs().max()) == 2 and bool((inp.x == -2).any()) and bool((inp.x == 2).any())
    assert bool((inp.y == 0).any()) and bool((inp.y < 0).any()) and bool((inp.y > 0).any())
    return inp


def gaussian_inputs(seed, c):
    Ho, Wo = out_size(c)
    g = torch.Generator().manual_seed(seed)
    return Inputs(torch.randn(c.B, c.Cin, c.H, c.W, generator=g),
                  torch.randn(c.Cout, c.Cin, c.KH, c.KW, generator=g) / (c.Cin * c.KH * c.KW) ** 0.5,
                  torch.randn(c.Cout, generator=g), torch.randn(c.B, c.Cout, Ho, Wo, generator=g),
                  torch.randn(c.B, c.Cout, Ho, Wo, generator=g))


def reference(x, w, bias, go, stride, pad, relu=False, dtype=torch.float64):
    """(out, grad_x, grad_w, grad_bias) of out = relu?(conv2d(x, w, bias)) by CPU autograd in ``dtype``; ``bias`` None: a zero
    bias, so grad_bias is returned all the same."""
    x, w = x.to(dtype).requires_grad_(True), w.to(dtype).requires_grad_(True)
    b = (torch.zeros(w.shape[0]) if bias is None else bias).to(dtype).requires_grad_(True)
    out = F.conv2d(x, w, b, stride, pad)
    if relu:
        out = torch.relu(out)
    return (out.detach(),) + tuple(torch.autograd.grad(out, (x, w, b), go.to(dtype)))


_exact = {}


def dyadic_reference(c, relu, has_bias):
    """The dyadic inputs of a case (seed sum(c)) and their float64 reference, computed once per (case, relu, bias) and shared by
    the tests that need them; callers leave both unchanged."""
    key = (c, bool(relu), bool(has_bias))
    if key not in _exact:
        inp = dyadic_inputs(sum(c), c)
        _exact[key] = (inp, reference(inp.x, inp.w, inp.bias if has_bias else None, inp.go, c.stride, c.pad, relu))
    return _exact[key]
