"""Cases, inputs and references of the f16x3 dense ConvTranspose2d backward suites (tests/test_deconv_backward_f16x3_cpu.py,
tests/test_deconv_backward_f16x3_gpu.py; test helper, not a test module).  The numeric premises are tests/f16x3_common.py's.

A dense layer ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1) on x [B,Cin,H,W]:
  grad_w[ci][co][tap] sums B H W products x * grad_out                     (reduction length B H W)
  grad_x[b][ci][y][x] sums 16 Cout products grad_out * w (every tap of the 4x4 / stride-2 convolution of grad_out; taps that
                      fall outside the grid are zeros)                     (reduction length 16 Cout)
"""
import functools

import torch
import torch.nn.functional as F

from tests import deconv_backward_ref as R
from tests.f16x3_common import TWO_LEVEL_MAX_SUM, _two, _unit

NAMES = ("grad_x", "grad_w")


def wgrad_plan(c):
    """(jobs, rows per slab, slabs) of the weight gradient's launch plan (csrc/conv_bwd.hip: cp_conv_wgrad_plan and slab_plan,
    called by csrc/deconv_bwd.hip with rows = B H, the convolution's input channels = Cout, its output channels = Cin and 16
    taps), restated: about 2048 wave jobs, at most 512 slabs, at most 64 MiB of slabs, at most one slab per row."""
    nh = 4 if c.Cin % 128 == 0 else 2 if c.Cin % 64 == 0 else 1
    kt = 16 * c.Cout // 32
    jobs = (c.Cin // (32 * nh)) * ((kt + 1) // 2)
    rows = c.B * c.H
    ns = min(512, (2048 + jobs - 1) // jobs)
    ns = min(ns, max(1, (64 << 20) // (c.Cin * 16 * c.Cout * 4)))
    ns = max(1, min(ns, rows))
    per = (rows + ns - 1) // ns
    return jobs, per, (rows + per - 1) // per


# (B, Cin, Cout, H, W) -> deconv_backward_ref.dense(B, H, W, Cin, Cout)
CASES = [R.dense(2, 2, 3, 256, 256),    # resdcn's first deconv at the network test's size: 2 x 3 map, four co tiles per wave
         R.dense(1, 5, 7, 64, 32),      # odd grid, two co tiles per wave, one N tile of 32 in the data gradient
         R.dense(2, 8, 8, 32, 96),      # one co tile per wave, 48 k tiles
         R.dense(3, 3, 17, 128, 64),    # a row of 17: one full step of 16 pixels and a ragged one
         R.dense(2, 9, 5, 32, 32)]      # 18 rows in 18 slabs: both levels of the slab sum (8 lanes, then lane order)
assert wgrad_plan(CASES[4])[2] == 18 and wgrad_plan(CASES[0])[2] == 4

# every partial sum of two-level values is exact in float32 up to TWO_LEVEL_MAX_SUM terms
TWO_LEVEL_CASES = [c for c in CASES if c.B * c.H * c.W <= TWO_LEVEL_MAX_SUM and 16 * c.Cout <= TWO_LEVEL_MAX_SUM]


def make_inputs(kind, seed, c):
    """R.Inputs (logical NCHW float32): "dyadic" {-1, 0, 1} everywhere; "two_xw" two-level x and w with unit grad_out; "two_go" the
    other way round; "gauss" N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    xs, ws, gs = (c.B, c.Cin, c.H, c.W), (c.Cin, c.Cout, 4, 4), (c.B, c.Cout, 2 * c.H, 2 * c.W)
    if kind == "gauss":
        return R.Inputs(torch.randn(xs, generator=g), torch.randn(ws, generator=g), None, torch.randn(gs, generator=g))
    fx = _two if kind == "two_xw" else _unit
    fg = _two if kind == "two_go" else _unit
    return R.Inputs(fx(g, *xs), fx(g, *ws), None, fg(g, *gs))


@functools.lru_cache(maxsize=None)
def cached_inputs(kind, seed, c):
    return make_inputs(kind, seed, c)


@functools.lru_cache(maxsize=None)
def cached_reference(kind, seed, c):
    """(grad_x, grad_w) by float64 CPU autograd, logical NCHW.  Shared: callers do not modify it."""
    inp = cached_inputs(kind, seed, c)
    x, w = inp.x.double().requires_grad_(True), inp.w.double().requires_grad_(True)
    return torch.autograd.grad(F.conv_transpose2d(x, w, None, 2, 1), (x, w), inp.go.double())


def device_backward(device, c, inp, precision="f16x3", need_x_grad=True):
    """(grad_x | None, grad_w) of hip.ops.conv_transpose2d_backward as CPU tensors, grad_x logical NCHW."""
    from centerpose_amd import hip
    gx, gw = hip.ops.conv_transpose2d_backward(R.nhwc(inp.x).to(device), inp.w.to(device), R.nhwc(inp.go).to(device), c.stride,
                                               c.pad, c.groups, need_x_grad=need_x_grad, precision=precision)
    return (None if gx is None else R.nchw(gx).cpu()), gw.cpu()


def assert_mask(c, want=3):
    from centerpose_amd import hip
    got = hip.lib().cp_conv_transpose2d_backward_prec_mask(*R.geo(c), hip.PRECISIONS["f16x3"])
    assert got == want, (R.case_id(c), got)


def errors(got, exp):
    return [(n, float((a.double() - e).abs().max()), float(e.abs().max())) for n, a, e in zip(NAMES, got, exp)]


def assert_equal(got, exp, what):
    for n, a, e in zip(NAMES, got, exp):
        assert torch.equal(a.double(), e), (what, n, float((a.double() - e).abs().max()))


def assert_close(got, exp, tol, what):
    for n, err, scale in errors(got, exp):
        assert scale > 0 and err <= tol * scale, (what, n, err, scale)
