"""Cases, input generators and helpers of the f16x3 Conv2d backward tests (tests/test_conv_backward_f16x3_{cpu,gpu}.py).

The mode (cp_conv2d_backward_prec_nhwc with CP_PREC_F16X3) pre-scales grad_out, x and w by exact powers of two, splits each
value into two binary16 numbers hi + lo (hi rounded towards zero to 11 bits, lo the rounded residual) and sums
hi*hi + hi*lo + lo*hi in float32.  Three kinds of inputs:

* dyadic (tests/conv_backward_ref.py): integers in [-2, 2] have no lo part, so the gradients must EQUAL the float64 reference.
* two-level dyadic: one operand of each contraction holds values a + b * 2^-12 with a, b in {-1, 0, 1}, the other integers in
  {-1, 0, 1}.  Such a value is exactly hi + lo with a non-zero lo whenever a and b are both non-zero, so each product is exactly
  hi*hi + lo*hi (or hi*hi + hi*lo): a multiple of 2^-12 of magnitude at most 1 + 2^-12.  With every reduction length
  (B*Ho*Wo for grad_w and grad_bias, k*k*CoP for grad_x) at most 4000, every partial sum in any order is a multiple of 2^-12
  below 2^12, hence exact in float32: the gradients must again EQUAL the float64 reference, and a dropped cross term cannot.
* Gaussian: within 1e-4 x max |reference| per gradient, the project's gradient tolerance (tests/test_conv_backward_gpu.py).
"""
import functools

import torch

from tests import conv_backward_ref as R
from tests.f16x3_common import TWO_LEVEL_MAX_SUM, TWO_LEVEL_VALUES, _two, _unit, np_scale, np_split  # noqa: F401  (reached as C.*)

NAMES = ("grad_x", "grad_w", "grad_bias")

# every MFMA case of the float32 tests no larger than 64 x 64 (B3_32to32_1x1 and B1_32to32_2x3 s2, the smallest maps, among
# them), and the padded ones
BASE_CASES = [c for c in R.CASES if R.is_mfma(c) and c.H <= 64 and c.W <= 64]
assert all(c in BASE_CASES for c in R.PADDED_CASES)
assert R.Case(3, 32, 32, 1, 1, 3, 1, 1) in BASE_CASES and R.Case(1, 32, 32, 2, 3, 3, 2, 1) in BASE_CASES


def _kstep(wo, k, stride):
    """A case with ``wo`` output columns: around the 16-pixel K step of the weight-gradient kernel."""
    w = wo if stride == 1 else 2 * wo - 1
    return R.Case(1, 32, 40, 5 if stride == 1 else 6, w, k, stride, k // 2)


KSTEP_CASES = [_kstep(wo, k, s) for (k, s) in ((3, 1), (3, 2), (1, 2)) for wo in (15, 16, 17, 31, 33)]
for _c in KSTEP_CASES:
    assert R.out_size(_c)[1] in (15, 16, 17, 31, 33) and R.is_mfma(_c)
CASES = BASE_CASES + KSTEP_CASES

# the MFMA geometries of tests/test_conv_backward_gpu.py's MODULE_CASES
MODULE_CASES = [R.Case(2, 64, 64, 16, 16, 3, 1, 1), R.Case(2, 32, 27, 9, 11, 3, 1, 1), R.Case(2, 64, 128, 13, 13, 1, 2, 0),
                R.Case(1, 32, 64, 12, 9, 3, 2, 1)]
assert all(R.is_mfma(c) for c in MODULE_CASES)

def cop(c):
    return (c.Cout + 31) // 32 * 32


def two_level_ok(c):
    """The premise of the two-level inputs holds for the case (module docstring)."""
    Ho, Wo = R.out_size(c)
    return c.B * Ho * Wo <= TWO_LEVEL_MAX_SUM and c.k * c.k * cop(c) <= TWO_LEVEL_MAX_SUM


TWO_LEVEL_CASES = [c for c in CASES if two_level_ok(c)]
assert len(TWO_LEVEL_CASES) >= 20 and any(c.stride == 1 and c.k == 3 for c in TWO_LEVEL_CASES)

def two_level_inputs(seed, c, which):
    """``which`` == "xw": x and w two-level, grad_out integer; "go": grad_out two-level, x and w integer.  Asserts the premise."""
    assert two_level_ok(c) and which in ("xw", "go")
    Ho, Wo = R.out_size(c)
    g = torch.Generator().manual_seed(seed)
    fine, coarse = (_two, _unit) if which == "xw" else (_unit, _two)
    inp = R.Inputs(fine(g, c.B, c.Cin, c.H, c.W), fine(g, c.Cout, c.Cin, c.k, c.k), _unit(g, c.Cout), coarse(g, c.B, c.Cout, Ho, Wo),
                   _unit(g, c.B, c.Cout, Ho, Wo))
    vals = set(TWO_LEVEL_VALUES)
    for t in (inp.x, inp.w, inp.go):
        assert set(t.double().unique().tolist()) <= vals
    for t in ((inp.go,) if which == "xw" else (inp.x, inp.w)):
        assert torch.equal(t, t.round())
    # (all but the tiniest tensors hold values with both parts: a non-zero lo half exists)
    return inp


def geo(c):
    return (c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.stride, c.pad)


def assert_f16x3(c):
    """Both contractions of the case run in f16x3: a silent float32 fallback cannot pass a test that calls this first."""
    from centerpose_amd import hip

    assert hip.ops.conv2d_backward_precision_mask(*geo(c), precision="f16x3") == 3, c
    assert hip.ops.conv2d_backward_precision_mask(*geo(c), precision="f32") == 0, c


def device_backward(device, c, inp, gated, precision="f16x3", need_x_grad=True, need_bias_grad=True):
    """hip.ops.conv2d_backward_prec on the case in ``precision``; (grad_x NCHW | None, grad_w, grad_bias | None) on the CPU."""
    from centerpose_amd import hip

    gx, gw, gb = hip.ops.conv2d_backward_prec(R.nhwc(inp.x).to(device), inp.w.to(device), R.nhwc(inp.go).to(device), stride=c.stride,
                                     pad=c.pad, y=R.nhwc(inp.y).to(device) if gated else None, need_x_grad=need_x_grad,
                                     need_bias_grad=need_bias_grad, precision=precision)
    return (gx.permute(0, 3, 1, 2).cpu() if gx is not None else None, gw.cpu(), gb.cpu() if gb is not None else None)


@functools.lru_cache(maxsize=None)
def cached_inputs(kind, seed, c):
    """Inputs shared between tests (never modified): kind "dyadic", "gauss", "two_xw" or "two_go"."""
    if kind == "dyadic":
        return R.dyadic_inputs(seed, c)
    if kind == "gauss":
        return R.gaussian_inputs(seed, c)
    return two_level_inputs(seed, c, kind[4:])


@functools.lru_cache(maxsize=None)
def cached_reference(kind, seed, c, gated):
    inp = cached_inputs(kind, seed, c)
    return R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, inp.y if gated else None)


def errors(got, exp):
    """[(name, max |got - exp|, max |exp|)] per gradient."""
    return [(n, float((a.double() - e.double()).abs().max()), float(e.abs().max())) for n, a, e in zip(NAMES, got, exp)]


def assert_close(got, exp, tol, what):
    """tests/test_conv_backward_gpu.py's rule: per gradient, max error <= tol x max |reference|."""
    for (name, err, scale), a, e in zip(errors(got, exp), got, exp):
        assert a.shape == e.shape, (what, name)
        print("%s %s: max err %.3g, max |ref| %.3g" % (what, name, err, scale))
        assert err <= tol * scale + 1e-300, "%s %s: max err %.3g vs max |ref| %.3g" % (what, name, err, scale)


def assert_equal(got, exp, what):
    for name, a, e in zip(NAMES, got, exp):
        bad = int((a.double() != e.double()).sum())
        print("%s %s: %d of %d differ" % (what, name, bad, e.numel()))
        assert a.shape == e.shape and bad == 0, (what, name, bad)
