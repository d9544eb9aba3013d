"""Cases and helpers of the f16x3 DCNv2 backward (cp_dcnv2_backward_prec; test helper, not a test module;
tests/test_dcn_backward_f16x3_{cpu,gpu}.py).

Dyadic cases.  Every input is a small integer over a power of two, so every product and every partial sum of the backward is a
dyadic number; where each of them fits float32's 24 bits, ANY summation order and either arithmetic mode gives the float64
reference bit for bit.  ``dyadic_case`` builds the inputs, ``dyadic_units`` the granularity (a power of two) of every gradient,
``abs_bounds`` an upper bound of every partial sum of every gradient in any order (the sums of the terms' absolute values); the
CPU test asserts bound / unit < 2^24 for every case the GPU test runs, and that the reference round-trips through float32.
The channel products C x Co differ by a factor 16 over the shapes, so w and grad_output are drawn sparse, with a density that
keeps about 32 non-zero (c, co) pairs per tap: the bounds then hold with a margin for every shape."""
import functools

import torch

from tests import dcn_backward_ref as R
from tests import dcn_det_cases as D

CP, NAMES = D.CP, D.NAMES
TOL = 1e-4   # x max |reference| per tensor: the f16x3 convolution backward's bound

# (B, C, H, W, Co), geometry CP
SHAPES = [
    (2, 16, 10, 10, 16),    # 9C = 144: ragged against 32-wide and 128-wide K tiles
    (3, 32, 9, 40, 24),     # ragged Co, odd rows, the batch case
    (2, 64, 13, 19, 64),    # a real layer's channels on a ragged map
    (1, 48, 16, 16, 80),    # neither count is a power of two
]
BATCH = SHAPES[1]
CHUNKED = D.CHUNKED         # two images fit no single chunk: per-chunk column buffer, per-call scales across chunks
STDS = [0.5, 2.0, 6.0]
LO_OPERANDS = ("w", "go", "x")   # the operand that carries k + k' 2^-12 in the two-level dyadic test
POW2 = [(-20, 7, 3, 2), (12, -30, -5, -1)]   # (a, c, b, m): x 2^a, w 2^c, grad_output 2^b, mask 2^m
# which of (a, c, b, m) each gradient contains as a factor
POW2_FACTORS = {"grad_input": (0, 1, 1, 1), "grad_offset": (1, 1, 1, 1), "grad_mask": (1, 1, 1, 0), "grad_weight": (1, 0, 1, 1),
                "grad_bias": (0, 0, 1, 0)}


def shape_id(s):
    return "x".join(map(str, s))


def gaussian_case(shape, std, seed=0):
    """tests/test_dcn_backward_gpu.py's case (masks uniform in [0, 1)) with sigmoid masks."""
    B, C, H, W, Co = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / (C * 9) ** 0.5
    b = torch.randn(Co, generator=g)
    off = std * torch.randn(B, 18, H, W, generator=g)
    mask = torch.sigmoid(torch.randn(B, 9, H, W, generator=g))
    go = torch.randn(B, Co, H, W, generator=g)
    return x, w, b, off, mask, go


def range_case(shape, factor, seed=5):
    """x, w and grad_output times `factor`, a mask drawn from [-3, 3] (no sigmoid's output)."""
    x, w, b, off, mask, go = gaussian_case(shape, 2.0, seed)
    g = torch.Generator().manual_seed(seed + 1)
    mask = 6.0 * torch.rand(mask.shape, generator=g) - 3.0
    return x * factor, w * factor, b, off, mask, go * factor


def _ints(g, shape, lo, hi, density=1.0):
    v = torch.randint(lo, hi + 1, shape, generator=g).float()
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density).float()
    return v


def dyadic_case(shape, lo_operand=None, seed=0):
    """x in {-2..2} ({-1, 0, 1} in the two-level cases), w and grad_output in {-1, 0, 1} and sparse, offsets multiples of 1/2 in
    [-3, 3] (samples leave (-1, H) x (-1, W) at the edges and land on its border), a few far outside, masks in {1/4, 1/2, 3/4, 1}.
    ``lo_operand``: that tensor gets + k' 2^-12, k' in {-1, 0, 1}, on its non-zero AND zero elements."""
    B, C, H, W, Co = shape
    g = torch.Generator().manual_seed(seed)
    density = min(1.0, (32.0 / (C * Co)) ** 0.5)
    x = _ints(g, (B, C, H, W), -1, 1) if lo_operand else _ints(g, (B, C, H, W), -2, 2)
    w = _ints(g, (Co, C, 3, 3), -1, 1, density)
    go = _ints(g, (B, Co, H, W), -1, 1, density)
    b = _ints(g, (Co,), -2, 2)
    off = _ints(g, (B, 18, H, W), -6, 6) / 2
    far = torch.rand(off.shape, generator=g) < 0.02
    off = torch.where(far, off + 4.0 * max(H, W), off)
    mask = _ints(g, (B, 9, H, W), 1, 4) / 4
    if lo_operand:
        t = {"w": w, "go": go, "x": x}[lo_operand]
        k2 = _ints(g, tuple(t.shape), -1, 1, density if lo_operand != "x" else 1.0) / 4096
        t += k2
    return x, w, b, off, mask, go


def dyadic_units(lo_operand):
    """log2 of the granularity of the five gradients (NAMES order): inputs' granularities plus those of the factors -- bilinear
    weights 2^-2 (offsets are halves), coordinate weights 2^-1, masks 2^-2."""
    gx, gw, gg = (-12 if lo_operand == n else 0 for n in ("x", "w", "go"))
    gcol, gm = gw + gg, -2
    return [gcol + gm - 2, gcol + gx - 1 + gm, gcol + gx - 2, gg + gx - 2 + gm, gg]


def abs_bounds(x, w, b, off, mask, go):
    """An upper bound of |every partial sum| of each gradient, in any order (NAMES order): the gradients of the absolute inputs
    (bilinear weights and masks are non-negative, so those ARE the sums of the terms' absolute values) -- except grad_offset, whose
    coordinate weights are signed: |cw| <= 2 max |x|, so it is bounded by 2 max |x| max |mask| sum_c |grad_col|."""
    gin, _, gmask, gw, gb = R.backward_f64(x.abs(), w.abs(), b, off, mask, go.abs(), *CP)
    Co = w.shape[0]
    s = torch.einsum("ot,bop->btp", w.abs().double().sum(1).view(Co, 9), go.abs().double().flatten(2))
    goff = 2 * float(x.abs().max()) * float(mask.abs().max()) * float(s.max())
    return [float(gin.max()), goff, float(gmask.max()), float(gw.max()), float(gb.abs().max())]


@functools.lru_cache(maxsize=None)
def reference(kind, shape, arg=None, seed=0):
    """(inputs, float64 gradients) of a case, computed once per session: kind "gaussian" (arg = std), "range" (arg = factor),
    "dyadic" (arg = lo operand or None)."""
    args = {"gaussian": lambda: gaussian_case(shape, arg, seed), "range": lambda: range_case(shape, arg),
            "dyadic": lambda: dyadic_case(shape, arg, seed)}[kind]()
    return args, R.backward_f64(*args, *CP)


def errors(got, exp):
    """max |got - exp| / max |exp| per gradient"""
    return [float((a.double() - e.double()).abs().max()) / max(float(e.double().abs().max()), 1e-300) for a, e in zip(got, exp)]
