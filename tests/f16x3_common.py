"""The numeric premises the f16x3 backward test suites share (tests/conv_backward_f16x3_cases.py,
tests/pose_heads_f16x3_cases.py; test helper, not a test module): the two-level dyadic values and their generators, the bound
on a reduction length under which every partial sum of such values is exact in float32, and a numpy restatement of the
device's scale and split.

The mode pre-scales each operand by an exact power of two, splits each value into two binary16 numbers hi + lo (hi rounded
towards zero to 11 bits, lo the rounded residual) and sums hi*hi + hi*lo + lo*hi in float32.  A two-level value a + b * 2^-12
with a, b in {-1, 0, 1} is exactly hi + lo, with a non-zero lo whenever a and b are both non-zero; its product with a value in
{-1, 0, 1} is a multiple of 2^-12 of magnitude at most 1 + 2^-12, so with at most TWO_LEVEL_MAX_SUM terms every partial sum in
any order is a multiple of 2^-12 below 2^12, hence exact in float32.
"""
import numpy as np
import torch

TWO_LEVEL_MAX_SUM = 4000
TWO_LEVEL_VALUES = sorted({a + b * 2.0 ** -12 for a in (-1, 0, 1) for b in (-1, 0, 1)})


def _two(g, *shape):
    a = torch.randint(-1, 2, shape, generator=g).double()
    b = torch.randint(-1, 2, shape, generator=g).double()
    return (a + b * 2.0 ** -12).float()


def _unit(g, *shape):
    return torch.randint(-1, 2, shape, generator=g).float()


# ---- a numpy restatement of the device's scale and split (csrc/cp_common.h: cp_amax_to_scale; igemm16_common.h: split2) ----
def np_scale(amax):
    """2^e with amax * 2^e in [2^14, 2^15) (clamped as the device clamps)."""
    bits = int(np.float32(amax).view(np.uint32))
    e = min(max((bits >> 23) & 0xff, 16), 253)
    return float(np.uint32((268 - e) << 23).view(np.float32))


def np_split(v):
    """float32 array -> (hi, lo) as float64: hi = v rounded towards zero to binary16's 11 significant bits (normal range), lo =
    the residual rounded to binary16 (nearest even)."""
    v = np.asarray(v, dtype=np.float32)
    hi = (v.view(np.uint32) & np.uint32(0xffffe000)).view(np.float32)
    assert np.all(hi.astype(np.float16).astype(np.float32) == hi)   # representable: inside binary16's normal range
    lo = (v - hi).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)
