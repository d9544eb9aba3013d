"""Reference and cases of the ConvTranspose2d training tests: ``F.conv_transpose2d`` (+ ``add``) under float64 CPU autograd on
float32 inputs drawn from N(0, 1).  The weights are random too: with ``fill_up_weights``' symmetric bilinear kernel a swapped
tap would go unseen."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

# 1e-4 x max |reference| per output: the project's gradient tolerance (tests/batchnorm_ref.py: TOL, tests/test_conv_backward_gpu.py)
TOL = 1e-4

Case = namedtuple("Case", "B H W Cin Cout K stride pad groups")


def dw(B, H, W, C, f):
    return Case(B, H, W, C, C, 2 * f, f, f // 2, C)


def dense(B, H, W, Cin, Cout):
    return Case(B, H, W, Cin, Cout, 4, 2, 1, 1)


DW_CASES = [dw(1, 1, 1, 4, 2),      # one source pixel, every tap at an edge
            dw(2, 3, 5, 20, 2),     # five lanes per pixel; does not divide a wave
            dw(1, 2, 3, 8, 4),      # f = 4 at the minimum
            dw(3, 9, 11, 64, 2),    # ragged grid
            dw(2, 5, 7, 64, 4),     # the f = 4 layer's width
            dw(1, 7, 9, 256, 2),    # the widest weight table
            dw(2, 33, 31, 64, 2),   # several slabs, ragged
            dw(1, 64, 64, 64, 2),   # the workload's row length
            # slab counts around the eight lanes of the two-level slab sum: 7, 8, 9 slabs
            dw(1, 28, 28, 64, 2), dw(1, 32, 32, 64, 2), dw(1, 33, 33, 64, 2),
            # the same 7, 8, 9 slabs on the four-tap-group instance
            dw(1, 28, 28, 16, 4), dw(1, 32, 32, 16, 4), dw(1, 33, 33, 16, 4)]
DENSE_CASES = [dense(1, 1, 1, 32, 32),       # minimum shape
               dense(2, 3, 5, 32, 64),       # unequal channel counts
               dense(2, 7, 9, 64, 32),       # the other way round
               dense(3, 13, 11, 64, 64),     # ragged
               dense(1, 16, 16, 128, 128),   # four co tiles per wave
               dense(2, 5, 6, 96, 96)]       # one co tile per wave, three k tile pairs


def case_id(c):
    return ("dw_%dx%dx%dx%d_f%d" % (c.B, c.H, c.W, c.Cin, c.stride) if c.groups != 1
            else "dense_%dx%dx%dx%dto%d" % (c.B, c.H, c.W, c.Cin, c.Cout))


def geo(c):
    """The geometry arguments of the C ABI's backward call and query, in order."""
    return (c.B, c.H, c.W, c.Cin, c.Cout, c.K, c.stride, c.pad, c.groups)


Inputs = namedtuple("Inputs", "x w add go")  # logical NCHW float32 CPU tensors; add is None for dense cases


def inputs(seed, c):
    g = torch.Generator().manual_seed(1000 * seed + 17 * c.B + 5 * c.H + 3 * c.W + c.Cin + c.stride)
    out = (c.B, c.Cout, c.stride * c.H, c.stride * c.W)
    x = torch.randn(c.B, c.Cin, c.H, c.W, generator=g)
    w = torch.randn(c.Cin, c.Cout // c.groups, c.K, c.K, generator=g)
    add = torch.randn(out, generator=g) if c.groups != 1 else None
    go = torch.randn(out, generator=g)
    return Inputs(x, w, add, go)


@functools.lru_cache(maxsize=None)
def reference(seed, c):
    """float64 CPU autograd: dict(y, y_add (depth-wise), grad_x, grad_w), logical NCHW.  Computed once per (seed, case) and shared:
    callers do not modify it."""
    inp = inputs(seed, c)
    x = inp.x.double().requires_grad_(True)
    w = inp.w.double().requires_grad_(True)
    y = F.conv_transpose2d(x, w, None, c.stride, c.pad, groups=c.groups)
    gx, gw = torch.autograd.grad(y, (x, w), inp.go.double())
    ref = dict(y=y.detach(), grad_x=gx, grad_w=gw)
    if inp.add is not None:
        ref["y_add"] = y.detach() + inp.add.double()
    return ref


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def check(got, ref, what):
    """Every tensor of ``got`` within TOL x max |reference| of ``ref``'s; prints each figure before asserting."""
    for name, t in got.items():
        r = ref[name]
        assert tuple(t.shape) == tuple(r.shape), (what, name, tuple(t.shape), tuple(r.shape))
        scale = float(r.abs().max())
        err = float((t.detach().cpu().double() - r).abs().max())
        print("%s %s: err %.3g, max |ref| %.3g" % (what, name, err, scale))
        assert scale > 0, (what, name)
        assert err <= TOL * scale, (what, name, err, scale)
