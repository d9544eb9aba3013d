"""Cases, input generators and the reference of the GroupNorm tests (tests/test_groupnorm_{cpu,gpu}.py).

Reference: ``act(F.group_norm(x, G, gamma, beta, eps))`` under autograd, float64, on the CPU.  For the gated backward (the layer
ended in a ReLU) the gate is taken from the ``y`` that is handed to the device call, as tests/batchnorm_ref.py does:
``grad_out * (y > 0)`` is fed to the graph without the ReLU.

Inputs are logical NCHW float32 tensors: x = mean + scale * N(0, 1), gamma = 1 + N(0, 1) / 2, beta and grad_out N(0, 1).
"""
import collections

import torch
import torch.nn.functional as F

from tests.batchnorm_ref import TOL, check, nchw, nhwc  # noqa: F401  (the project's gradient tolerance and its check)

Case = collections.namedtuple("Case", "B H W C G")
# (1,1,2,4,1): minimum, n = 8, one float4; (2,5,7,16,16): C/G = 1; (2,5,7,64,32): C/G = 2, head_conv 64; (3,9,11,128,32): C/G = 4;
# (2,13,13,256,32): C/G = 8, a group over two lanes, head_conv 256; (1,7,9,512,32): two channel passes; (2,3,5,40,2): C/G = 20,
# five lanes per group, ten per row; (3,37,45,32,16): ragged, several slabs per image; (1,128,128,64,32): many slabs;
# (1,14,14,256,32), (1,16,16,256,32), (1,16,18,256,32): 7, 8 and 9 reduction slabs per image (C = 256: four rows per workgroup
# step, eight steps per slab: 196 / 256 / 288 rows), around the eight lanes of two_level_sum; (1,72,72,256,32): beyond the cap
# of 128 reduction slabs per image (1296 steps want 162 slabs of eight: 118 slabs of eleven steps instead)
CASES = [Case(1, 1, 2, 4, 1), Case(2, 5, 7, 16, 16), Case(2, 5, 7, 64, 32), Case(3, 9, 11, 128, 32), Case(2, 13, 13, 256, 32),
         Case(1, 7, 9, 512, 32), Case(2, 3, 5, 40, 2), Case(3, 37, 45, 32, 16), Case(1, 128, 128, 64, 32),
         Case(1, 14, 14, 256, 32), Case(1, 16, 16, 256, 32), Case(1, 16, 18, 256, 32), Case(1, 72, 72, 256, 32)]
LARGE_MEAN_CASES = [Case(2, 8, 8, 64, 32), Case(4, 33, 31, 256, 32)]
EPS = 1e-5


def case_id(c):
    return "B%d_%dx%d_C%d_G%d" % c


Inputs = collections.namedtuple("Inputs", "x gamma beta go")


def inputs(seed, c, mean=0.0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    shape = (c.B, c.C, c.H, c.W)
    return Inputs(mean + scale * torch.randn(shape, generator=g), 1 + 0.5 * torch.randn(c.C, generator=g),
                  torch.randn(c.C, generator=g), torch.randn(shape, generator=g))


def _pre(inp, c, affine):
    x = inp.x.double().requires_grad_(True)
    w = inp.gamma.double().requires_grad_(True) if affine else None
    b = inp.beta.double().requires_grad_(True) if affine else None
    return F.group_norm(x, c.G, w, b, EPS), (x, w, b)


def reference_forward(inp, c, act, affine=True):
    """dict of y (logical NCHW), save_mean, save_invstd [B,G], float64"""
    with torch.no_grad():
        out, _ = _pre(inp, c, affine)
        xg = inp.x.double().reshape(c.B, c.G, -1)
        mean, var = xg.mean(2), xg.var(2, unbiased=False)
    return dict(y=torch.relu(out) if act else out, save_mean=mean, save_invstd=1 / torch.sqrt(var + EPS))


def reference_backward(inp, c, gate_y=None, affine=True):
    """dict of grad_x, grad_gamma, grad_beta (float64; None where there is no such input)"""
    out, leaves = _pre(inp, c, affine)
    g = inp.go.double()
    if gate_y is not None:
        g = torch.where(gate_y <= 0, torch.zeros_like(g), g)   # torch's threshold_backward: a NaN y passes the gradient
    grads = torch.autograd.grad(out, [t for t in leaves if t is not None], g)
    it = iter(grads)
    return dict(zip(("grad_x", "grad_gamma", "grad_beta"), [next(it) if t is not None else None for t in leaves]))


def device_forward(device, inp, c, act, affine=True):
    """hip.group_norm_forward on the case -> (dict like reference_forward's on the CPU, the device's y NHWC, mean, invstd)"""
    from centerpose_amd import hip

    y, mean, invstd = hip.group_norm_forward(nhwc(inp.x).to(device), c.G, inp.gamma.to(device) if affine else None,
                                             inp.beta.to(device) if affine else None, EPS, act)
    return dict(y=nchw(y).cpu(), save_mean=mean.cpu(), save_invstd=invstd.cpu()), y, mean, invstd


def device_backward(device, inp, c, dev_fwd, act, affine=True, **need):
    from centerpose_amd import hip

    _, y, mean, invstd = dev_fwd
    gx, gg, gb = hip.group_norm_backward(nhwc(inp.x).to(device), nhwc(inp.go).to(device), c.G, mean, invstd,
                                         gamma=inp.gamma.to(device) if affine else None, y=y if act else None,
                                         need_gamma_grad=affine, need_beta_grad=affine, **need)
    cpu = lambda t, f=lambda v: v: None if t is None else f(t).cpu()
    return dict(grad_x=cpu(gx, nchw), grad_gamma=cpu(gg), grad_beta=cpu(gb))
