"""Cases, input generators and the reference of the BatchNorm tests (tests/test_batchnorm_{cpu,gpu}.py).

Reference: ``act(F.batch_norm(x, ...) + residual)`` under autograd, float64, on the CPU -- what the reference project's layers
call (nn.BatchNorm2d, ``out += residual``, ReLU).  For the gated backward (the layer ended in a ReLU) the gate is taken from
the ``y`` that is handed to the device call, as tests/conv_backward_ref.py does: ``grad_out * (y > 0)`` is fed to the graph
without the ReLU.  (A gate recomputed in another precision flips wherever a pre-activation is within rounding of zero, and
one flipped gate moves a gradient by a large share of its maximum; that would test the inputs, not the kernels.)

Inputs are logical NCHW float32 tensors: x = mean + scale * N(0, 1), gamma = 1 + N(0, 1) / 2, beta, residual, grad_out
N(0, 1), running_mean N(0, 1), running_var uniform in [0.5, 1.5).
"""
import collections

import torch
import torch.nn.functional as F

Case = collections.namedtuple("Case", "B H W C")
# (1,1,2,4): n = 2, minimum C; (2,5,7,16), (3,9,11,64): small ragged grids; (2,3,5,20): five lanes per row, does not divide a
# wave; (2,13,13,136): 34 lanes per row; (1,7,9,512): two channel passes; (3,37,45,32): ragged, several slabs; (2,128,128,16):
# many slabs, DLA level 0's width; (1,14,14,256), (1,16,16,256), (1,16,18,256): 7, 8, 9 reduction slabs, around the eight
# lanes of the two-level slab sum (a lane without a slab, one each, one lane with two)
CASES = [Case(1, 1, 2, 4), Case(2, 5, 7, 16), Case(3, 9, 11, 64), Case(2, 3, 5, 20), Case(2, 13, 13, 136), Case(1, 7, 9, 512),
         Case(3, 37, 45, 32), Case(2, 128, 128, 16), Case(1, 14, 14, 256), Case(1, 16, 16, 256), Case(1, 16, 18, 256)]
LARGE_MEAN_CASES = [Case(2, 8, 8, 32), Case(4, 33, 31, 128)]
EPS, MOMENTUM = 1e-5, 0.1
TOL = 1e-4   # x max |reference| per output: the project's gradient tolerance


def case_id(c):
    return "B%d_%dx%d_C%d" % c


Inputs = collections.namedtuple("Inputs", "x gamma beta res go rmean rvar")


def inputs(seed, c, mean=0.0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    shape = (c.B, c.C, c.H, c.W)
    return Inputs(mean + scale * torch.randn(shape, generator=g), 1 + 0.5 * torch.randn(c.C, generator=g),
                  torch.randn(c.C, generator=g), torch.randn(shape, generator=g), torch.randn(shape, generator=g),
                  torch.randn(c.C, generator=g), 0.5 + torch.rand(c.C, generator=g))


def _pre(inp, residual, training, affine, x=None):
    """The graph without the activation, in float64; returns (pre-activation, leaves, running_mean, running_var)."""
    x = (inp.x if x is None else x).double().requires_grad_(True)
    w = inp.gamma.double().requires_grad_(True) if affine else None
    b = inp.beta.double().requires_grad_(True) if affine else None
    r = inp.res.double().requires_grad_(True) if residual else None
    rm, rv = inp.rmean.double().clone(), inp.rvar.double().clone()
    out = F.batch_norm(x, rm, rv, w, b, training, MOMENTUM, EPS)
    if residual:
        out = out + r
    return out, (x, w, b, r), rm, rv


def reference_forward(inp, residual, act, training=True, affine=True):
    """dict of y, save_mean, save_invstd, running_mean, running_var (float64, y logical NCHW)."""
    with torch.no_grad():
        out, _, rm, rv = _pre(inp, residual, training, affine)
        x = inp.x.double()
        mean = x.mean((0, 2, 3)) if training else inp.rmean.double()
        var = x.var((0, 2, 3), unbiased=False) if training else inp.rvar.double()
    return dict(y=torch.relu(out) if act else out, save_mean=mean, save_invstd=1 / torch.sqrt(var + EPS), running_mean=rm,
                running_var=rv)


def reference_backward(inp, residual, gate_y=None, training=True, affine=True):
    """dict of grad_x, grad_gamma, grad_beta, grad_residual (float64; None where there is no such input).  ``gate_y``: the
    activated output (logical NCHW) whose sign gates grad_out, or None for a layer without ReLU."""
    out, leaves, _, _ = _pre(inp, residual, training, affine)
    g = inp.go.double()
    if gate_y is not None:
        g = torch.where(gate_y <= 0, torch.zeros_like(g), g)   # torch's threshold_backward: a NaN y passes the gradient
    grads = torch.autograd.grad(out, [t for t in leaves if t is not None], g)
    it = iter(grads)
    return dict(zip(("grad_x", "grad_gamma", "grad_beta", "grad_residual"), [next(it) if t is not None else None for t in leaves]))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def device_forward(device, inp, residual, act, training=True, affine=True, running=True):
    """hip.batch_norm_forward on the case -> (dict like reference_forward's on the CPU, the device's y NHWC, mean, invstd)."""
    from centerpose_amd import hip

    rm = inp.rmean.to(device) if running else None
    rv = inp.rvar.to(device) if running else None
    y, mean, invstd = hip.batch_norm_forward(nhwc(inp.x).to(device), inp.gamma.to(device) if affine else None,
                                             inp.beta.to(device) if affine else None, nhwc(inp.res).to(device) if residual else None,
                                             rm, rv, training, MOMENTUM, EPS, act)
    got = dict(y=nchw(y).cpu(), save_mean=mean.cpu(), save_invstd=invstd.cpu())
    if running:
        got.update(running_mean=rm.cpu(), running_var=rv.cpu())
    return got, y, mean, invstd


def device_backward(device, inp, dev_fwd, residual, act, training=True, affine=True, **need):
    """hip.batch_norm_backward on the case with the forward's own y and statistics -> dict like reference_backward's."""
    from centerpose_amd import hip

    _, y, mean, invstd = dev_fwd
    gx, gr, gg, gb = hip.batch_norm_backward(nhwc(inp.x).to(device), nhwc(inp.go).to(device), mean, invstd,
                                             gamma=inp.gamma.to(device) if affine else None, y=y if act else None, training=training,
                                             need_residual_grad=residual, need_gamma_grad=affine, need_beta_grad=affine, **need)
    cpu = lambda t, f=lambda v: v: None if t is None else f(t).cpu()
    return dict(grad_x=cpu(gx, nchw), grad_gamma=cpu(gg), grad_beta=cpu(gb), grad_residual=cpu(gr, nchw))


def check(got, exp, what, tol=TOL):
    """Every output of ``exp`` within tol x max |reference|; prints each figure before it asserts."""
    for name, e in exp.items():
        if e is None:
            continue
        a = got[name]
        assert a is not None and a.shape == e.shape, (what, name)
        scale = float(e.abs().max())
        err = float((a.double() - e).abs().max())
        print("%s %s: max err %.3g, max |ref| %.3g (%.3g)" % (what, name, err, scale, err / scale if scale else 0.0))
        assert err <= tol * scale, "%s %s: max err %.3g vs max |ref| %.3g" % (what, name, err, scale)
