"""Reference and case list of the optimizer tests (tests/test_optim_cpu.py, tests/test_optim_gpu.py).

The reference is gradient-norm clipping + Adam written out in float64 from torch's documented formulas
(torch.nn.utils.clip_grad_norm_: coef = min(1, max_norm / (total_norm + 1e-6)); torch.optim.Adam, amsgrad=False,
maximize=False), fed the same float32-rounded parameters and gradients as the code under test.

The case: one optimizer over 1-D tensors of LENGTHS elements (around 4 = one 16-byte lane, 64 = one wavefront, 1024 = one
sweep of a 256-thread workgroup at 4 elements a lane, 4096 = one chunk of the table, and 12289 = three chunks and one
element), a 4-D [32, 16, 3, 3] weight, a channels_last 4-D parameter, a view that starts 4 bytes into its storage (no 16-byte
lanes), an empty tensor and a parameter that never gets a gradient.  STEPS steps; parameters ~ N(0, 0.1^2) and lr = 0.05, so
that an update is a visible fraction of its parameter (one variant runs at the reference's lr = 1.25e-4); gradient scales
log-spaced over 1e-4 .. 1e2 across the tensors.
"""
import functools
import math
import zlib
from collections import OrderedDict

import torch

LENGTHS = (1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 12289)
STEPS = 5
SEED = 23
UNALIGNED_LEN = 1030

# Error limit of the device results against the float64 reference, in the measures of ``errors``: ten times the worst error of
# torch's own float32 CPU path (clip_grad_norm_ + torch.optim.Adam) on these cases, every variant, tensor and measure.
# Measured: 2.68e-7 (variant weight_decay, exp_avg_sq of len12289; the other variants 1.9e-7 .. 2.1e-7, the norm 5.5e-8), the
# same with one thread and with all of them.  It is recorded to one significant digit, rounded up: the figure is a few float32
# roundings of an element-wise chain, and whether a CPU kernel contracts a product and a sum into one fma moves it by more
# than its third digit, so a limit read off the third digit would test the torch build and not this project.
# tests/test_optim_cpu.py::test_float32_error_is_far_below_the_gpu_limit prints what it measures and asserts that it stays
# <= 0.1 * TOL.
MEASURED_F32 = 3e-7
TOL = 10 * MEASURED_F32


def _gen(name):
    return torch.Generator().manual_seed(SEED * 1000003 + zlib.crc32(name.encode()))


class Case(object):
    """names, float32 CPU parameters (in their memory layouts), per-step float32 gradients (None: no gradient, ever)."""

    def __init__(self):
        shapes = OrderedDict(("len%d" % n, (n,)) for n in LENGTHS)
        shapes["weight4d"] = (32, 16, 3, 3)
        shapes["channels_last"] = (8, 6, 5, 3)
        shapes["unaligned"] = (UNALIGNED_LEN,)
        shapes["empty"] = (0,)
        shapes["no_grad"] = (7,)
        self.names = list(shapes)
        self.params, self.grads = OrderedDict(), [OrderedDict() for _ in range(STEPS)]
        with_grad = [k for k in self.names if k != "no_grad"]
        for k, shape in shapes.items():
            p = 0.1 * torch.randn(shape, generator=_gen("p" + k))
            self.params[k] = p.contiguous(memory_format=torch.channels_last) if k == "channels_last" else p
            for s in range(STEPS):
                if k == "no_grad":
                    self.grads[s][k] = None
                    continue
                scale = 10.0 ** (-4 + 6 * with_grad.index(k) / (len(with_grad) - 1))
                g = float(scale) * torch.randn(shape, generator=_gen("g%d%s" % (s, k)))
                self.grads[s][k] = g.contiguous(memory_format=torch.channels_last) if k == "channels_last" else g
        norms = [math.sqrt(sum(float(g.double().pow(2).sum()) for g in gs.values() if g is not None)) for gs in self.grads]
        self.min_norm, self.max_norm = min(norms), max(norms)

    def variants(self):
        """name -> hyper-parameters; ``max_grad_norm`` below every step's norm (active), 100 x above (inactive) or None."""
        active, inactive = 0.5 * self.min_norm, 100.0 * self.max_norm
        base = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=active)
        return OrderedDict([
            ("clip_active", dict(base)),
            ("clip_inactive", dict(base, max_grad_norm=inactive)),
            ("clip_off", dict(base, max_grad_norm=None)),
            ("weight_decay", dict(base, weight_decay=1e-2)),
            ("betas", dict(base, betas=(0.5, 0.9))),
            ("reference_lr", dict(base, lr=1.25e-4)),
        ])


@functools.lru_cache(maxsize=None)
def case():
    return Case()


VARIANTS = ("clip_active", "clip_inactive", "clip_off", "weight_decay", "betas", "reference_lr")


class Result(object):
    def __init__(self, p, m, v, step, norms):
        self.p, self.m, self.v, self.step, self.norms = p, m, v, step, norms


def adam_float64(params, grads_per_step, lr, betas, eps, weight_decay, max_grad_norm):
    """clip + Adam in float64.  params: name -> tensor; grads_per_step: list of name -> tensor or None.  Returns a Result of
    name -> float64 tensors (m, v: None where no step was taken), step counts and the total norm of every step."""
    b1, b2 = betas
    p = OrderedDict((k, t.double().clone()) for k, t in params.items())
    m, v, step = OrderedDict((k, None) for k in p), OrderedDict((k, None) for k in p), OrderedDict((k, 0) for k in p)
    norms = []
    for grads in grads_per_step:
        gs = OrderedDict((k, g.double()) for k, g in grads.items() if g is not None)
        norm = torch.sqrt(sum(g.pow(2).sum() for g in gs.values()))
        norms.append(float(norm))
        coef = 1.0
        if max_grad_norm:
            coef = min(1.0, max_grad_norm / (float(norm) + 1e-6))
        for k, g in gs.items():
            if m[k] is None:
                m[k], v[k] = torch.zeros_like(p[k]), torch.zeros_like(p[k])
            step[k] += 1
            g = coef * g + weight_decay * p[k]
            m[k] = m[k] + (1 - b1) * (g - m[k])
            v[k] = b2 * v[k] + (1 - b2) * g * g
            bc1, bc2 = 1 - b1 ** step[k], 1 - b2 ** step[k]
            p[k] = p[k] - (lr / bc1) * m[k] / (v[k].sqrt() / math.sqrt(bc2) + eps)
    return Result(p, m, v, step, norms)


@functools.lru_cache(maxsize=None)
def reference(variant, steps=STEPS):
    """The float64 Result of ``steps`` steps of the case under ``variant``; computed once, left unchanged by its users."""
    c = case()
    return adam_float64(c.params, c.grads[:steps], **c.variants()[variant])


def rel(got, ref):
    """max |got - ref| / max |ref| (0 for empty tensors and for a reference that is zero everywhere and met exactly)."""
    if ref.numel() == 0:
        return 0.0
    d, s = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
    return d / s if s > 0 else (0.0 if d == 0 else float("inf"))


def errors(ref, p, m, v, norms):
    """The error measures per tensor: name -> {p, m, v: max |delta| / max |reference|}, and the worst relative error of the
    norms.  p, m, v: name -> tensor (m, v: missing or None where the reference took no step: asserted)."""
    out = OrderedDict()
    for k in ref.p:
        e = {"p": rel(p[k], ref.p[k])}
        for name, got, want in (("m", m.get(k), ref.m[k]), ("v", v.get(k), ref.v[k])):
            if want is None:
                assert got is None, "%s: state of a parameter that never had a gradient" % k
            else:
                e[name] = rel(got, want)
        out[k] = e
    norm_err = max(abs(a - b) / b for a, b in zip(norms, ref.norms)) if norms else 0.0
    return out, norm_err


def worst(errs, norm_err):
    return max([norm_err] + [x for e in errs.values() for x in e.values()])


def torch_float32(variant, steps=STEPS, device="cpu", optimizer=None):
    """clip_grad_norm_ + torch.optim.Adam in float32 on ``device``: (params, optimizer, norms of every step)."""
    c = case()
    hp = dict(c.variants()[variant])
    max_norm = hp.pop("max_grad_norm")
    params = materialize(c, device)
    opt = (optimizer or torch.optim.Adam)(list(params.values()), **hp)
    norms = []
    for s in range(steps):
        set_grads(params, c.grads[s], device)
        with_grad = [p for p in params.values() if p.grad is not None]
        if max_norm:
            norms.append(float(torch.nn.utils.clip_grad_norm_(with_grad, max_norm)))
        else:
            norms.append(float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in with_grad))))
        opt.step()
    return params, opt, norms


def materialize(c, device, order=None):
    """The case's parameters as leaf tensors on ``device``, each in its memory layout: name -> Parameter, in ``order``."""
    out = OrderedDict()
    for k in (order or c.names):
        t = c.params[k]
        if k == "unaligned":
            base = torch.zeros(t.numel() + 1, dtype=torch.float32, device=device)
            base[1:].copy_(t)
            out[k] = torch.nn.Parameter(base[1:])
            assert out[k].data_ptr() % 16 == 4
        else:
            out[k] = torch.nn.Parameter(t.to(device).clone(memory_format=torch.preserve_format))
    return out


def set_grads(params, grads, device):
    for k, p in params.items():
        g = grads[k]
        p.grad = None if g is None else g.to(device).clone(memory_format=torch.preserve_format)


def state_of(opt, params):
    """(m, v, step) dicts by name from an optimizer's state (missing where the parameter has no state)."""
    m, v, step = {}, {}, {}
    for k, p in params.items():
        st = opt.state.get(p)
        if st:
            m[k], v[k], step[k] = st["exp_avg"], st["exp_avg_sq"], float(st["step"])
    return m, v, step
