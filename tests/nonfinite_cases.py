"""Non-finite values through the training operators (test helper, not a test module): the poison, the comparison and the case
lists of tests/test_nonfinite_cpu.py and tests/test_nonfinite_gpu.py.

The contract ("Non-finite values"): one call of a training operator, one poisoned input element, against the float64
torch autograd of the same operation.

1. No laundering: every output element that is NaN or +-Inf in the reference is non-finite on the device.  Only finiteness is
   compared, not the class: Inf against NaN may differ with the summation order.
2. No collateral: every output element that is finite in the reference is within the bound of the operator's Gaussian-input GPU
   test, taken against max |reference| over the finite reference elements.

Rule 2 holds on every float32 path with any poison and on the f16x3 paths with a NaN.  An Inf operand of an f16x3 product makes
that operand's |max| infinite, so its power-of-two scale collapses and the finite elements of the call carry no information:
there rule 1 is asserted and the elements that miss rule 2 are counted and printed.  Neither rule looks at the elements a
poisoned weight or gradient element reaches only through zeros from beyond the other operand's range (``Case.reference``).

A case (``Case``) is one operator at one shape and mode: its float32 inputs, the torch graph in any float dtype, and the device
call.  The torch graphs are written here once, generic in the dtype, because the CPU test builds the non-finite mask from the
same graph in float32 and in float64; shapes, input generators and device wrappers come from the operators' own reference
modules.  ReLU is ``torch.relu`` and its gradient torch's threshold_backward (the gradient passes unless y <= 0, so it passes
where y is NaN).  On the device a gated backward gets the ``y`` the device forward made of the poisoned input, and the
reference takes its gate from that same ``y``, as the operators' own references do (a gate recomputed in another precision
flips where a pre-activation is within rounding of zero).
"""
import collections

import torch
import torch.nn.functional as F

from tests import batchnorm_ref as BN
from tests import conv_backward_ref as CB
from tests import conv_gru_ref as GRU
from tests import deconv_backward_ref as DC
from tests import groupnorm_ref as GN
from tests import dcn_backward_f16x3_cases as DF
from tests import pose_heads_ref as PH
from tests import pose_net_ref as PN

VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
WHERES = ("first", "last", "interior")
# the (kind, where) pairs every poisoned tensor goes through
POISONS = [("nan", "first"), ("nan", "last"), ("nan", "interior"), ("+inf", "interior"), ("-inf", "last")]


def poison(t, kind, where, allowed=None):
    """A copy of ``t`` with one element replaced by NaN, +Inf or -Inf: the first, the last or an interior element (row-major).
    ``allowed`` (a bool tensor of t's shape): the first allowed element at or after that one, wrapping round -- the grad_out of a
    gated case is poisoned where the layer's ReLU is open, elsewhere the gate drops the poison and the case tests nothing."""
    n = t.numel()
    assert n >= 3 and kind in VALUES and where in WHERES
    out = t.clone().contiguous()
    i = {"first": 0, "last": n - 1, "interior": (5 * n) // 11}[where]
    if allowed is not None:
        ok = allowed.contiguous().view(-1)
        assert ok.numel() == n and bool(ok.any())
        i = next(j % n for j in range(i, i + n) if bool(ok[j % n]))
    out.view(-1)[i] = VALUES[kind]
    return out


def nonfinite(t):
    return ~torch.isfinite(t)


Stats = collections.namedtuple("Stats", "ref_nonfinite got_nonfinite laundered missed worst")


def compare(got, ref64, tol, what, collateral=True, exempt=None):
    """Rules 1 and 2 on every output of ``ref64`` (dict name -> float64 tensor or None).  ``tol``: a number or a dict per output;
    0 means equal.  Prints, per output, the non-finite counts of the reference, of the result and of their symmetric difference,
    and the worst rule 2 error as a fraction of its bound; then asserts.  ``collateral=False``: rule 2 is counted and printed,
    not asserted (f16x3 with an Inf operand).  ``exempt``: dict name -> bool mask of elements neither rule looks at
    (``Case.reference``).  Returns dict name -> Stats."""
    stats, failures = {}, []
    for name, ref in ref64.items():
        if ref is None:
            continue
        a = got[name]
        assert a is not None and tuple(a.shape) == tuple(ref.shape), (what, name)
        a = a.detach().cpu().double()
        bad_r, bad_a = nonfinite(ref), nonfinite(a)
        skip = exempt[name] if exempt is not None and exempt.get(name) is not None else torch.zeros_like(bad_r)
        laundered = int((bad_r & ~bad_a & ~skip).sum())
        fin = ~bad_r & ~skip
        t = tol[name] if isinstance(tol, dict) else tol
        missed, worst = 0, 0.0
        if bool(fin.any()):
            r, v = ref[fin], a[fin]
            scale = float(r.abs().max())
            err = (v - r).abs()
            err = torch.where(torch.isfinite(v), err, torch.full_like(err, float("inf")))
            bound = t * scale
            missed = int((err > bound).sum())
            worst = float(err.max()) / bound if bound > 0 else (float("inf") if float(err.max()) > 0 else 0.0)
        stats[name] = Stats(int(bad_r.sum()), int(bad_a.sum()), laundered, missed, worst)
        print("%s %s: non-finite ref %d, got %d, differ %d (laundered %d); finite ref elements beyond the bound %d of %d, worst %.3g x bound"
              % (what, name, int(bad_r.sum()), int(bad_a.sum()), int((bad_r ^ bad_a).sum()), laundered, missed, int(fin.sum()), worst))
        if laundered:
            failures.append("%s %s: %d non-finite reference elements are finite in the result (rule 1)" % (what, name, laundered))
        if missed and collateral:
            failures.append("%s %s: %d finite reference elements miss the bound, worst %.3g x (rule 2)" % (what, name, missed, worst))
    assert not failures, "\n".join(failures)
    return stats


class _Relu(torch.autograd.Function):
    """torch.relu whose gradient gate (threshold_backward's) reads ``gate`` in place of its own output when one is given"""

    @staticmethod
    def forward(ctx, pre, gate):
        y = torch.relu(pre)
        ctx.save_for_backward(y if gate is None else gate.to(pre.dtype))
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return torch.where(y <= 0, torch.zeros_like(g), g), None


def relu(pre, gate=None):
    return _Relu.apply(pre, gate)


class Case:
    """name; inputs: OrderedDict name -> float32 CPU tensor (logical NCHW where the operator has a layout); targets: the inputs
    poisoned in turn; torch(inputs, dtype, gate) -> OrderedDict of outputs; device(device, inputs) -> (outputs on the CPU, gate or
    None); tol: the bound(s); f16x3: the call runs split-binary16 products (Inf poisons: rule 1 only).
    open_gate (gated cases): inputs -> the clean float64 activated output, of grad_out's shape; grad_out is poisoned where it is
    clearly positive.  live: dict target -> (inputs -> bool mask of the elements that reach an output at all), for weights whose
    outer taps the padding crops.  absorbs: the (target, kind) pairs whose poison the operation itself turns into finite
    numbers -- relu(-Inf) = 0, sigmoid(+-Inf), tanh(+-Inf) -- so that the whole reference is finite: rule 1 has nothing to
    test there, rule 2 still says that the device's result is finite and right.  tests/test_nonfinite_cpu.py checks that the
    list is exactly the pairs this happens for.  reach: dict target -> dict output -> the dimensions of that output other than
    the channel it shares with the target (see reference())."""

    def __init__(self, name, inputs, targets, torch_fn, device_fn, tol, f16x3=False, open_gate=None, live=None, absorbs=(), reach=None):
        self.reach = dict(reach or {})
        self.clean_gate = open_gate
        self.name, self.inputs, self.targets, self.torch, self.device, self.tol, self.f16x3 = name, inputs, targets, torch_fn, device_fn, tol, f16x3
        self.live = dict(live or {})
        if open_gate is not None:   # clearly open: no rounding of the device's forward closes it
            self.live["go"] = lambda inp: open_gate(inp) > 0.05
        self.absorbs = set(absorbs)
        self._masks = {}

    def poisoned(self, target, kind, where):
        inp = collections.OrderedDict(self.inputs)
        if target in self.live and target not in self._masks:
            self._masks[target] = self.live[target](self.inputs)
        inp[target] = poison(inp[target], kind, where, self._masks.get(target))
        return inp

    def reference(self, inp, target, gate=None):
        """(the float64 reference, the exempt masks: dict output -> bool tensor of the elements neither rule looks at).

        A convolution multiplies the poisoned element with values of the other operand and, at the border, with zeros from
        beyond that operand's range: the padding, the rows a transposed convolution has no grad_out for, a tile's ragged edge.
        Whether such a product exists is the implementation's business -- torch's own CPU kernels differ (the float64 ones
        multiply 0 x NaN where the float32 ones skip the tap, and which does what depends on the machine), and a device kernel
        may read zeros through its range check or branch round them.  So, for the outputs ``reach`` names: an element TRULY
        depends on the poison if the output changes with the poisoned element's value, everything else held fixed (the ReLU
        off or its gate fixed: the operations are linear in each operand then); the elements of the same channel slice that do
        not are the ones a zero-times-poison product can reach, and they are exempt.  Rule 1 is asserted on the true
        dependents, rule 2 on everything outside the slice."""
        r64 = self.torch(inp, torch.float64, gate)
        exempt = {}
        if target in self.reach:
            bad = nonfinite(inp[target])
            assert int(bad.sum()) == 1
            gate = gate if gate is not None or self.clean_gate is None else self.clean_gate(self.inputs)
            runs = []
            for v in (-1.0, 1.0):
                probe = collections.OrderedDict(inp)
                probe[target] = torch.where(bad, torch.full_like(inp[target], v), inp[target])
                runs.append(self.torch(probe, torch.float64, gate, linear=True))
            for name, dims in self.reach[target].items():
                true = runs[0][name] != runs[1][name]
                window = true
                for d in dims:
                    window = window.any(d, keepdim=True)
                exempt[name] = window.expand_as(true) & ~true
        return r64, exempt

    def __repr__(self):
        return self.name


def _cast(inp, dtype, leaves):
    t = {k: (None if v is None else v.to(dtype).clone()) for k, v in inp.items()}
    for k in leaves:
        t[k].requires_grad_(True)
    return t


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


# ---- BatchNorm ----
BN_GEOMETRIES = [BN.Case(1, 3, 5, 16), BN.Case(2, 3, 5, 20), BN.Case(1, 2, 3, 260)]   # 60 of 64 lanes; two channel passes
BN_TOL = BN.TOL


def _bn_torch(training, act, residual):
    def fn(inp, dtype, gate=None, linear=False):
        leaves = ["x", "gamma", "beta"] + (["res"] if residual else [])
        t = _cast(inp, dtype, leaves)
        # the affine step written out: F.batch_norm folds it into x * (invstd * gamma) + (beta - mean * invstd * gamma), which
        # for an infinite gamma is Inf - Inf = NaN in the whole channel, where (x - mean) * invstd * gamma is +-Inf by sign
        pre = F.batch_norm(t["x"], t["rmean"], t["rvar"], None, None, training, BN.MOMENTUM, BN.EPS)
        pre = pre * t["gamma"].view(1, -1, 1, 1) + t["beta"].view(1, -1, 1, 1)
        if residual:
            pre = pre + t["res"]
        y = relu(pre, gate) if act else pre
        g = torch.autograd.grad(y, [t[k] for k in leaves], t["go"])
        with torch.no_grad():
            x = t["x"].detach()
            mean = x.mean((0, 2, 3)) if training else inp["rmean"].to(dtype)
            var = x.var((0, 2, 3), unbiased=False) if training else inp["rvar"].to(dtype)
        out = collections.OrderedDict(y=y.detach(), save_mean=mean, save_invstd=1 / torch.sqrt(var + BN.EPS), running_mean=t["rmean"],
                                      running_var=t["rvar"], grad_x=g[0], grad_gamma=g[1], grad_beta=g[2])
        if residual:
            out["grad_residual"] = g[3]
        return out
    return fn


def _bn_device(training, act, residual):
    def fn(device, inp):
        i = BN.Inputs(*(inp[k] for k in BN.Inputs._fields))
        fwd = BN.device_forward(device, i, residual, act, training)
        out = collections.OrderedDict(fwd[0])
        bwd = BN.device_backward(device, i, fwd, residual, act, training)
        out.update((k, v) for k, v in bwd.items() if v is not None)
        return out, (out["y"] if act else None)
    return fn


def _y_of(torch_fn):
    return lambda inp: torch_fn(inp, torch.float64)["y"]


def bn_cases(geo):
    cases = []
    for training in (True, False):
        for act in (0, 1):
            for residual in (False, True):
                inp = collections.OrderedDict(BN.inputs(sum(geo) + 2 * act + residual, geo)._asdict())
                targets = ["x", "gamma", "go"] + (["res"] if residual else []) + ([] if training else ["rmean"])
                cases.append(Case("batchnorm %s %s act=%d res=%d" % (BN.case_id(geo), "train" if training else "eval", act, residual),
                                  inp, targets, _bn_torch(training, act, residual), _bn_device(training, act, residual), BN_TOL,
                                  open_gate=_y_of(_bn_torch(training, act, residual)) if act else None,
                                  absorbs=[("res", "-inf")] if act and residual else []))
    return cases


# ---- GroupNorm: the smallest cases with C / G = 1, 2 and 4 ----
GN_GEOMETRIES = [GN.CASES[1], GN.CASES[2], GN.CASES[3]]
GN_TOL = GN.TOL


def _gn_torch(c, act):
    def fn(inp, dtype, gate=None, linear=False):
        leaves = ["x", "gamma", "beta"]
        t = _cast(inp, dtype, leaves)
        pre = F.group_norm(t["x"], c.G, None, None, GN.EPS) * t["gamma"].view(1, -1, 1, 1) + t["beta"].view(1, -1, 1, 1)   # (as _bn_torch)
        y = relu(pre, gate) if act else pre
        g = torch.autograd.grad(y, [t[k] for k in leaves], t["go"])
        with torch.no_grad():
            xg = t["x"].detach().reshape(c.B, c.G, -1)
            mean, var = xg.mean(2), xg.var(2, unbiased=False)
        return collections.OrderedDict(y=y.detach(), save_mean=mean, save_invstd=1 / torch.sqrt(var + GN.EPS), grad_x=g[0],
                                       grad_gamma=g[1], grad_beta=g[2])
    return fn


def _gn_device(c, act):
    def fn(device, inp):
        i = GN.Inputs(*(inp[k] for k in GN.Inputs._fields))
        fwd = GN.device_forward(device, i, c, act)
        out = collections.OrderedDict(fwd[0])
        out.update(GN.device_backward(device, i, c, fwd, act))
        return out, (out["y"] if act else None)
    return fn


def gn_cases(c):
    return [Case("groupnorm %s act=%d" % (GN.case_id(c), act), collections.OrderedDict(GN.inputs(sum(c) + act, c)._asdict()),
                 ["x", "gamma", "go"], _gn_torch(c, act), _gn_device(c, act), GN_TOL, open_gate=_y_of(_gn_torch(c, act)) if act else None)
            for act in (0, 1)]


# ---- Conv2d forward (hip.conv2d_nhwc) ----
# one MFMA case (Cin % 32 == 0, 3x3), one generic case (Cin 8), one whose Cout is no multiple of the tile, the low-channel layer
# ... and whole 8 x 16 patches at 3x3 / stride 1, which the f16x3 launch runs on the halo-resident kernel (patch16_common.h's epilogue)
CONV_FWD_GEOMETRIES = [CB.Case(1, 32, 32, 6, 7, 3, 1, 1), CB.Case(1, 8, 16, 6, 7, 3, 2, 1), CB.Case(2, 32, 40, 5, 6, 1, 1, 0),
                       CB.Case(1, 16, 16, 64, 64, 3, 1, 1), CB.Case(1, 32, 32, 8, 16, 3, 1, 1)]
CONV_FWD_TOL = 2e-5   # tests/test_conv_geometry_gpu.py: FWD_TOL
GRAD_TOL = 1e-4       # tests/test_conv_backward_gpu.py, tests/test_conv_backward_f16x3_gpu.py, tests/test_stem_gpu.py


def _conv_inputs(seed, c, with_go):
    i = CB.gaussian_inputs(seed, c)
    inp = collections.OrderedDict(x=i.x, w=i.w, shift=i.bias)
    if with_go:
        inp["go"] = i.go
    return inp


def _conv_fwd_torch(c, act):
    def fn(inp, dtype, gate=None, linear=False):
        t = _cast(inp, dtype, [])
        y = F.conv2d(t["x"], t["w"], t["shift"], c.stride, c.pad)
        return collections.OrderedDict(out=torch.relu(y) if act and not linear else y)
    return fn


def _conv_fwd_device(c, act, precision):
    def fn(device, inp):
        from centerpose_amd import hip

        hip.set_default_precision(precision)
        y = hip.conv2d_nhwc(nhwc(inp["x"]).to(device), inp["w"].to(device), shift=inp["shift"].to(device), stride=c.stride, pad=c.pad,
                            act=act)
        return collections.OrderedDict(out=nchw(y).cpu()), None
    return fn


def conv_fwd_cases(c):
    return [Case("conv2d %s act=%d %s" % (CB.case_id(c), act, prec), _conv_inputs(40 + act, c, False), ["x", "w", "shift"],
                 _conv_fwd_torch(c, act), _conv_fwd_device(c, act, prec), CONV_FWD_TOL, f16x3=prec == "f16x3" and c.Cin % 32 == 0,
                 absorbs=[("shift", "-inf")] if act else [], reach={"w": {"out": (0, 2, 3)}})
            for act in (0, 1) for prec in ("f32", "f16x3")]


# ---- Conv2d backward (hip.ops.conv2d_backward_prec) ----
def conv_bwd_geometries():
    from tests import conv_backward_f16x3_cases as C16
    from tests import conv_lowc_cases as LC

    return [CB.CASES[1], CB.PADDED_CASES[0], CB.GENERIC_CASES[2], C16.KSTEP_CASES[0], LC.LOWC_CASES[4]]


def _conv_bwd_torch(c, gated):
    def fn(inp, dtype, gate=None, linear=False):
        leaves = ["x", "w", "shift"]
        t = _cast(inp, dtype, leaves)
        y = F.conv2d(t["x"], t["w"], t["shift"], c.stride, c.pad)
        if gated:
            y = relu(y, gate)
        g = torch.autograd.grad(y, [t[k] for k in leaves], t["go"])
        return collections.OrderedDict(grad_x=g[0], grad_w=g[1], grad_bias=g[2])
    return fn


def _conv_bwd_device(c, gated, precision):
    def fn(device, inp):
        from centerpose_amd import hip

        x, w, go = nhwc(inp["x"]).to(device), inp["w"].to(device), nhwc(inp["go"]).to(device)
        y = None
        if gated:   # the activated output the device's own forward makes of the (poisoned) inputs
            hip.set_default_precision("f32")
            y = hip.conv2d_nhwc(x, w, shift=inp["shift"].to(device), stride=c.stride, pad=c.pad, act=1)
        gx, gw, gb = hip.ops.conv2d_backward_prec(x, w, go, stride=c.stride, pad=c.pad, y=y, precision=precision)
        return collections.OrderedDict(grad_x=nchw(gx).cpu(), grad_w=gw.cpu(), grad_bias=gb.cpu()), (nchw(y).cpu() if gated else None)
    return fn


def _conv_y(c):
    return lambda inp: torch.relu(F.conv2d(inp["x"].double(), inp["w"].double(), inp["shift"].double(), c.stride, c.pad))


def conv_bwd_cases(c):
    return [Case("conv2d_backward %s gated=%d %s" % (CB.case_id(c), gated, prec), _conv_inputs(60 + gated, c, True), ["x", "w", "go"],
                 _conv_bwd_torch(c, gated), _conv_bwd_device(c, gated, prec), GRAD_TOL, f16x3=prec == "f16x3" and CB.is_mfma(c),
                 open_gate=_conv_y(c) if gated else None,
                 reach={"w": {"grad_x": (0, 2, 3)}, "go": {"grad_w": (1, 2, 3)}, "x": {"grad_w": (0, 2, 3)}})
            for gated in (0, 1) for prec in ("f32", "f16x3")]


# ---- stem backward (hip.conv2d_stem_backward): Cin 3, Cout 16, 9 x 11, gated ----
STEM_GEOMETRIES = [CB.Case(1, 3, 16, 9, 11, 7, 1, 3), CB.Case(1, 3, 16, 9, 11, 7, 2, 3)]


def _stem_torch(c):
    def fn(inp, dtype, gate=None, linear=False):
        leaves = ["w", "shift"]
        t = _cast(inp, dtype, leaves)
        y = relu(F.conv2d(t["x"], t["w"], t["shift"], c.stride, c.pad), gate)
        g = torch.autograd.grad(y, [t[k] for k in leaves], t["go"])
        return collections.OrderedDict(grad_w=g[0], grad_bias=g[1])
    return fn


def _stem_device(c):
    def fn(device, inp):
        from centerpose_amd import hip

        hip.set_default_precision("f32")
        x = inp["x"].to(device)
        x4 = F.pad(nhwc(x), (0, 1))   # the forward takes channel quads: a zero plane with zero weights (centerpose_amd/stem.py)
        w4 = F.pad(inp["w"].to(device), (0, 0, 0, 0, 0, 1))
        y = hip.conv2d_nhwc(x4, w4, shift=inp["shift"].to(device), stride=c.stride, pad=c.pad, act=1)
        gw, gb = hip.conv2d_stem_backward(x, nhwc(inp["go"]).to(device), stride=c.stride, y=y)
        return collections.OrderedDict(grad_w=gw.cpu(), grad_bias=gb.cpu()), nchw(y).cpu()
    return fn


def stem_cases(c):
    return [Case("stem_backward %s" % CB.case_id(c), _conv_inputs(80, c, True), ["x", "go"], _stem_torch(c), _stem_device(c), GRAD_TOL,
                 open_gate=_conv_y(c), reach={"go": {"grad_w": (1, 2, 3)}, "x": {"grad_w": (0, 2, 3)}})]


# ---- ConvGRU gates (hip.gru_gate_*): M = 5, Ch = 4 ----
def _gru_torch(inp, dtype, gate=None, linear=False):
    r = GRU.gate_reference(GRU.GateInputs(*(inp[k] for k in GRU.GateInputs._fields)), False, dtype)
    return collections.OrderedDict((k, v.detach()) for k, v in r.items())


def _gru_device(device, inp):
    from centerpose_amd import hip

    x3, h3, hp, go = (inp[k].to(device) for k in GRU.GateInputs._fields)
    out = hip.gru_gate_forward(x3, h3, hp)
    g = hip.gru_gate_backward(x3, h3, hp, go)
    return collections.OrderedDict(hout=out.cpu(), grad_x3=g[0].cpu(), grad_h3=g[1].cpu(), grad_hprev=g[2].cpu()), None


def gru_cases():
    inp = collections.OrderedDict(GRU.gate_inputs(5, 5, 4)._asdict())
    # POISONS' Infs land on saturating inputs: x3 +inf@interior and h3 +inf@interior on r (sigmoid -> 1, derivative 0), x3 -inf@last
    # on n (tanh -> -1, derivative 0); h3 -inf@last is n's hidden term, which r multiplies: (-inf) stays
    return [Case("gru_gate M=5 Ch=4", inp, ["x3", "h3", "hprev", "go"], _gru_torch, _gru_device, GRU.TOL,
                 absorbs=[("x3", "+inf"), ("x3", "-inf"), ("h3", "+inf")])]


# ---- hourglass merge (hip.upsample2_add_*): 1 x 3 x 5 x 4, small integers so that every sum is exact in any order ----
def _merge_torch(inp, dtype, gate=None, linear=False):
    t = _cast(inp, dtype, ["up1", "low"])
    out = t["up1"] + F.interpolate(t["low"], scale_factor=2, mode="nearest")
    g = torch.autograd.grad(out, [t["up1"], t["low"]], t["go"])
    return collections.OrderedDict(out=out.detach(), grad_low=g[1])


def _merge_device(device, inp):
    from centerpose_amd import hip

    out = hip.ops.upsample2_add_forward(nhwc(inp["up1"]).to(device), nhwc(inp["low"]).to(device))
    gl = hip.ops.upsample2_add_backward(nhwc(inp["go"]).to(device), tuple(nhwc(inp["low"]).shape))
    return collections.OrderedDict(out=nchw(out).cpu(), grad_low=nchw(gl).cpu()), None


def merge_cases():
    g = torch.Generator().manual_seed(9)
    ints = lambda *s: torch.randint(-8, 9, s, generator=g).float()
    inp = collections.OrderedDict(up1=ints(1, 4, 6, 10), low=ints(1, 4, 3, 5), go=ints(1, 4, 6, 10))
    return [Case("upsample2_add 1x3x5x4", inp, ["up1", "low", "go"], _merge_torch, _merge_device, 0.0)]


# ---- ConvTranspose2d: IDAUp's depth-wise up (f = 2, f = 4) and the dense k 4 / stride 2 layer ----
DECONV_GEOMETRIES = [DC.DW_CASES[0], DC.DW_CASES[2], DC.DENSE_CASES[0]]
DECONV_TOL = DC.TOL


def _deconv_torch(c):
    def fn(inp, dtype, gate=None, linear=False):
        t = _cast(inp, dtype, ["x", "w"])
        y = F.conv_transpose2d(t["x"], t["w"], None, c.stride, c.pad, groups=c.groups)
        g = torch.autograd.grad(y, [t["x"], t["w"]], t["go"])
        out = collections.OrderedDict(y=y.detach() if c.groups == 1 else y.detach() + t["add"], grad_x=g[0], grad_w=g[1])
        if c.groups == 1:   # the dense layer's fused ReLU (resdcn's deconv + BatchNorm + ReLU in evaluation form)
            out["y_relu"] = y.detach() if linear else torch.relu(y.detach())
        return out
    return fn


def _deconv_device(c, precision):
    def fn(device, inp):
        from centerpose_amd import hip

        hip.set_default_precision(precision)
        x, w, go = nhwc(inp["x"]).to(device), inp["w"].to(device), nhwc(inp["go"]).to(device)
        if c.groups == 1:
            y = hip.conv_transpose2d(x, w)
        else:
            y = hip.conv_transpose2d_dw(x, w, c.stride, add=nhwc(inp["add"]).to(device))
        gx, gw = hip.ops.conv_transpose2d_backward(x, w, go, c.stride, c.pad, c.groups, precision=precision)
        out = collections.OrderedDict(y=nchw(y).cpu(), grad_x=nchw(gx).cpu(), grad_w=gw.cpu())
        if c.groups == 1:
            out["y_relu"] = nchw(hip.conv_transpose2d(x, w, act=1)).cpu()
        return out, None
    return fn


def deconv_cases(c):
    i = DC.inputs(3, c)
    inp = collections.OrderedDict((k, v) for k, v in i._asdict().items() if v is not None)
    targets = ["x", "w", "go"] + (["add"] if c.groups != 1 else [])

    # w is [Cin, Cout / groups, K, K]: dense, its two channels are those of x and of y; depth-wise, dimension 0 is the one channel
    go_w = (0, 2, 3) if c.groups == 1 else (1, 2, 3)
    reach = {"w": {"y": (0, 2, 3), "grad_x": (0, 2, 3)}, "go": {"grad_w": go_w}, "x": {"grad_w": (1, 2, 3)}}
    if c.groups == 1:
        reach["w"]["y_relu"] = (0, 2, 3)

    def live_taps(inp):   # the taps some output pixel uses (on a 1 x 1 input the padding crops the outer ring of the kernel)
        w = inp["w"].double().requires_grad_(True)
        y = F.conv_transpose2d(torch.ones_like(inp["x"], dtype=torch.float64), w, None, c.stride, c.pad, groups=c.groups)
        return torch.autograd.grad(y.sum(), w)[0] != 0

    return [Case("conv_transpose2d %s %s" % (DC.case_id(c), prec), inp, targets, _deconv_torch(c), _deconv_device(c, prec), DECONV_TOL,
                 f16x3=prec == "f16x3" and c.groups == 1, live={"w": live_taps}, reach=reach) for prec in (("f32", "f16x3") if c.groups == 1 else ("f32",))]


# ---- PoseHeads forward and backward (hip.pose_heads_*): ``ragged_13x19``, two heads, on the strict inputs of
# tests/pose_heads_ref.py -- every hidden value is an odd multiple of 1/32, exact in float32 and in f16x3, so no ReLU gate can
# differ between the device's recomputed hidden layer and the float64 reference ----
HEADS_SHAPE = PH.DYADIC_SHAPES["ragged_13x19"]
HEADS_FWD_TOL, HEADS_GRAD_TOL = 2e-5, 1e-4   # tests/test_pose_heads_gpu.py: FWD_TOL, GRAD_TOL
_HEAD_KEYS = ("w0", "b0", "w1", "b1")


def _heads_torch(n):
    def fn(inp, dtype, gate=None, linear=False):
        leaves = ["feat"] + ["%s_%d" % (k, i) for i in range(n) for k in _HEAD_KEYS]
        t = _cast(inp, dtype, leaves)
        outs = []
        for i in range(n):
            h = F.conv2d(t["feat"], t["w0_%d" % i], t["b0_%d" % i], padding=1)
            outs.append(F.conv2d(h if linear else relu(h), t["w1_%d" % i], t["b1_%d" % i]))
        g = torch.autograd.grad(outs, [t[k] for k in leaves], [t["go_%d" % i] for i in range(n)])
        res = collections.OrderedDict(("out_%d" % i, o.detach()) for i, o in enumerate(outs))
        res["grad_feat"] = g[0]
        res.update(("grad_" + k, v) for k, v in zip(leaves[1:], g[1:]))
        return res
    return fn


def _heads_device(n, precision):
    def fn(device, inp):
        from centerpose_amd import hip

        hip.set_default_precision(precision)
        feat = inp["feat"].to(device)
        params = [tuple(inp["%s_%d" % (k, i)].to(device) for k in _HEAD_KEYS) for i in range(n)]
        outs = hip.pose_heads_forward(feat, params)
        gfeat, grads = hip.ops.pose_heads_backward_prec(feat, params, [inp["go_%d" % i].to(device) for i in range(n)], precision=precision)
        res = collections.OrderedDict(("out_%d" % i, o.cpu()) for i, o in enumerate(outs))
        res["grad_feat"] = gfeat.cpu()
        for i in range(n):
            res.update(("grad_%s_%d" % (k, i), v.cpu()) for k, v in zip(_HEAD_KEYS, grads[i]))
        return res, None
    return fn


def heads_cases():
    case = PH.dyadic_case(31, *HEADS_SHAPE)
    n = len(case.params)
    inp = collections.OrderedDict(feat=case.feat)
    for i in range(n):
        inp.update(("%s_%d" % (k, i), v) for k, v in zip(_HEAD_KEYS, case.params[i]))
        inp["go_%d" % i] = case.grad_outs[i]
    tol = {k: HEADS_FWD_TOL for k in ("out_0", "out_1")}
    tol.update(("grad_" + k, HEADS_GRAD_TOL) for k in list(inp)[1:] + ["feat"] if not k.startswith("go_"))

    def centre_tap(inp):   # the one tap of the 3x3 weight that meets no padding at any pixel: its hidden channel is poisoned everywhere
        m = torch.zeros_like(inp["w0_0"], dtype=torch.bool)
        m[:, :, 1, 1] = True
        return m

    # feat, one hidden weight, one output bias, one grad_out.  grad_out reaches the whole 3x3 weight gradient of its head (through
    # every open hidden unit), the feature map the input-channel slice of both
    reach = {"feat": {"grad_w0_0": (0, 2, 3), "grad_w0_1": (0, 2, 3)}, "go_1": {"grad_w0_1": (0, 1, 2, 3)}}
    return [Case("pose_heads ragged_13x19 %s" % prec, inp, ["feat", "w0_0", "b1_1", "go_1"], _heads_torch(n), _heads_device(n, prec), tol,
                 f16x3=prec == "f16x3", live={"w0_0": centre_tap}, reach=reach) for prec in ("f32", "f16x3")]


# ---- DCNv2 forward and backward (hip.dcn_v2_forward, hip.ops.dcn_v2_backward): the smallest shape of
# tests/dcn_backward_f16x3_cases.py, float32 (atomic and deterministic input gradient) and f16x3.  The graph is
# tests/pose_net_ref.py's differentiable restatement, which runs in any float dtype.  x, mask and grad_out are poisoned at
# pixels two or more away from the border: the restatement clamps the indices of corners outside the image and multiplies them by
# a zero weight, so a poisoned border pixel would reach samples that never read it, and a poisoned mask or grad_out at a border
# pixel would meet samples outside the image, which the kernels skip.  Offsets are not poisoned here (test_nonfinite_gpu.py has
# the offset rule of each forward).
# SHAPES[0] (C = Co = 16): the backward's fast geometry; its forward is the generic kernel (the fast forward wants more than 32
# output channels, the f16x3 one C % 32 == 0).  SHAPES[2] (64 -> 64 on 13 x 19): the fast forward in float32 and in f16x3.
DCN_SHAPES = [DF.SHAPES[0], DF.SHAPES[2]]
DCN_FWD_TOL, DCN_GRAD_TOL = 2e-5, DF.TOL   # tests/test_gpu_parity.py's forward bound; tests/test_dcn_backward_gpu.py's 1e-4
_DCN_GRADS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")


def _dcn_torch(inp, dtype, gate=None, linear=False):
    leaves = ["x", "off", "mask", "w", "b"]
    t = _cast(inp, dtype, leaves)
    out = PN.dcn_v2(t["x"], t["w"], t["b"], t["off"], t["mask"])
    g = torch.autograd.grad(out, [t[k] for k in leaves], t["go"])
    res = collections.OrderedDict(out=out.detach())
    res.update(zip(_DCN_GRADS, g))
    return res


def _dcn_device(precision, det):
    def fn(device, inp):
        from centerpose_amd import hip

        hip.set_default_precision(precision)
        x, w, b, off, mask, go = (inp[k].to(device) for k in ("x", "w", "b", "off", "mask", "go"))
        out = hip.dcn_v2_forward(x, w, b, off, mask, *DF.CP)
        grads = hip.ops.dcn_v2_backward(x, w, b, off, mask, go, *DF.CP, deterministic=det, precision=precision)
        res = collections.OrderedDict(out=out.cpu())
        res.update((k, v.cpu()) for k, v in zip(_DCN_GRADS, grads))
        return res, None
    return fn


def dcn_cases(shape):
    x, w, b, off, mask, go = DF.gaussian_case(shape, 0.5)
    inp = collections.OrderedDict(x=x, w=w, b=b, off=off, mask=mask, go=go)

    def interior(name):
        def fn(inp):
            m = torch.zeros_like(inp[name], dtype=torch.bool)
            m[:, :, 2:-2, 2:-2] = True
            return m
        return fn

    tol = dict(out=DCN_FWD_TOL, **{k: DCN_GRAD_TOL for k in _DCN_GRADS})
    reach = {"w": {"out": (0, 2, 3), "grad_input": (0, 2, 3), "grad_offset": (0, 2, 3), "grad_mask": (0, 2, 3)},
             "go": {"grad_weight": (1, 2, 3)}}
    return [Case("dcn_v2 %s %s%s" % (DF.shape_id(shape), prec, " deterministic" if det else ""), inp, ["x", "w", "go", "mask"],
                 _dcn_torch, _dcn_device(prec, det), tol, f16x3=prec == "f16x3",
                 live={k: interior(k) for k in ("x", "mask", "go")}, reach=reach)
            for prec, det in (("f32", False), ("f32", True), ("f16x3", False))]


def groups():
    """The case lists by test id: OrderedDict id -> function that returns the Cases (built on demand: the inputs are random draws)."""
    out = collections.OrderedDict()
    for geo in BN_GEOMETRIES:
        out["batchnorm_" + BN.case_id(geo)] = lambda geo=geo: bn_cases(geo)
    for c in GN_GEOMETRIES:
        out["groupnorm_" + GN.case_id(c)] = lambda c=c: gn_cases(c)
    for c in CONV_FWD_GEOMETRIES:
        out["conv2d_" + CB.case_id(c)] = lambda c=c: conv_fwd_cases(c)
    for c in conv_bwd_geometries():
        out["conv2d_backward_" + CB.case_id(c)] = lambda c=c: conv_bwd_cases(c)
    for c in STEM_GEOMETRIES:
        out["stem_backward_" + CB.case_id(c)] = lambda c=c: stem_cases(c)
    out["pose_heads"] = heads_cases
    for shape in DCN_SHAPES:
        out["dcn_v2_" + DF.shape_id(shape)] = lambda shape=shape: dcn_cases(shape)
    out["gru_gate"] = gru_cases
    out["upsample2_add"] = merge_cases
    for c in DECONV_GEOMETRIES:
        out["conv_transpose2d_" + DC.case_id(c)] = lambda c=c: deconv_cases(c)
    return out


# ---- MaxPool: explicit positions (first tap, last tap, a middle tap of a window; a tap shared by four windows; image corners,
# which at (3, 2, 1) sit beside the padding) ----
POOL_SHAPE = (1, 4, 5, 7)   # B, C, H, W
POOL_POSITIONS = {(2, 2, 0): [(2, 2), (3, 3), (2, 3), (0, 0), (3, 5), (4, 6)],       # (4, 6): the row and column flooring drops
                  (3, 2, 1): [(1, 1), (2, 2), (3, 3), (1, 3), (0, 0), (4, 6), (0, 3)]}   # (1, 1), (1, 3), (3, 3): in four windows


def pool_inputs():
    g = torch.Generator().manual_seed(21)
    x = torch.relu(torch.randn(POOL_SHAPE, generator=g))   # ties, as in the network
    return x, g


def pool_reference(x, go, geo, dtype=torch.float64):
    xr = x.to(dtype).requires_grad_(True)
    y = F.max_pool2d(xr, *geo)
    gx, = torch.autograd.grad(y, xr, go.to(dtype))
    return collections.OrderedDict(y=y.detach(), grad_x=gx)


def pool_out_size(geo):
    k, s, p = geo
    return (POOL_SHAPE[2] + 2 * p - k) // s + 1, (POOL_SHAPE[3] + 2 * p - k) // s + 1
