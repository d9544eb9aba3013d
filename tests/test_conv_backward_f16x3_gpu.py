"""The f16x3 mode of the Conv2d backward on the device (pytest -m gpu): cp_conv2d_backward_prec_nhwc with CP_PREC_F16X3, and
conv.Conv2d / use_hip_convs / set_backward_precision with backward_precision = "f16x3", against torch.nn.functional.conv2d under
float64 CPU autograd.  Inputs, their premises and the tolerance: tests/conv_backward_f16x3_cases.py.  Every test first asserts,
through cp_conv2d_backward_prec_mask, that both contractions of its case run in f16x3."""
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from centerpose_amd import conv, hip
from tests import conv_backward_f16x3_cases as C
from tests import conv_backward_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", C.CASES, ids=R.case_id)
def test_dyadic_inputs_are_exact(device, c):
    C.assert_f16x3(c)
    inp = C.cached_inputs("dyadic", sum(c), c)
    for gated in (False, True):
        got = C.device_backward(device, c, inp, gated)
        C.assert_equal(got, C.cached_reference("dyadic", sum(c), c, gated), "%s gated=%d" % (R.case_id(c), gated))


@pytest.mark.parametrize("which", ["xw", "go"])
@pytest.mark.parametrize("c", C.TWO_LEVEL_CASES, ids=R.case_id)
def test_two_level_dyadic_inputs_are_exact(device, c, which):
    """Exact only if every cross term (hi*lo and lo*hi) of every product is there."""
    C.assert_f16x3(c)
    kind, seed = "two_" + which, sum(c) + 3
    inp = C.cached_inputs(kind, seed, c)
    for gated in (False, True):
        got = C.device_backward(device, c, inp, gated)
        C.assert_equal(got, C.cached_reference(kind, seed, c, gated), "%s %s gated=%d" % (R.case_id(c), which, gated))


@pytest.mark.parametrize("c", C.CASES, ids=R.case_id)
def test_gaussian_inputs(device, c):
    C.assert_f16x3(c)
    inp = C.cached_inputs("gauss", sum(c) + 1, c)
    for gated in (False, True):
        exp = C.cached_reference("gauss", sum(c) + 1, c, gated)
        f32 = C.device_backward(device, c, inp, gated, precision="f32")
        got = C.device_backward(device, c, inp, gated)
        for (n, e16, s), (_, e32, _) in zip(C.errors(got, exp), C.errors(f32, exp)):
            print("%s gated=%d %s: f16x3 err %.3g, f32 err %.3g, max |ref| %.3g" % (R.case_id(c), gated, n, e16, e32, s))
        C.assert_close(got, exp, 1e-4, "%s gated=%d" % (R.case_id(c), gated))


@pytest.mark.parametrize("c", [R.Case(2, 32, 64, 37, 45, 3, 2, 1), R.Case(2, 64, 27, 40, 40, 3, 1, 1)], ids=R.case_id)
def test_the_other_kernels_ran(device, c):
    """On Gaussian inputs the f16x3 grad_w and grad_x are not the float32 mode's bits; grad_bias, float32 in both, is."""
    C.assert_f16x3(c)
    inp = C.cached_inputs("gauss", sum(c) + 1, c)
    a = C.device_backward(device, c, inp, True)
    b = C.device_backward(device, c, inp, True, precision="f32")
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    assert torch.equal(a[2], b[2])


RANGE_CASES = [R.CASES[2], C.KSTEP_CASES[2]]   # 3x3 stride 2 (the float32 test's case) and 3x3 stride 1


@pytest.mark.parametrize("scale", [1e-6, 1e3])
@pytest.mark.parametrize("c", RANGE_CASES, ids=R.case_id)
def test_input_range(device, c, scale):
    C.assert_f16x3(c)
    inp = C.cached_inputs("gauss", 11, c)
    inp = inp._replace(x=inp.x * scale, w=inp.w * scale, go=inp.go * scale)
    got = C.device_backward(device, c, inp, True)
    C.assert_close(got, R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, inp.y), 1e-4, "%s scale %g" % (R.case_id(c), scale))


@pytest.mark.parametrize("abc", [(-20, 7, 3), (12, -30, -5)])
@pytest.mark.parametrize("c", RANGE_CASES + [C.KSTEP_CASES[8]], ids=R.case_id)
def test_power_of_two_equivariance(device, c, abc):
    """x * 2^a, grad_out * 2^b, w * 2^c: grad_w * 2^(a+b), grad_x * 2^(b+c), grad_bias * 2^b, bit for bit."""
    C.assert_f16x3(c)
    a, b, cc = abc
    inp = C.cached_inputs("gauss", 12, c)
    base = C.device_backward(device, c, inp, True)
    scaled = inp._replace(x=inp.x * 2.0 ** a, go=inp.go * 2.0 ** b, w=inp.w * 2.0 ** cc)
    got = C.device_backward(device, c, scaled, True)
    exp = (base[0] * 2.0 ** (b + cc), base[1] * 2.0 ** (a + b), base[2] * 2.0 ** b)
    for t in exp:
        assert bool(torch.isfinite(t).all()) and float(t.abs()[t != 0].min()) > 2.0 ** -120   # no over- or underflow in the claim
    C.assert_equal(got, exp, "%s (a, b, c) = %s" % (R.case_id(c), abc))


@pytest.mark.parametrize("c", [R.Case(2, 64, 64, 40, 40, 3, 1, 1), R.CASES[1], R.CASES[7]], ids=R.case_id)
def test_two_calls_are_bit_identical(device, c):
    C.assert_f16x3(c)
    inp = C.cached_inputs("gauss", 5, c)
    a = C.device_backward(device, c, inp, True)
    b = C.device_backward(device, c, inp, True)
    for name, p, q in zip(C.NAMES, a, b):
        assert torch.equal(p, q), name


def _raw_call(device, c, inp, nbytes, precision, gx=None, gb=None):
    L = hip.lib()
    x, w, go, y = (t.to(device) for t in (R.nhwc(inp.x), inp.w, R.nhwc(inp.go), R.nhwc(inp.y)))
    gw = torch.full_like(w, 7.25)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = L.cp_conv2d_backward_prec_nhwc(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(x), p(w), p(y), p(go), p(gx), p(gw),
                                        p(gb), *C.geo(c), precision, p(ws), nbytes)
    torch.cuda.synchronize()
    return rc, gw


@pytest.mark.parametrize("c", [R.CASES[1], R.PADDED_CASES[0]], ids=R.case_id)
def test_null_outputs_are_not_touched(device, c):
    C.assert_f16x3(c)
    inp = C.cached_inputs("gauss", 6, c)
    full = C.device_backward(device, c, inp, True)
    L = hip.lib()
    canary_x = torch.full((c.B, c.H, c.W, c.Cin), 7.25, device=device)
    canary_b = torch.full((c.Cout,), 7.25, device=device)
    nbytes = L.cp_conv2d_backward_prec_workspace_bytes(*C.geo(c), 0, 1)
    rc, gw = _raw_call(device, c, inp, nbytes, 1)
    assert rc == 0, L.cp_last_error()
    assert bool((canary_x == 7.25).all()) and bool((canary_b == 7.25).all())
    assert torch.equal(gw.cpu(), full[1])
    for need_x, need_b in ((False, True), (True, False), (False, False)):
        gx, gw2, gb = C.device_backward(device, c, inp, True, need_x_grad=need_x, need_bias_grad=need_b)
        assert (gx is None) == (not need_x) and (gb is None) == (not need_b)
        assert torch.equal(gw2, full[1])
        assert gx is None or torch.equal(gx, full[0])
        assert gb is None or torch.equal(gb, full[2])


@pytest.mark.parametrize("c", [R.CASES[1], R.PADDED_CASES[0]], ids=R.case_id)
def test_short_workspace_is_refused_before_any_launch(device, c):
    C.assert_f16x3(c)
    inp = C.cached_inputs("gauss", 6, c)
    L = hip.lib()
    need = L.cp_conv2d_backward_prec_workspace_bytes(*C.geo(c), 1, 1)
    assert need > L.cp_conv2d_backward_workspace_bytes(*C.geo(c), 1) > 0
    gx = torch.full((c.B, c.H, c.W, c.Cin), 7.25, device=device)
    gb = torch.full((c.Cout,), 7.25, device=device)
    rc, gw = _raw_call(device, c, inp, need - 1, 1, gx=gx, gb=gb)
    assert rc == -1 and b"workspace too small" in L.cp_last_error()
    assert bool((gx == 7.25).all()) and bool((gb == 7.25).all()) and bool((gw == 7.25).all())
    rc, _ = _raw_call(device, c, inp, need, 7, gx=gx, gb=gb)
    assert rc == -1 and b"unknown precision" in L.cp_last_error() and bool((gx == 7.25).all())


@pytest.mark.parametrize("c", [R.CASES[1], R.CASES[5], R.PADDED_CASES[0], R.GENERIC_CASES[2]], ids=R.case_id)
def test_f32_through_the_new_entry_is_the_old_entry(device, c):
    inp = C.cached_inputs("gauss", 8, c)
    L = hip.lib()
    old = R.device_backward(device, c, inp, True)
    for need_x in (0, 1):
        assert L.cp_conv2d_backward_prec_workspace_bytes(*C.geo(c), need_x, 0) == L.cp_conv2d_backward_workspace_bytes(*C.geo(c), need_x)
    gx = torch.empty((c.B, c.H, c.W, c.Cin), device=device)
    gb = torch.empty((c.Cout,), device=device)
    rc, gw = _raw_call(device, c, inp, L.cp_conv2d_backward_prec_workspace_bytes(*C.geo(c), 1, 0), 0, gx=gx, gb=gb)
    assert rc == 0, L.cp_last_error()
    assert torch.equal(gx.permute(0, 3, 1, 2).cpu(), old[0]) and torch.equal(gw.cpu(), old[1]) and torch.equal(gb.cpu(), old[2])


def _make(kind, c, has_bias, device):
    """A conv.Conv2d in f16x3 backward mode, built in one of the three ways."""
    if kind == "direct":
        mod = conv.Conv2d(c.Cin, c.Cout, c.k, c.stride, c.pad, bias=has_bias).to(device)
        mod.backward_precision = "f16x3"
    else:
        mod = nn.Conv2d(c.Cin, c.Cout, c.k, c.stride, c.pad, bias=has_bias).to(device)
        if kind == "use_hip_convs":
            assert conv.use_hip_convs(mod, backward_precision="f16x3") == ([""], {})
        else:
            assert conv.use_hip_convs(mod) == ([""], {}) and mod.backward_precision == "f32"
            assert conv.set_backward_precision(mod, "f16x3") == 1
    assert type(mod) is conv.Conv2d and mod.backward_precision == "f16x3" and conv.Conv2d.backward_precision == "f32"
    return mod


@pytest.mark.parametrize("c", C.MODULE_CASES, ids=R.case_id)
def test_layer_backward_is_exact(device, c):
    C.assert_f16x3(c)
    hip.set_default_precision("f32")
    inp = C.cached_inputs("dyadic", sum(c) + 2, c)
    for relu in (False, True):
        for has_bias in (False, True):
            x64, w64 = inp.x.double().requires_grad_(True), inp.w.double().requires_grad_(True)
            b64 = inp.bias.double().requires_grad_(True) if has_bias else None
            out64 = F.conv2d(x64, w64, b64, c.stride, c.pad)
            if relu:
                out64 = torch.relu(out64)
            exp = torch.autograd.grad(out64, (x64, w64) + ((b64,) if has_bias else ()), inp.go.double())
            for kind in ("direct", "use_hip_convs", "set_backward_precision"):
                what = (kind, relu, has_bias)
                mod = _make(kind, c, has_bias, device)
                mod.relu = relu
                with torch.no_grad():
                    mod.weight.copy_(inp.w)
                    if has_bias:
                        mod.bias.copy_(inp.bias)
                xm = inp.x.to(device).requires_grad_(True)
                om = mod(xm)
                assert torch.equal(om.detach().cpu().double(), out64.detach()), what
                om.backward(inp.go.to(device))
                assert torch.equal(xm.grad.cpu().double(), exp[0]), what
                assert torch.equal(mod.weight.grad.cpu().double(), exp[1]), what
                if has_bias:
                    assert torch.equal(mod.bias.grad.cpu().double(), exp[2]), what


@pytest.mark.parametrize("c", C.MODULE_CASES[:2] + C.MODULE_CASES[3:], ids=R.case_id)
def test_layer_modes_reach_the_library(device, c):
    """Gaussian inputs: the f16x3 layer gives hip.ops.conv2d_backward_prec(precision="f16x3")'s bits, a layer left at the default (and the
    functional form without the argument) the old entry's."""
    C.assert_f16x3(c)
    hip.set_default_precision("f32")
    inp = C.cached_inputs("gauss", 9, c)
    new = C.device_backward(device, c, inp, True)
    old = R.device_backward(device, c, inp, False)
    for prec in ("f16x3", "f32"):
        mod = conv.Conv2d(c.Cin, c.Cout, c.k, c.stride, c.pad).to(device)
        assert mod.backward_precision == "f32"
        if prec == "f16x3":
            assert conv.set_backward_precision(nn.Sequential(mod, nn.ReLU()), prec) == 1
        with torch.no_grad():
            mod.weight.copy_(inp.w)
            mod.bias.copy_(inp.bias)
        xm = inp.x.to(device).requires_grad_(True)
        om = mod(xm)   # (relu off: the ungated backward)
        om.backward(inp.go.to(device))
        got = (xm.grad.cpu(), mod.weight.grad.cpu(), mod.bias.grad.cpu())
        ref = C.device_backward(device, c, inp, False, precision=prec)
        for name, a, e in zip(C.NAMES, got, ref):
            assert torch.equal(a, e), (prec, name)
        if prec == "f32":
            for name, a, e in zip(C.NAMES, got, old):
                assert torch.equal(a, e), ("default", name)
    # the functional form
    xd, wd = inp.x.to(device).requires_grad_(True), inp.w.to(device).requires_grad_(True)
    for prec, ref in ((None, old), ("f16x3", C.device_backward(device, c, inp, False))):
        out = conv.conv2d(xd, wd, None, c.stride, c.pad) if prec is None else conv.conv2d(xd, wd, None, c.stride, c.pad,
                                                                                          backward_precision=prec)
        gx, gw = torch.autograd.grad(out, (xd, wd), inp.go.to(device))
        assert torch.equal(gx.cpu(), ref[0]) and torch.equal(gw.cpu(), ref[1]), prec
    assert not torch.equal(new[1], R.device_backward(device, c, inp, True)[1])
