"""The f16x3 mode of the dense ConvTranspose2d backward on the device (pytest -m gpu): cp_conv_transpose2d_backward_prec_nhwc with
CP_PREC_F16X3, and deconv.ConvTranspose2d / use_hip_deconvs / set_backward_precision with backward_precision = "f16x3", against
torch.nn.functional.conv_transpose2d under float64 CPU autograd.  Inputs, their premises and the cases:
tests/deconv_backward_f16x3_cases.py.  Every test of a dense case first asserts, through cp_conv_transpose2d_backward_prec_mask,
that both contractions run in f16x3."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from centerpose_amd import deconv, hip
from tests import deconv_backward_f16x3_cases as C
from tests import deconv_backward_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _f32():
    """The dense forward follows the default precision: the layer tests compare it exactly."""
    hip.set_default_precision("f32")
    yield
    hip.set_default_precision("f32")


@pytest.mark.parametrize("c", C.CASES, ids=R.case_id)
def test_dyadic_inputs_are_exact(device, c):
    C.assert_mask(c)
    inp = C.cached_inputs("dyadic", sum(c), c)
    C.assert_equal(C.device_backward(device, c, inp), C.cached_reference("dyadic", sum(c), c), R.case_id(c))


@pytest.mark.parametrize("which", ["xw", "go"])
@pytest.mark.parametrize("c", C.TWO_LEVEL_CASES, ids=R.case_id)
def test_two_level_dyadic_inputs_are_exact(device, c, which):
    """Exact only if every cross term (hi*lo and lo*hi) of every product is there."""
    C.assert_mask(c)
    kind, seed = "two_" + which, sum(c) + 3
    got = C.device_backward(device, c, C.cached_inputs(kind, seed, c))
    C.assert_equal(got, C.cached_reference(kind, seed, c), "%s %s" % (R.case_id(c), which))


@pytest.mark.parametrize("c", C.CASES, ids=R.case_id)
def test_gaussian_inputs(device, c):
    C.assert_mask(c)
    inp, exp = C.cached_inputs("gauss", sum(c) + 1, c), C.cached_reference("gauss", sum(c) + 1, c)
    f32 = C.device_backward(device, c, inp, precision="f32")
    got = C.device_backward(device, c, inp)
    for (n, e16, s), (_, e32, _) in zip(C.errors(got, exp), C.errors(f32, exp)):
        print("%s %s: f16x3 err %.3g, f32 err %.3g, max |ref| %.3g" % (R.case_id(c), n, e16, e32, s))
    C.assert_close(got, exp, 1e-4, R.case_id(c))
    # the other kernels ran: not the float32 mode's bits; and the float32 mode is the plain entry
    assert not torch.equal(got[0], f32[0]) and not torch.equal(got[1], f32[1])
    gx, gw = hip.conv_transpose2d_backward(R.nhwc(inp.x).to(device), inp.w.to(device), R.nhwc(inp.go).to(device), 2, 1, 1)
    assert torch.equal(R.nchw(gx).cpu(), f32[0]) and torch.equal(gw.cpu(), f32[1])
    # bitwise reproducible call to call
    again = C.device_backward(device, c, inp)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


@pytest.mark.parametrize("c", [C.CASES[1], C.CASES[3]], ids=R.case_id)
def test_without_grad_x(device, c):
    """need_x_grad=False: no grad_x, the same grad_w, and a workspace without the data gradient's part."""
    C.assert_mask(c)
    inp = C.cached_inputs("gauss", sum(c) + 1, c)
    full = C.device_backward(device, c, inp)
    none, gw = C.device_backward(device, c, inp, need_x_grad=False)
    assert none is None and torch.equal(gw, full[1])
    L, f16 = hip.lib(), hip.PRECISIONS["f16x3"]
    with_x, without = (L.cp_conv_transpose2d_backward_prec_workspace_bytes(*R.geo(c), nx, f16) for nx in (1, 0))
    assert 0 < without < with_x
    assert without > L.cp_conv_transpose2d_backward_workspace_bytes(*R.geo(c), 0) > 0


@pytest.mark.parametrize("c", [R.DW_CASES[1], R.DW_CASES[4]], ids=R.case_id)
def test_depthwise_layers_stay_float32(device, c):
    C.assert_mask(c, 0)
    inp = R.inputs(4, c)
    a = C.device_backward(device, c, inp, precision="f16x3")
    b = C.device_backward(device, c, inp, precision="f32")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    L = hip.lib()
    assert (L.cp_conv_transpose2d_backward_prec_workspace_bytes(*R.geo(c), 1, hip.PRECISIONS["f16x3"])
            == L.cp_conv_transpose2d_backward_workspace_bytes(*R.geo(c), 1))


def _make(kind, c, device):
    """A deconv.ConvTranspose2d in f16x3 backward mode, built in one of the three ways."""
    if kind == "direct":
        mod = deconv.ConvTranspose2d(c.Cin, c.Cout, 4, 2, 1, bias=False).to(device)
        assert mod.backward_precision == "f32"
        mod.backward_precision = "f16x3"
    else:
        mod = nn.ConvTranspose2d(c.Cin, c.Cout, 4, 2, 1, bias=False).to(device)
        if kind == "use_hip_deconvs":
            assert deconv.use_hip_deconvs(mod, backward_precision="f16x3") == ([""], {})
        else:
            assert deconv.use_hip_deconvs(mod) == ([""], {}) and mod.backward_precision == "f32"
            assert deconv.set_backward_precision(nn.Sequential(mod, nn.ReLU()), "f16x3") == 1
    assert type(mod) is deconv.ConvTranspose2d and mod.backward_precision == "f16x3"
    return mod


@pytest.mark.parametrize("c", [C.CASES[1], C.CASES[2]], ids=R.case_id)
def test_layer_modes_reach_the_library(device, c):
    """Dyadic inputs: the layer in f16x3 mode, built each way, is exact.  Gaussian inputs: it gives the operator's f16x3 bits, a
    layer left at the default (and the functional form without the argument) the float32 entry's."""
    C.assert_mask(c)
    inp = C.cached_inputs("dyadic", sum(c) + 2, c)
    exp = C.cached_reference("dyadic", sum(c) + 2, c)
    out64 = F.conv_transpose2d(inp.x.double(), inp.w.double(), None, 2, 1)
    for kind in ("direct", "use_hip_deconvs", "set_backward_precision"):
        mod = _make(kind, c, device)
        with torch.no_grad():
            mod.weight.copy_(inp.w)
        xm = inp.x.to(device).requires_grad_(True)
        om = mod(xm)
        assert torch.equal(om.detach().cpu().double(), out64), kind
        om.backward(inp.go.to(device))
        C.assert_equal((xm.grad.cpu(), mod.weight.grad.cpu()), exp, kind)
    inp = C.cached_inputs("gauss", 9, c)
    for prec in ("f16x3", "f32"):
        ref = C.device_backward(device, c, inp, precision=prec)
        mod = deconv.ConvTranspose2d(c.Cin, c.Cout, 4, 2, 1, bias=False).to(device)
        if prec == "f16x3":
            assert deconv.set_backward_precision(mod, prec) == 1
        with torch.no_grad():
            mod.weight.copy_(inp.w)
        xm = inp.x.to(device).requires_grad_(True)
        mod(xm).backward(inp.go.to(device))
        assert torch.equal(xm.grad.cpu(), ref[0]) and torch.equal(mod.weight.grad.cpu(), ref[1]), prec
        xd, wd = inp.x.to(device).requires_grad_(True), inp.w.to(device).requires_grad_(True)
        kw = {} if prec == "f32" else dict(backward_precision=prec)
        gx, gw = torch.autograd.grad(deconv.conv_transpose2d(xd, wd, 2, 1, **kw), (xd, wd), inp.go.to(device))
        assert torch.equal(gx.cpu(), ref[0]) and torch.equal(gw.cpu(), ref[1]), prec
    with pytest.raises(ValueError, match="backward_precision"):
        deconv.set_backward_precision(mod, "f16")
