"""The low-channel 3x3 conv backward path on the device (pytest -m gpu): conv_bwd_lowc.hip through cp_conv2d_backward_nhwc and
through conv.Conv2d, against torch.nn.functional.conv2d under float64 CPU autograd (tests/conv_backward_ref.py).  Dyadic inputs
must match EXACTLY (the generator's premise makes every gradient exact in float32 in any summation order, so a wrong tap,
parity class, halo pixel, ragged tile or slab breaks equality); Gaussian inputs within 1e-4 x max |reference| per gradient, the
project's gradient tolerance (tests/test_conv_backward_gpu.py).  Cases: tests/conv_lowc_cases.py."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from centerpose_amd import conv, hip
from tests import conv_backward_ref as R
from tests import conv_lowc_cases as LC

pytestmark = pytest.mark.gpu
NAMES = ("grad_x", "grad_w", "grad_bias")
CASES = LC.ALL_LOWC + [LC.BELOW_CASE]


@functools.lru_cache(maxsize=None)
def _dyadic(c):
    inp = R.dyadic_inputs(sum(c), c)
    return inp, {g: R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, inp.y if g else None) for g in (False, True)}


@functools.lru_cache(maxsize=None)
def _gaussian(c):
    inp = R.gaussian_inputs(sum(c) + 1, c)
    return inp, {g: R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, inp.y if g else None) for g in (False, True)}


def _close(got, exp, tol, what):
    for name, a, e in zip(NAMES, got, exp):
        assert a.shape == e.shape, (what, name)
        scale = float(e.abs().max())
        err = float((a.double() - e.double()).abs().max())
        print("%s %s: max err %.3g, max |ref| %.3g" % (what, name, err, scale))
        assert err <= tol * scale + 1e-300, "%s %s: max err %.3g vs max |ref| %.3g" % (what, name, err, scale)


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_paths(c):
    assert hip.conv2d_backward_path(*LC.geo(c)) == (LC.GENERIC if c == LC.BELOW_CASE else LC.LOWC)


@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_dyadic_inputs_are_exact(device, c, gated):
    inp, exp = _dyadic(c)
    got = R.device_backward(device, c, inp, gated)
    for name, a, e in zip(NAMES, got, exp[gated]):
        bad = int((a.double() != e).sum())
        print("%s gated=%d %s: %d of %d differ" % (R.case_id(c), gated, name, bad, e.numel()))
        assert a.shape == e.shape and torch.equal(a.double(), e), (name, gated, bad)


@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_gaussian_inputs(device, c, gated):
    inp, exp = _gaussian(c)
    _close(R.device_backward(device, c, inp, gated), exp[gated], 1e-4, "%s gated=%d" % (R.case_id(c), gated))


@pytest.mark.parametrize("c", LC.ALL_LOWC, ids=R.case_id)
def test_reduced_outputs(device, c):
    """The outputs that are asked for do not depend on the ones that are not, and a NULL output is not written."""
    inp, exp = _gaussian(c)
    full = R.device_backward(device, c, inp, True)
    _close(full, exp[True], 1e-4, R.case_id(c))
    for need_x, need_b in ((False, True), (True, False), (False, False)):
        gx, gw, gb = R.device_backward(device, c, inp, True, need_x_grad=need_x, need_bias_grad=need_b)
        assert (gx is None) == (not need_x) and (gb is None) == (not need_b)
        assert torch.equal(gw, full[1])
        assert gx is None or torch.equal(gx, full[0])
        assert gb is None or torch.equal(gb, full[2])
    # the raw call with NULL grad_x and grad_bias and the smaller workspace of need_grad_x = 0; dyadic, so exact
    inp, exp = _dyadic(c)
    L = hip.lib()
    x, w, go, y = (t.to(device) for t in (R.nhwc(inp.x), inp.w, R.nhwc(inp.go), R.nhwc(inp.y)))
    canary_x = torch.full((c.B, c.H, c.W, c.Cin), 7.25, device=device)
    canary_b = torch.full((c.Cout,), 7.25, device=device)
    gw = torch.full_like(w, 7.25)
    nbytes = L.cp_conv2d_backward_workspace_bytes(*LC.geo(c), 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.cp_conv2d_backward_nhwc(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(x), p(w), p(y), p(go), None, p(gw),
                                   None, *LC.geo(c), p(ws), nbytes)
    assert rc == 0, L.cp_last_error()
    torch.cuda.synchronize()
    assert bool((canary_x == 7.25).all()) and bool((canary_b == 7.25).all())
    assert torch.equal(gw.cpu().double(), exp[True][1])


@pytest.mark.parametrize("c", [LC.LOWC_CASES[0], LC.LOWC_CASES[2]], ids=R.case_id)
def test_two_calls_are_bit_identical(device, c):
    inp, _ = _gaussian(c)
    a = R.device_backward(device, c, inp, True)
    b = R.device_backward(device, c, inp, True)
    for name, p, q in zip(NAMES, a, b):
        assert torch.equal(p, q), name


def test_batch_split(device):
    c = LC.LOWC_CASES[2]._replace(B=5)   # 16 -> 32 on 75 x 133, stride 2: 2 + 3 images, both parts on the path
    inp = R.gaussian_inputs(7, c)
    whole = R.device_backward(device, c, inp, True)
    parts = []
    for lo, hi in ((0, 2), (2, 5)):
        sub_c = c._replace(B=hi - lo)
        assert hip.conv2d_backward_path(*LC.geo(sub_c)) == LC.LOWC
        sub = R.Inputs(inp.x[lo:hi], inp.w, inp.bias, inp.go[lo:hi], inp.y[lo:hi])
        parts.append(R.device_backward(device, sub_c, sub, True))
    joined = (torch.cat([parts[0][0], parts[1][0]]), parts[0][1] + parts[1][1], parts[0][2] + parts[1][2])
    _close(whole, joined, 1e-4, "batch split " + R.case_id(c))
    assert torch.equal(whole[0], joined[0])   # an image's data gradient does not depend on its neighbours


@pytest.mark.parametrize("B,cout,stride", [(2, 16, 1), (4, 32, 2)])
def test_module_forward_and_backward_are_exact(device, B, cout, stride):
    """conv.Conv2d(16, cout, 3, stride, padding=1, bias=False) on 37 x 131 images (the first case's; four of them at stride 2,
    where two have 2508 output pixels) reaches the path through the operator."""
    hip.set_default_precision("f32")
    c = R.Case(B, 16, cout, 37, 131, 3, stride, 1)
    assert hip.conv2d_backward_path(*LC.geo(c)) == LC.LOWC
    inp = R.dyadic_inputs(sum(c) + 2, c)
    x64, w64 = inp.x.double().requires_grad_(True), inp.w.double().requires_grad_(True)
    out64 = F.conv2d(x64, w64, None, stride, 1)
    exp = torch.autograd.grad(out64, (x64, w64), inp.go.double())
    m = conv.Conv2d(16, cout, 3, stride=stride, padding=1, bias=False).to(device)
    with torch.no_grad():
        m.weight.copy_(inp.w.to(device))
    xd = inp.x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = m(xd)
    assert torch.equal(out.detach().cpu().double(), out64.detach())
    out.backward(inp.go.to(device))
    assert torch.equal(xd.grad.cpu().double(), exp[0])
    assert torch.equal(m.weight.grad.cpu().double(), exp[1])
