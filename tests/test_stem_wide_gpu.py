"""GPU tests of the image stems above 64 output channels (centerpose_amd/stem.py; cp_conv2d_stem_wide_backward: the kernels of
cp_conv2d_stem_backward run over channel blocks of at most 64), after tests/test_stem_gpu.py, with its references and bounds.

Reference: ``F.conv2d`` under CPU autograd in float64.  Dyadic inputs (integers in [-2, 2]: every partial sum of every gradient
is an integer below 2^24 in any order) must match EXACTLY; Gaussian inputs within 1e-4 x max |reference| per gradient, the
project's gradient tolerance.  Results are bitwise the same from call to call.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import conv_backward_ref as R

pytestmark = pytest.mark.gpu

# (Cin, Cout, stride, H, W, B)
CASES = [(3, 128, 2, 10, 13, 2),     # two full channel blocks: the hourglass's stem (large_hourglass.py:210)
         (3, 80, 1, 9, 11, 1),       # a full block and a ragged one of 16
         (1, 96, 2, 7, 7, 1),        # a full block and a ragged one of 32; the image is smaller than the halo
         (3, 128, 2, 140, 132, 2)]   # 9 x 2 tiles of 8 x 64 output pixels per image, ragged last row band and column band


def _case(t):
    cin, cout, stride, H, W, B = t
    return R.Case(B, cin, cout, H, W, 7, stride, 3)


def _id(t):
    return "%dto%d_s%d_%dx%d_B%d" % t


def _reference(c, inp, gated):
    _, gw, gb = R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, y=inp.y if gated else None)
    return gw, gb


def _device(device, c, inp, gated, bias):
    from centerpose_amd import hip

    gw, gb = hip.conv2d_stem_backward(inp.x.to(device), R.nhwc(inp.go).to(device), stride=c.stride,
                                      y=R.nhwc(inp.y).to(device) if gated else None, need_bias_grad=bias)
    assert (gb is None) == (not bias)
    return gw.cpu(), gb.cpu() if bias else None


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("gated", [True, False], ids=["gated", "plain"])
@pytest.mark.parametrize("t", CASES, ids=_id)
def test_dyadic_exact(device, t, gated, bias):
    c = _case(t)
    inp = R.dyadic_inputs(500 + CASES.index(t), c)
    gw_ref, gb_ref = _reference(c, inp, gated)
    gw, gb = _device(device, c, inp, gated, bias)
    assert torch.equal(gw.double(), gw_ref)
    if bias:
        assert torch.equal(gb.double(), gb_ref)
    gw2, gb2 = _device(device, c, inp, gated, bias)
    assert torch.equal(gw, gw2) and (not bias or torch.equal(gb, gb2))


@pytest.mark.parametrize("gated", [True, False], ids=["gated", "plain"])
@pytest.mark.parametrize("t", CASES, ids=_id)
def test_gaussian(device, t, gated):
    c = _case(t)
    inp = R.gaussian_inputs(600 + CASES.index(t), c)
    gw_ref, gb_ref = _reference(c, inp, gated)
    gw, gb = _device(device, c, inp, gated, True)
    for name, got, ref in (("grad_w", gw, gw_ref), ("grad_bias", gb, gb_ref)):
        err, lim = float((got.double() - ref).abs().max()), 1e-4 * float(ref.abs().max())
        print("%s %s %s: err %.3e limit %.3e" % (_id(t), "gated" if gated else "plain", name, err, lim))
        assert err <= lim, name
    gw2, gb2 = _device(device, c, inp, gated, True)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)  # call to call


def test_narrow_stems_give_the_same_bits_through_either_entry_point(device):
    """Up to 64 channels there is one channel block: cp_conv2d_stem_wide_backward is cp_conv2d_stem_backward."""
    from centerpose_amd import hip

    c = _case((3, 48, 2, 20, 70, 2))
    inp = R.gaussian_inputs(650, c)
    gw, gb = _device(device, c, inp, True, True)
    L = hip.lib()
    geo = (c.B, c.H, c.W, c.Cin, c.Cout, c.stride)
    nbytes = L.cp_conv2d_stem_wide_backward_workspace_bytes(*geo)
    assert nbytes == L.cp_conv2d_stem_backward_workspace_bytes(*geo) > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    x, go, y = inp.x.to(device), R.nhwc(inp.go).to(device), R.nhwc(inp.y).to(device)
    gw2, gb2 = torch.empty(c.Cout, c.Cin, 7, 7, device=device), torch.empty(c.Cout, device=device)
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    rc = L.cp_conv2d_stem_wide_backward(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(x), p(go), p(y), p(gw2), p(gb2),
                                        p(ws), nbytes, *geo)
    assert rc == 0, L.cp_last_error()
    assert torch.equal(gw2.cpu(), gw) and torch.equal(gb2.cpu(), gb)


@pytest.mark.parametrize("t", [CASES[0], CASES[3]], ids=_id)
def test_workspace_canary_and_unrequested_bias(device, t):
    """At Cout = 128 the operator writes inside the queried workspace only, and a NULL grad_bias is not touched."""
    from centerpose_amd import hip

    c = _case(t)
    inp = R.dyadic_inputs(700, c)
    gw_ref, _ = _reference(c, inp, True)
    L = hip.lib()
    geo = (c.B, c.H, c.W, c.Cin, c.Cout, c.stride)
    nbytes = L.cp_conv2d_stem_wide_backward_workspace_bytes(*geo)
    assert nbytes > 0 and nbytes % 256 == 0
    words = 1024
    ws = torch.full((nbytes // 4 + words,), 0x5A5A5A5A, dtype=torch.int32, device=device)
    x, go, y = inp.x.to(device), R.nhwc(inp.go).to(device), R.nhwc(inp.y).to(device)
    gw = torch.full((c.Cout, c.Cin, 7, 7), 7.25, device=device)
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.cp_conv2d_stem_wide_backward(stream, p(x), p(go), p(y), p(gw), None, p(ws), nbytes, *geo)
    assert rc == 0, L.cp_last_error()
    torch.cuda.synchronize()
    assert bool((ws[nbytes // 4:] == 0x5A5A5A5A).all())
    assert torch.equal(gw.cpu().double(), gw_ref)
    # one byte short is refused before any launch
    gw.fill_(7.25)
    rc = L.cp_conv2d_stem_wide_backward(stream, p(x), p(go), p(y), p(gw), None, p(ws), nbytes - 1, *geo)
    torch.cuda.synchronize()
    assert rc == -1 and b"workspace" in L.cp_last_error() and bool((gw == 7.25).all())


@pytest.mark.parametrize("relu,bias", [(False, False), (True, True)])
def test_module_forward_backward(device, relu, bias):
    """StemConv2d(3, 128, 7, stride=2, padding=3) against F.conv2d in float64: the forward and the gradients through autograd."""
    from centerpose_amd import hip, stem

    c = _case(CASES[0])
    inp = R.gaussian_inputs(800, c)
    hip.set_default_precision("f32")
    m = stem.StemConv2d(c.Cin, c.Cout, 7, stride=c.stride, padding=3, bias=bias)
    m.relu = relu
    with torch.no_grad():
        m.weight.copy_(inp.w)
        if bias:
            m.bias.copy_(inp.bias)
    w64 = inp.w.double().requires_grad_(True)
    b64 = inp.bias.double().requires_grad_(True) if bias else None
    y64 = F.conv2d(inp.x.double(), w64, b64, c.stride, 3)
    if relu:
        y64 = F.relu(y64)
    g64 = torch.autograd.grad(y64, [w64] + ([b64] if bias else []), inp.go.double())
    m = m.to(device)
    y = m(inp.x.to(device))
    assert y.is_contiguous(memory_format=torch.channels_last)
    y.backward(inp.go.to(device))
    assert float((y.detach().cpu().double() - y64.detach()).abs().max()) <= 1e-4 * float(y64.abs().max())
    got = [m.weight.grad] + ([m.bias.grad] if bias else [])
    for a, r in zip(got, g64):
        assert float((a.cpu().double() - r).abs().max()) <= 1e-4 * float(r.abs().max())
