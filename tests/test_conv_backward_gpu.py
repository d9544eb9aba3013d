"""Conv2d backward on the device (pytest -m gpu): cp_conv2d_backward_nhwc, conv.conv2d / Conv2d and use_hip_convs against
torch.nn.functional.conv2d under float64 CPU autograd (tests/conv_backward_ref.py).  Dyadic inputs must match EXACTLY (the
generator's premise makes every gradient exact in float32 in any summation order); Gaussian inputs within 1e-4 x max
|reference| per gradient, the project's gradient tolerance (tests/test_dcn_backward_gpu.py, tests/test_pose_heads_gpu.py)."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from centerpose_amd import conv, hip
from tests import conv_backward_ref as R

pytestmark = pytest.mark.gpu
NAMES = ("grad_x", "grad_w", "grad_bias")


def _close(got, exp, tol, what):
    for name, a, e in zip(NAMES, got, exp):
        assert a.shape == e.shape, (what, name)
        scale = float(e.abs().max())
        err = float((a.double() - e.double()).abs().max())
        print("%s %s: max err %.3g, max |ref| %.3g" % (what, name, err, scale))
        assert err <= tol * scale + 1e-300, "%s %s: max err %.3g vs max |ref| %.3g" % (what, name, err, scale)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_dyadic_inputs_are_exact(device, c):
    inp = R.dyadic_inputs(sum(c), c)
    for gated in (False, True):
        got = R.device_backward(device, c, inp, gated)
        exp = R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, inp.y if gated else None)
        for name, a, e in zip(NAMES, got, exp):
            bad = int((a.double() != e).sum())
            print("%s gated=%d %s: %d of %d differ" % (R.case_id(c), gated, name, bad, e.numel()))
            assert a.shape == e.shape and torch.equal(a.double(), e), (name, gated, bad)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_gaussian_inputs(device, c):
    inp = R.gaussian_inputs(sum(c) + 1, c)
    for gated in (False, True):
        got = R.device_backward(device, c, inp, gated)
        exp = R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, inp.y if gated else None)
        _close(got, exp, 1e-4, "%s gated=%d" % (R.case_id(c), gated))


@pytest.mark.parametrize("scale", [1e-6, 1e3])
def test_input_range(device, scale):
    c = R.CASES[2]
    inp = R.gaussian_inputs(11, c)
    inp = inp._replace(x=inp.x * scale, w=inp.w * scale, go=inp.go * scale)
    got = R.device_backward(device, c, inp, True)
    _close(got, R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, inp.y), 1e-4, "scale %g" % scale)


@pytest.mark.parametrize("c", [R.CASES[0], R.GENERIC_CASES[0]], ids=R.case_id)
def test_two_calls_are_bit_identical(device, c):
    inp = R.gaussian_inputs(5, c)
    a = R.device_backward(device, c, inp, True)
    b = R.device_backward(device, c, inp, True)
    for name, p, q in zip(NAMES, a, b):
        assert torch.equal(p, q), name


@pytest.mark.parametrize("c", [R.CASES[1], R.PADDED_CASES[0], R.GENERIC_CASES[2]], ids=R.case_id)
def test_null_outputs_are_not_touched(device, c):
    inp = R.gaussian_inputs(6, c)
    full = R.device_backward(device, c, inp, True)
    Ho, Wo = R.out_size(c)
    L = hip.lib()
    x, w, go, y = (t.to(device) for t in (R.nhwc(inp.x), inp.w, R.nhwc(inp.go), R.nhwc(inp.y)))
    canary_x = torch.full((c.B, c.H, c.W, c.Cin), 7.25, device=device)
    canary_b = torch.full((c.Cout,), 7.25, device=device)
    gw = torch.full_like(w, 7.25)
    geo = (c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.stride, c.pad)
    nbytes = L.cp_conv2d_backward_workspace_bytes(*geo, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.cp_conv2d_backward_nhwc(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(x), p(w), p(y), p(go), None, p(gw),
                                   None, *geo, p(ws), nbytes)
    assert rc == 0, L.cp_last_error()
    torch.cuda.synchronize()
    assert bool((canary_x == 7.25).all()) and bool((canary_b == 7.25).all())
    assert torch.equal(gw.cpu(), full[1])
    # through the binding: the outputs that are asked for do not depend on the ones that are not
    for need_x, need_b in ((False, True), (True, False), (False, False)):
        gx, gw2, gb = R.device_backward(device, c, inp, True, need_x_grad=need_x, need_bias_grad=need_b)
        assert (gx is None) == (not need_x) and (gb is None) == (not need_b)
        assert torch.equal(gw2, full[1])
        assert gx is None or torch.equal(gx, full[0])
        assert gb is None or torch.equal(gb, full[2])


@pytest.mark.parametrize("c", [R.Case(5, 64, 64, 64, 64, 3, 1, 1), R.Case(5, 32, 64, 37, 45, 3, 2, 1)], ids=R.case_id)
def test_batch_split(device, c):
    inp = R.gaussian_inputs(7, c)
    whole = R.device_backward(device, c, inp, True)
    parts = []
    for lo, hi in ((0, 2), (2, 5)):
        sub = R.Inputs(inp.x[lo:hi], inp.w, inp.bias, inp.go[lo:hi], inp.y[lo:hi])
        parts.append(R.device_backward(device, c._replace(B=hi - lo), sub, True))
    joined = (torch.cat([parts[0][0], parts[1][0]]), parts[0][1] + parts[1][1], parts[0][2] + parts[1][2])
    _close(whole, joined, 1e-4, "batch split " + R.case_id(c))


MODULE_CASES = [R.Case(2, 64, 64, 16, 16, 3, 1, 1), R.Case(2, 32, 27, 9, 11, 3, 1, 1), R.Case(2, 64, 128, 13, 13, 1, 2, 0),
                R.Case(1, 32, 64, 12, 9, 3, 2, 1), R.Case(1, 8, 20, 9, 7, 3, 2, 1)]


@pytest.mark.parametrize("c", MODULE_CASES, ids=R.case_id)
def test_module_forward_and_backward_are_exact(device, c):
    hip.set_default_precision("f32")
    inp = R.dyadic_inputs(sum(c) + 2, c)
    for channels_last in (False, True):
        for relu in (False, True):
            for has_bias in (False, True):
                what = (channels_last, relu, has_bias)
                bias64 = inp.bias.double() if has_bias else None
                x64, w64 = inp.x.double().requires_grad_(True), inp.w.double().requires_grad_(True)
                b64 = bias64.requires_grad_(True) if has_bias else None
                out64 = F.conv2d(x64, w64, b64, c.stride, c.pad)
                if relu:
                    out64 = torch.relu(out64)
                exp = torch.autograd.grad(out64, (x64, w64) + ((b64,) if has_bias else ()), inp.go.double())
                xd = inp.x.to(device)
                if channels_last:
                    xd = xd.contiguous(memory_format=torch.channels_last)
                xd.requires_grad_(True)
                # the functional form
                wd = inp.w.to(device).requires_grad_(True)
                bd = inp.bias.to(device).requires_grad_(True) if has_bias else None
                out = conv.conv2d(xd, wd, bd, c.stride, c.pad, relu=relu)
                assert out.shape == out64.shape and out.is_contiguous(memory_format=torch.channels_last), what
                assert torch.equal(out.detach().cpu().double(), out64.detach()), what
                got = torch.autograd.grad(out, (xd, wd) + ((bd,) if has_bias else ()), inp.go.to(device))
                for a, e in zip(got, exp):
                    assert torch.equal(a.cpu().double(), e), what
                # the module, with and without a gradient for its input
                mod = conv.Conv2d(c.Cin, c.Cout, c.k, c.stride, c.pad, bias=has_bias).to(device)
                mod.relu = relu
                with torch.no_grad():
                    mod.weight.copy_(inp.w)
                    if has_bias:
                        mod.bias.copy_(inp.bias)
                for x_grad in (True, False):
                    xm = xd.detach().clone().requires_grad_(x_grad)
                    mod.zero_grad()
                    om = mod(xm)
                    assert torch.equal(om.detach(), out.detach()) and om.is_contiguous(memory_format=torch.channels_last), what
                    om.backward(inp.go.to(device))
                    assert (xm.grad is not None) == x_grad
                    if x_grad:
                        assert torch.equal(xm.grad.cpu().double(), exp[0]), what
                    assert torch.equal(mod.weight.grad.cpu().double(), exp[1]), what
                    if has_bias:
                        assert torch.equal(mod.bias.grad.cpu().double(), exp[2]), what


class _Block(nn.Module):
    """BasicBlock-shaped (pose_dla_dcn.py:48-62): conv3x3-BN-ReLU-conv3x3-BN, residual add, ReLU; a 1x1 projection of the
    residual when the block strides."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.project = nn.Conv2d(cin, cout, 1, stride, bias=True) if stride != 1 or cin != cout else None

    def forward(self, x):
        res = x if self.project is None else self.project(x)
        out = torch.relu(self.bn1(self.conv1(x)))
        return torch.relu(self.bn2(self.conv2(out)) + res)


@pytest.mark.parametrize("stride", [1, 2])
def test_use_hip_convs_basic_block_sgd_step(device, stride):
    hip.set_default_precision("f32")
    torch.manual_seed(stride)
    ref = _Block(64, 64, stride).double()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 64, 32, 32, generator=g)
    target = torch.randn(4, 64, 32 // stride, 32 // stride, generator=g)
    lr = 0.1
    dnet = copy.deepcopy(ref).float().to(device)
    params = dict(dnet.named_parameters())
    converted, skipped = conv.use_hip_convs(dnet)
    assert converted == ["conv1", "conv2"] + (["project"] if stride == 2 else []) and not skipped
    assert all(p is params[n] for n, p in dnet.named_parameters())
    opt = torch.optim.SGD(dnet.parameters(), lr=lr)
    opt.zero_grad()
    ((dnet(x.to(device)) - target.to(device)) ** 2).mean().backward()
    dev_grads = {n: p.grad.detach().cpu() for n, p in dnet.named_parameters()}
    opt.step()
    p0 = {n: p.detach().clone() for n, p in ref.named_parameters()}
    ((ref(x.double()) - target.double()) ** 2).mean().backward()
    for n, p in ref.named_parameters():
        gc = p.grad
        scale = float(gc.abs().max())
        err = float((dev_grads[n].double() - gc).abs().max())
        print("stride %d %s: grad err %.3g, max |ref| %.3g" % (stride, n, err, scale))
        assert scale > 0 and err <= 1e-3 * scale, n
        stepped = p0[n] - lr * gc
        assert float((params[n].detach().cpu().double() - stepped).abs().max()) <= 1e-3 * lr * scale + 1e-6, n


def test_dcn_with_converted_offset_convolution(device):
    """The mirror's DCN(64, 64, 3, 1, 1) with its conv_offset_mask on the library, against the same layer with torch's."""
    from centerpose_amd.lib.models.networks.DCNv2.dcn_v2 import DCN

    hip.set_default_precision("f32")
    torch.manual_seed(0)
    ref = DCN(64, 64, 3, 1, 1)
    with torch.no_grad():
        ref.conv_offset_mask.weight.normal_(0, 0.02)
        ref.conv_offset_mask.bias.normal_(0, 0.5)
    ref = ref.to(device)
    ours = copy.deepcopy(ref)
    converted, skipped = conv.use_hip_convs(ours.conv_offset_mask)
    assert converted == [""] and not skipped and type(ours.conv_offset_mask) is conv.Conv2d
    assert type(ref.conv_offset_mask) is nn.Conv2d
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 64, 24, 24, generator=g).to(device)
    go = torch.randn(2, 64, 24, 24, generator=g).to(device)
    res = []
    for net in (ours, ref):
        xi = x.clone().requires_grad_(True)
        y = net(xi)
        y.backward(go)
        res.append([("out", y.detach()), ("grad_x", xi.grad)] + [(n, p.grad) for n, p in net.named_parameters()])
    for (n, a), (_, e) in zip(*res):
        scale = float(e.abs().max())
        err = float((a - e).abs().max())
        print("dcn %s: err %.3g, max |ref| %.3g" % (n, err, scale))
        assert scale > 0 and err <= 1e-4 * scale, n
