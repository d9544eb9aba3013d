"""GPU tests of the ConvTranspose2d training path: cp_conv_transpose2d_dw_nhwc and cp_conv_transpose2d_backward_nhwc against
float64 CPU autograd (tests/deconv_backward_ref.py), the deconv.ConvTranspose2d module against nn.ConvTranspose2d, and one SGD
step of an IDAUp-shaped and a resdcn-shaped block with every parametrised layer on the library."""
import copy
import ctypes

import pytest
import torch
from torch import nn

from centerpose_amd import conv, deconv, hip, norm
from tests import deconv_backward_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _f32():
    """The dense forward follows the default precision: these tests compare it at float32 tolerances."""
    hip.set_default_precision("f32")
    yield
    hip.set_default_precision("f32")


def _device_run(device, c, inp, need_x=True):
    x, go = R.nhwc(inp.x).to(device), R.nhwc(inp.go).to(device)
    return hip.conv_transpose2d_backward(x, inp.w.to(device), go, c.stride, c.pad, c.groups, need_x_grad=need_x)


@pytest.mark.parametrize("c", R.DW_CASES + R.DENSE_CASES, ids=R.case_id)
def test_operators_against_float64_autograd(device, c):
    inp, ref = R.inputs(1, c), R.reference(1, c)
    x, w = R.nhwc(inp.x).to(device), inp.w.to(device)
    if c.groups != 1:
        add = R.nhwc(inp.add).to(device)
        y = hip.conv_transpose2d_dw(x, w, c.stride)
        ya = hip.conv_transpose2d_dw(x, w, c.stride, add=add)
        R.check(dict(y=R.nchw(y), y_add=R.nchw(ya)), ref, R.case_id(c))
    else:
        R.check(dict(y=R.nchw(hip.conv_transpose2d(x, w))), ref, R.case_id(c))
    gx, gw = _device_run(device, c, inp)
    R.check(dict(grad_x=R.nchw(gx), grad_w=gw), ref, R.case_id(c))
    # need_x_grad=False: no grad_x, the same grad_w bitwise
    none, gw2 = _device_run(device, c, inp, need_x=False)
    assert none is None and torch.equal(gw2, gw)
    # two calls are bit-identical
    gx3, gw3 = _device_run(device, c, inp)
    assert torch.equal(gx3, gx) and torch.equal(gw3, gw)


@pytest.mark.parametrize("c", [R.DW_CASES[3], R.DW_CASES[4], R.DENSE_CASES[1]], ids=R.case_id)
def test_outputs_stay_inside_guard_bands(device, c):
    """Through the C ABI with every output inside a canary buffer: the guard bands on both sides stay as they were."""
    inp = R.inputs(2, c)
    L = hip.lib()
    G = 1024
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, go, w = R.nhwc(inp.x).to(device), R.nhwc(inp.go).to(device), inp.w.to(device)
    exp_gx, exp_gw = _device_run(device, c, inp)
    nbytes = L.cp_conv_transpose2d_backward_workspace_bytes(*R.geo(c), 1)
    assert nbytes > 0
    ws = torch.full((nbytes + 8 * G,), 0x5a, dtype=torch.uint8, device=device)
    bufs = [torch.full((n + 2 * G,), 7.25, device=device) for n in (x.numel(), w.numel(), go.numel())]  # grad_x, grad_w, out
    rc = L.cp_conv_transpose2d_backward_nhwc(stream, p(x), p(w), p(go), p(bufs[0], G), p(bufs[1], G), *R.geo(c), p(ws, G), nbytes)
    assert rc == 0, L.cp_last_error()
    if c.groups != 1:
        add = R.nhwc(inp.add).to(device)
        rc = L.cp_conv_transpose2d_dw_nhwc(stream, p(x), p(w), p(add), p(bufs[2], G), c.B, c.H, c.W, c.Cin, c.stride)
        assert rc == 0, L.cp_last_error()
    torch.cuda.synchronize()
    for t in bufs:
        assert bool((t[:G] == 7.25).all()) and bool((t[-G:] == 7.25).all())
    assert bool((ws[:4 * G] == 0x5a).all()) and bool((ws[-4 * G:] == 0x5a).all())
    assert torch.equal(bufs[0][G:-G].view_as(x), exp_gx) and torch.equal(bufs[1][G:-G].view_as(w), exp_gw)
    if c.groups != 1:
        assert torch.equal(bufs[2][G:-G].view_as(go), hip.conv_transpose2d_dw(x, w, c.stride, add=add))
    # a NULL grad_x is not touched: nothing else is written either
    gw_only = torch.full((w.numel() + 2 * G,), 7.25, device=device)
    rc = L.cp_conv_transpose2d_backward_nhwc(stream, p(x), p(w), p(go), None, p(gw_only, G), *R.geo(c), p(ws, G), nbytes)
    assert rc == 0, L.cp_last_error()
    torch.cuda.synchronize()
    assert bool((gw_only[:G] == 7.25).all()) and bool((gw_only[-G:] == 7.25).all())
    assert torch.equal(gw_only[G:-G].view_as(w), exp_gw)
    assert bool((ws[:4 * G] == 0x5a).all()) and bool((ws[-4 * G:] == 0x5a).all())


MODULE_CASES = [R.DW_CASES[1], R.DW_CASES[4], R.DENSE_CASES[1]]


@pytest.mark.parametrize("x_grad", [True, False], ids=["x_grad", "no_x_grad"])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("c", MODULE_CASES, ids=R.case_id)
def test_module_against_nn_conv_transpose2d(device, c, layout, x_grad):
    torch.manual_seed(5)
    theirs = nn.ConvTranspose2d(c.Cin, c.Cout, c.K, c.stride, c.pad, groups=c.groups, bias=False)
    with torch.no_grad():
        theirs.weight.normal_()
    ours = copy.deepcopy(theirs).to(device)
    theirs = theirs.double()
    params = dict(ours.named_parameters())
    assert deconv.use_hip_deconvs(ours) == ([""], {}) and type(ours) is deconv.ConvTranspose2d
    assert all(p is params[n] for n, p in ours.named_parameters())
    inp = R.inputs(3, c)
    fmt = torch.channels_last if layout == "channels_last" else torch.contiguous_format
    xd = inp.x.to(device).contiguous(memory_format=fmt).requires_grad_(x_grad)
    xr = inp.x.double().requires_grad_(x_grad)
    with_add = c.groups != 1
    if with_add:
        addd = inp.add.to(device).contiguous(memory_format=fmt).requires_grad_(True)
        addr = inp.add.double().requires_grad_(True)
        y, yr = ours(xd, addd), theirs(xr) + addr
    else:
        y, yr = ours(xd), theirs(xr)
    assert y.shape == yr.shape and y.is_contiguous(memory_format=torch.channels_last)
    god = inp.go.to(device).contiguous(memory_format=fmt)
    seen = []  # the function's own grad_x (a leaf's .grad is re-laid-out to the leaf's strides)
    if x_grad:
        xd.register_hook(lambda t: seen.append(t.is_contiguous(memory_format=torch.channels_last)))
    y.backward(god)
    yr.backward(inp.go.double())
    got, exp = dict(y=y, grad_w=ours.weight.grad), dict(y=yr.detach(), grad_w=theirs.weight.grad)
    if x_grad:
        got["grad_x"], exp["grad_x"] = xd.grad, xr.grad
        assert seen == [True]
    else:
        assert xd.grad is None
    R.check(got, exp, "%s %s" % (R.case_id(c), layout))
    if with_add:
        assert torch.equal(addd.grad, god) and torch.equal(addr.grad, inp.go.double())
    assert ours.weight.grad.shape == ours.weight.shape


def test_add_gradient_is_grad_out_itself(device):
    c = R.DW_CASES[1]
    inp = R.inputs(4, c)
    x, w = inp.x.to(device).requires_grad_(True), inp.w.to(device).requires_grad_(True)
    add = inp.add.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = deconv.conv_transpose2d(x, w, c.stride, c.pad, c.groups, add=add)
    go = inp.go.to(device).contiguous(memory_format=torch.channels_last)
    fn = y.grad_fn
    assert len(fn.saved_tensors) == 2  # x and weight only
    grads = fn.apply(go)  # (the node's Python side: the autograd function's backward on this context)
    assert len(grads) == 6 and grads[2] is go  # grad_out itself, not a copy
    assert grads[0].shape == x.shape and grads[1].shape == w.shape and grads[3:] == (None, None, None)
    with pytest.raises(NotImplementedError, match="depth-wise"):
        d = R.DENSE_CASES[0]
        di = R.inputs(4, d)
        deconv.conv_transpose2d(di.x.to(device), di.w.to(device), 2, 1, 1, add=torch.zeros(1, 32, 2, 2, device=device))
    with pytest.raises(RuntimeError, match="add has shape"):
        deconv.conv_transpose2d(x, w, c.stride, c.pad, c.groups, add=add[:, :, :-1])


class _IdaStep(nn.Module):
    """One IDAUp step (pose_dla_dcn.py:411-417) with a plain 3x3 in the node's place:
    node(up(relu(bn(proj(x)))) + skip)."""

    def __init__(self):
        super().__init__()
        self.proj = nn.Conv2d(64, 32, 1, bias=False)
        self.bn = nn.BatchNorm2d(32)
        self.up = nn.ConvTranspose2d(32, 32, 4, stride=2, padding=1, groups=32, bias=False)
        self.node = nn.Conv2d(32, 32, 3, padding=1, bias=False)

    def forward(self, x, skip):
        return self.node(self.up(torch.relu(self.bn(self.proj(x)))) + skip)


class _IdaStepFused(_IdaStep):
    """_IdaStep after INTEGRATION.md's edits: bn.relu = True and the skip tensor goes into the up-sampling layer as `add`."""

    def forward(self, x, skip):
        return self.node(self.up(self.bn(self.proj(x)), skip))


class _ResdcnPair(nn.Module):
    """resnet_dcn.py:232-240's dense deconv -> BatchNorm2d -> ReLU."""

    def __init__(self):
        super().__init__()
        self.up = nn.ConvTranspose2d(64, 64, 4, stride=2, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(64)

    def forward(self, x, skip=None):
        return torch.relu(self.bn(self.up(x)))


class _ResdcnPairFused(_ResdcnPair):
    def forward(self, x, skip=None):
        return self.bn(self.up(x))


@pytest.mark.parametrize("kind", ["idaup", "resdcn"])
def test_sgd_step_with_the_up_sampling_layer_on_the_library(device, kind):
    torch.manual_seed(11)
    ref = (_IdaStep() if kind == "idaup" else _ResdcnPair()).double()
    with torch.no_grad():
        ref.up.weight.normal_(0.0, 0.5)  # (not fill_up_weights' symmetric kernel)
    g = torch.Generator().manual_seed(3)
    cout = 32 if kind == "idaup" else 64
    x = torch.randn(2, 64, 12, 12, generator=g)
    skip = torch.randn(2, cout, 24, 24, generator=g)
    target = torch.randn(2, cout, 24, 24, generator=g)
    lr = 0.1
    dnet = copy.deepcopy(ref).float().to(device)
    dnet.__class__ = _IdaStepFused if kind == "idaup" else _ResdcnPairFused
    params = dict(dnet.named_parameters())
    assert conv.use_hip_convs(dnet)[0] == (["proj", "node"] if kind == "idaup" else [])
    assert norm.use_hip_norms(dnet) == (["bn"], {})
    assert deconv.use_hip_deconvs(dnet) == (["up"], {})
    dnet.bn.relu = True
    assert all(p is params[n] for n, p in dnet.named_parameters())
    opt = torch.optim.SGD(dnet.parameters(), lr=lr)
    opt.zero_grad()
    ((dnet(x.to(device), skip.to(device)) - target.to(device)) ** 2).mean().backward()
    dev_grads = {n: p.grad.detach().cpu() for n, p in dnet.named_parameters()}
    opt.step()
    p0 = {n: p.detach().clone() for n, p in ref.named_parameters()}
    ((ref(x.double(), skip.double()) - target.double()) ** 2).mean().backward()
    for n, p in ref.named_parameters():
        gc = p.grad
        scale = float(gc.abs().max())
        err = float((dev_grads[n].double() - gc).abs().max())
        print("%s %s: grad err %.3g, max |ref| %.3g" % (kind, n, err, scale))
        assert scale > 0 and err <= 1e-3 * scale, n
        stepped = p0[n] - lr * gc
        assert float((params[n].detach().cpu().double() - stepped).abs().max()) <= 1e-3 * lr * scale + 1e-6, n
