"""Training GroupNorm on the device (pytest -m gpu): cp_groupnorm_forward_nhwc / cp_groupnorm_backward_nhwc,
group_norm.group_norm / GroupNorm and use_hip_group_norms against F.group_norm + ReLU under float64 CPU autograd
(tests/groupnorm_ref.py).  Everything is compared at 1e-4 x max |reference| per output, the project's gradient tolerance."""
import copy
import ctypes

import pytest
import torch
from torch import nn

from centerpose_amd import conv, group_norm, hip
from tests import groupnorm_ref as R

pytestmark = pytest.mark.gpu
GRID = [(act, affine) for act in (0, 1) for affine in (True, False)]


def _both(device, inp, c, act, affine=True):
    fwd = R.device_forward(device, inp, c, act, affine)
    return fwd, R.device_backward(device, inp, c, fwd, act, affine)


def _check_both(device, inp, c, act, what, affine=True):
    fwd, bwd = _both(device, inp, c, act, affine)
    R.check(fwd[0], R.reference_forward(inp, c, act, affine), what)
    R.check(bwd, R.reference_backward(inp, c, fwd[0]["y"] if act else None, affine), what)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_forward_and_backward(device, c):
    inp = R.inputs(sum(c), c)
    for act, affine in GRID:
        _check_both(device, inp, c, act, "%s act=%d affine=%d" % (R.case_id(c), act, affine), affine)


@pytest.mark.parametrize("c", R.LARGE_MEAN_CASES, ids=R.case_id)
def test_large_mean(device, c):
    """x = 1000 + N(0, 1): E[x^2] - mean^2 from raw float32 sums is wrong by tens of per cent here, and torch's own float32
    GroupNorm is at 1e-4 .. 1.3e-3 of the maximum.  Pivoted sums merged by Chan's rule stay inside the limit; the worst output
    is grad_gamma = sum g xhat, which carries the float32 rounding of save_mean itself (half an ulp of 1000 is 3e-5) times
    sum g."""
    inp = R.inputs(sum(c), c, mean=1000.0)
    _check_both(device, inp, c, 1, "mean 1000 " + R.case_id(c))


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_input_scale(device, scale):
    c = R.CASES[3]
    inp = R.inputs(11, c, scale=scale)   # 1e-3: the variance (1e-6) is below eps
    _check_both(device, inp, c, 1, "scale %g" % scale)


@pytest.mark.parametrize("c", [R.CASES[4], R.CASES[6], R.CASES[7]], ids=R.case_id)
def test_two_calls_are_bit_identical(device, c):
    inp = R.inputs(5, c)
    a, b = _both(device, inp, c, 1), _both(device, inp, c, 1)
    for p, q in ((a[0][0], b[0][0]), (a[1], b[1])):
        for name in p:
            assert torch.equal(p[name], q[name]), name


@pytest.mark.parametrize("c", [R.CASES[2], R.CASES[5], R.CASES[6], R.CASES[7]], ids=R.case_id)
def test_null_outputs_and_guard_bands(device, c):
    inp = R.inputs(6, c)
    full_f, full_b = _both(device, inp, c, 1)
    # the outputs that are asked for do not depend on the ones that are not
    for need_x, need_g, need_b in ((False, True, True), (True, False, False), (False, False, True), (True, True, False)):
        gx, gg, gb = hip.group_norm_backward(R.nhwc(inp.x).to(device), R.nhwc(inp.go).to(device), c.G, full_f[2], full_f[3],
                                             gamma=inp.gamma.to(device), y=full_f[1], need_x_grad=need_x, need_gamma_grad=need_g,
                                             need_beta_grad=need_b)
        assert (gx is None) == (not need_x) and (gg is None) == (not need_g) and (gb is None) == (not need_b)
        assert gx is None or torch.equal(R.nchw(gx).cpu(), full_b["grad_x"])
        assert gg is None or torch.equal(gg.cpu(), full_b["grad_gamma"])
        assert gb is None or torch.equal(gb.cpu(), full_b["grad_beta"])
    # through the C ABI with every output inside a canary buffer: the guard bands on both sides stay as they were
    L = hip.lib()
    n, K = c.B * c.H * c.W * c.C, 1024
    geo = tuple(c)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, go = (R.nhwc(t).to(device) for t in (inp.x, inp.go))
    gamma, beta = inp.gamma.to(device), inp.beta.to(device)
    nbytes = L.cp_groupnorm_workspace_bytes(*geo)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    big = [torch.full((n + 2 * K,), 7.25, device=device) for _ in range(2)]              # y, grad_x
    stat = [torch.full((c.B * c.G + 2 * K,), 7.25, device=device) for _ in range(2)]     # save_mean, save_invstd
    vec = [torch.full((c.C + 2 * K,), 7.25, device=device) for _ in range(2)]            # grad_gamma, grad_beta
    rc = L.cp_groupnorm_forward_nhwc(stream, p(x), p(gamma), p(beta), p(big[0], K), p(stat[0], K), p(stat[1], K), *geo, R.EPS, 1,
                                     p(ws), nbytes)
    assert rc == 0, L.cp_last_error()
    rc = L.cp_groupnorm_backward_nhwc(stream, p(x), p(big[0], K), p(go), p(gamma), p(stat[0], K), p(stat[1], K), p(big[1], K),
                                      p(vec[0], K), p(vec[1], K), *geo, p(ws), nbytes)
    assert rc == 0, L.cp_last_error()
    torch.cuda.synchronize()
    for t in big + stat + vec:
        assert bool((t[:K] == 7.25).all()) and bool((t[-K:] == 7.25).all())
    assert torch.equal(big[0][K:-K].view(c.B, c.H, c.W, c.C), full_f[1])
    assert torch.equal(stat[0][K:-K].view(c.B, c.G), full_f[2]) and torch.equal(stat[1][K:-K].view(c.B, c.G), full_f[3])
    assert torch.equal(R.nchw(big[1][K:-K].view(c.B, c.H, c.W, c.C)).cpu(), full_b["grad_x"])
    assert torch.equal(vec[0][K:-K].cpu(), full_b["grad_gamma"]) and torch.equal(vec[1][K:-K].cpu(), full_b["grad_beta"])
    # a backward with every output NULL launches nothing and touches nothing
    rc = L.cp_groupnorm_backward_nhwc(stream, p(x), p(big[0], K), p(go), p(gamma), p(stat[0], K), p(stat[1], K), None, None, None,
                                      *geo, p(ws), nbytes)
    assert rc == 0, L.cp_last_error()


@pytest.mark.parametrize("cfg", [dict(G=32, C=64), dict(G=4, C=16), dict(G=2, C=40, affine=False)],
                         ids=lambda d: "_".join("%s=%s" % kv for kv in d.items()))
def test_module_and_function_against_nn_groupnorm(device, cfg):
    cfg = dict(cfg)
    G, C = cfg.pop("G"), cfg.pop("C")
    shape = (3, C, 9, 11)
    g = torch.Generator().manual_seed(17)
    for channels_last in (False, True):
        for relu in (False, True):
            for x_grad in (True, False):
                what = "G%d C%d %s cl=%d relu=%d xgrad=%d" % (G, C, cfg, channels_last, relu, x_grad)
                ref = nn.GroupNorm(G, C, **cfg).double()
                if ref.affine:
                    with torch.no_grad():
                        ref.weight.copy_(1 + 0.5 * torch.randn(C, generator=g))
                        ref.bias.copy_(torch.randn(C, generator=g))
                ours = copy.deepcopy(ref).float().to(device)
                assert group_norm.use_hip_group_norms(ours) == ([""], {}) and type(ours) is group_norm.GroupNorm
                ours.relu = relu
                x, go = (torch.randn(shape, generator=g) for _ in range(2))
                xd = x.to(device)
                if channels_last:
                    xd = xd.contiguous(memory_format=torch.channels_last)
                xd.requires_grad_(x_grad)
                y = ours(xd)
                assert y.shape == shape and y.is_contiguous(memory_format=torch.channels_last), what
                if y.requires_grad:
                    y.backward(go.to(device))
                x64 = x.double().requires_grad_(True)
                pre = ref(x64)
                gate = (y.detach().cpu() > 0).double() if relu else torch.ones(shape, dtype=torch.float64)
                (pre * gate).backward(go.double())   # the ReLU with the device's gate (tests/groupnorm_ref.py)
                got = dict(y=y.detach().cpu(), grad_x=xd.grad.cpu() if x_grad else None)
                exp = dict(y=torch.relu(pre.detach()) if relu else pre.detach(), grad_x=x64.grad if x_grad else None)
                assert (xd.grad is None) == (not x_grad), what
                if ref.affine:
                    got.update(grad_gamma=ours.weight.grad.cpu(), grad_beta=ours.bias.grad.cpu())
                    exp.update(grad_gamma=ref.weight.grad, grad_beta=ref.bias.grad)
                R.check(got, exp, what)
    # the functional form on the same kernels
    x = torch.randn(shape, generator=g)
    xd = x.to(device).requires_grad_(True)
    y = group_norm.group_norm(xd, G, None, None)
    R.check(dict(y=y.detach().cpu()), dict(y=torch.nn.functional.group_norm(x.double(), G)), "functional")
    with pytest.raises(RuntimeError, match="float32"):
        group_norm.group_norm(xd.double(), G, None, None)
    with pytest.raises(RuntimeError, match="per group"):
        group_norm.group_norm(torch.zeros(1, 48, 4, 4, device=device), 16, None, None)


class _Head(nn.Module):
    """A dlav1-shaped head on a small tree: conv3x3 -> GroupNorm -> ReLU -> conv1x1"""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(32, 64, 3, padding=1, bias=False)
        self.gn = nn.GroupNorm(32, 64)
        self.act = nn.ReLU()
        self.out = nn.Conv2d(64, 8, 1)

    def forward(self, x):
        return self.out(self.act(self.gn(self.conv(x))))


def test_head_sgd_step_on_hip_convs_and_group_norms(device):
    hip.set_default_precision("f32")
    torch.manual_seed(2)
    ref = _Head().double()
    with torch.no_grad():
        ref.gn.bias.add_(4.0)   # gate flips at the ReLU are a property of the graph, not of the kernels
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 32, 24, 20, generator=g)
    target = torch.randn(4, 8, 24, 20, generator=g)
    lr = 0.1
    dnet = copy.deepcopy(ref).float().to(device)
    params = dict(dnet.named_parameters())
    assert conv.use_hip_convs(dnet) == (["conv", "out"], {})
    assert group_norm.use_hip_group_norms(dnet) == (["gn"], {})
    dnet.gn.relu, dnet.act = True, nn.Identity()
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
        print("%s: grad err %.3g, max |ref| %.3g" % (n, err, float(gc.abs().max())))
        assert scale > 0 and err <= 1e-3 * scale, n
        stepped = p0[n] - lr * gc
        assert float((params[n].detach().cpu().double() - stepped).abs().max()) <= 1e-3 * lr * scale + 1e-6, n
