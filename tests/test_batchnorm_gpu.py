"""Training BatchNorm on the device (pytest -m gpu): cp_batchnorm_forward_nhwc / cp_batchnorm_backward_nhwc, norm.batch_norm /
BatchNorm2d and use_hip_norms against F.batch_norm + add + ReLU under float64 CPU autograd (tests/batchnorm_ref.py).
Everything is compared at 1e-4 x max |reference| per output, the project's gradient tolerance (tests/test_conv_backward_gpu.py,
tests/test_dcn_backward_gpu.py).

One output is ill-conditioned by construction and sits closest to that bound: grad_x of the n = 2 case (1,1,2,4).  With two
values per channel grad_x is (g1 - g2) / 2 * eps / (var + eps) * gamma * invstd -- the difference of two O(1) terms that
agree to eps / var -- so the float32 rounding of save_invstd alone (relative 6e-8) moves it by 1.2e-7 * var / eps relative:
1e-2 * var.  A float32 emulation of the kernels' arithmetic and torch's own float32 path both give 6.5e-5 on this case's
inputs."""
import copy
import ctypes

import pytest
import torch
from torch import nn

from centerpose_amd import conv, hip, norm
from tests import batchnorm_ref as R

pytestmark = pytest.mark.gpu
GRID = [(residual, act) for residual in (False, True) for act in (0, 1)]


def _both(device, inp, residual, act, training=True, affine=True):
    fwd = R.device_forward(device, inp, residual, act, training, affine)
    bwd = R.device_backward(device, inp, fwd, residual, act, training, affine)
    return fwd, bwd


def _check_both(device, inp, residual, act, what, training=True, affine=True):
    fwd, bwd = _both(device, inp, residual, act, training, affine)
    R.check(fwd[0], R.reference_forward(inp, residual, act, training, affine), what)
    R.check(bwd, R.reference_backward(inp, residual, fwd[0]["y"] if act else None, training, affine), what)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_forward_training(device, c):
    inp = R.inputs(sum(c), c)
    for residual, act in GRID:
        got = R.device_forward(device, inp, residual, act)[0]
        R.check(got, R.reference_forward(inp, residual, act), "%s res=%d act=%d" % (R.case_id(c), residual, act))


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_backward(device, c):
    inp = R.inputs(sum(c), c)
    for residual, act in GRID:
        fwd, got = _both(device, inp, residual, act)
        exp = R.reference_backward(inp, residual, fwd[0]["y"] if act else None)
        R.check(got, exp, "%s res=%d act=%d" % (R.case_id(c), residual, act))
        if residual and not act:   # nothing gates: grad_residual is grad_out itself
            assert torch.equal(got["grad_residual"], inp.go)


@pytest.mark.parametrize("c", R.LARGE_MEAN_CASES, ids=R.case_id)
def test_large_mean(device, c):
    """x = 1000 + N(0, 1): E[x^2] - mean^2 from raw float32 sums is wrong by tens of per cent here."""
    inp = R.inputs(sum(c), c, mean=1000.0)
    _check_both(device, inp, True, 1, "mean 1000 " + R.case_id(c))


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_input_scale(device, scale):
    c = R.CASES[2]
    inp = R.inputs(11, c, scale=scale)   # 1e-3: the variance (1e-6) is below eps
    _check_both(device, inp, True, 1, "scale %g" % scale)


@pytest.mark.parametrize("c", [R.CASES[1], R.CASES[4], R.CASES[5]], ids=R.case_id)
def test_evaluation_mode(device, c):
    inp = R.inputs(sum(c) + 1, c)
    for residual, act in GRID:
        what = "eval %s res=%d act=%d" % (R.case_id(c), residual, act)
        fwd, bwd = _both(device, inp, residual, act, training=False)
        R.check(fwd[0], R.reference_forward(inp, residual, act, training=False), what)
        R.check(bwd, R.reference_backward(inp, residual, fwd[0]["y"] if act else None, training=False), what)
        # the running pair is read, not written
        assert torch.equal(fwd[0]["running_mean"], inp.rmean) and torch.equal(fwd[0]["running_var"], inp.rvar)


@pytest.mark.parametrize("c", [R.CASES[3], R.CASES[6], R.CASES[7]], ids=R.case_id)
def test_two_calls_are_bit_identical(device, c):
    inp = R.inputs(5, c)
    a, b = _both(device, inp, True, 1), _both(device, inp, True, 1)
    for p, q in ((a[0][0], b[0][0]), (a[1], b[1])):
        for name in p:
            assert torch.equal(p[name], q[name]), name


@pytest.mark.parametrize("c", [R.CASES[3], R.CASES[5], R.CASES[6]], ids=R.case_id)
def test_null_outputs_and_guard_bands(device, c):
    inp = R.inputs(6, c)
    full_f, full_b = _both(device, inp, True, 1)
    # running statistics NULL in training: the same y and saved statistics
    lone = R.device_forward(device, inp, True, 1, running=False)[0]
    for name in lone:
        assert torch.equal(lone[name], full_f[0][name]), name
    # the outputs that are asked for do not depend on the ones that are not
    for need_x, need_g, need_b in ((False, True, True), (True, False, False), (False, False, True), (True, True, False)):
        gx, gr, gg, gb = hip.batch_norm_backward(R.nhwc(inp.x).to(device), R.nhwc(inp.go).to(device), full_f[2], full_f[3],
                                               gamma=inp.gamma.to(device), y=full_f[1], need_x_grad=need_x, need_residual_grad=need_x,
                                               need_gamma_grad=need_g, need_beta_grad=need_b)
        assert (gx is None) == (not need_x) == (gr is None) and (gg is None) == (not need_g) and (gb is None) == (not need_b)
        assert gx is None or (torch.equal(R.nchw(gx).cpu(), full_b["grad_x"]) and torch.equal(R.nchw(gr).cpu(), full_b["grad_residual"]))
        assert gg is None or torch.equal(gg.cpu(), full_b["grad_gamma"])
        assert gb is None or torch.equal(gb.cpu(), full_b["grad_beta"])
    # through the C ABI with every output inside a canary buffer: the guard bands on both sides stay as they were
    L = hip.lib()
    n, G = c.B * c.H * c.W * c.C, 1024
    geo = tuple(c)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, res, go = (R.nhwc(t).to(device) for t in (inp.x, inp.res, inp.go))
    gamma, beta = inp.gamma.to(device), inp.beta.to(device)
    nbytes = L.cp_batchnorm_workspace_bytes(*geo)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    big = [torch.full((n + 2 * G,), 7.25, device=device) for _ in range(3)]      # y, grad_x, grad_residual
    small = [torch.full((c.C + 2 * G,), 7.25, device=device) for _ in range(4)]  # save_mean, save_invstd, grad_gamma, grad_beta
    rc = L.cp_batchnorm_forward_nhwc(stream, p(x), p(gamma), p(beta), p(res), None, None, p(big[0], G), p(small[0], G), p(small[1], G),
                                     *geo, 1, R.MOMENTUM, R.EPS, 1, p(ws), nbytes)
    assert rc == 0, L.cp_last_error()
    rc = L.cp_batchnorm_backward_nhwc(stream, p(x), p(big[0], G), p(go), p(gamma), p(small[0], G), p(small[1], G), p(big[1], G),
                                      p(big[2], G), p(small[2], G), p(small[3], G), *geo, 1, p(ws), nbytes)
    assert rc == 0, L.cp_last_error()
    torch.cuda.synchronize()
    for t in big + small:
        assert bool((t[:G] == 7.25).all()) and bool((t[-G:] == 7.25).all())
    assert torch.equal(big[0][G:-G].view(c.B, c.H, c.W, c.C), full_f[1])
    assert torch.equal(R.nchw(big[1][G:-G].view(c.B, c.H, c.W, c.C)).cpu(), full_b["grad_x"])
    assert torch.equal(small[2][G:-G].cpu(), full_b["grad_gamma"]) and torch.equal(small[3][G:-G].cpu(), full_b["grad_beta"])


CONFIGS = [dict(momentum=0.1), dict(momentum=None), dict(affine=False), dict(track_running_stats=False), dict(momentum=0.1, eval=True)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda d: "_".join("%s=%s" % kv for kv in d.items()))
def test_module_and_function_against_nn_batchnorm2d(device, cfg):
    cfg = dict(cfg)
    evaluate = cfg.pop("eval", False)
    C, shape = 20, (3, 20, 9, 11)
    g = torch.Generator().manual_seed(17)
    for channels_last in (False, True):
        for residual, relu in GRID:
            for x_grad in (True, False):
                what = "%s cl=%d res=%d relu=%d xgrad=%d" % (cfg, channels_last, residual, relu, x_grad)
                ref = nn.BatchNorm2d(C, **cfg).double()
                with torch.no_grad():
                    if ref.affine:
                        ref.weight.copy_(1 + 0.5 * torch.randn(C, generator=g))
                        ref.bias.copy_(torch.randn(C, generator=g))
                    if ref.track_running_stats:
                        ref.running_mean.copy_(torch.randn(C, generator=g))
                        ref.running_var.copy_(0.5 + torch.rand(C, generator=g))
                ours = copy.deepcopy(ref).float().to(device)
                assert norm.use_hip_norms(ours) == ([""], {}) and type(ours) is norm.BatchNorm2d
                ours.relu = bool(relu)
                if evaluate:
                    ref.eval(), ours.eval()
                for step in range(2):
                    x, r, go = (torch.randn(shape, generator=g) for _ in range(3))
                    xd, rd = x.to(device), r.to(device)
                    if channels_last:
                        xd, rd = (t.contiguous(memory_format=torch.channels_last) for t in (xd, rd))
                    xd.requires_grad_(x_grad)
                    rd.requires_grad_(True)
                    ours.zero_grad()
                    y = ours(xd, rd) if residual else ours(xd)
                    assert y.shape == shape and y.is_contiguous(memory_format=torch.channels_last), what
                    if y.requires_grad:   # (affine=False without a differentiable input: nothing to propagate)
                        y.backward(go.to(device))
                    x64, r64 = x.double().requires_grad_(True), r.double().requires_grad_(True)
                    ref.zero_grad()
                    pre = ref(x64) + r64 if residual else ref(x64)
                    gate = (y.detach().cpu() > 0).double() if relu else torch.ones(shape, dtype=torch.float64)
                    (pre * gate).backward(go.double())   # the ReLU with the device's gate (tests/batchnorm_ref.py)
                    got = dict(y=y.detach().cpu(), grad_x=xd.grad.cpu() if x_grad else None,
                               grad_residual=rd.grad.cpu() if residual else None)
                    exp = dict(y=torch.relu(pre.detach()) if relu else pre.detach(), grad_x=x64.grad if x_grad else None,
                               grad_residual=r64.grad if residual else None)
                    assert (xd.grad is None) == (not x_grad) and (rd.grad is None) == (not residual), what
                    if ref.affine:
                        got.update(grad_gamma=ours.weight.grad.cpu(), grad_beta=ours.bias.grad.cpu())
                        exp.update(grad_gamma=ref.weight.grad, grad_beta=ref.bias.grad)
                    if ref.track_running_stats:
                        got.update(running_mean=ours.running_mean.cpu(), running_var=ours.running_var.cpu())
                        exp.update(running_mean=ref.running_mean, running_var=ref.running_var)
                        assert int(ours.num_batches_tracked) == int(ref.num_batches_tracked) == (0 if evaluate else step + 1), what
                    R.check(got, exp, "%s step %d" % (what, step))
    # the functional form on the same kernels
    x = torch.randn(shape, generator=g)
    xd = x.to(device).requires_grad_(True)
    y = norm.batch_norm(xd, None, None, None, None, True, 0.1, 1e-5, relu=False)
    exp = torch.nn.functional.batch_norm(x.double(), None, None, None, None, True, 0.1, 1e-5)
    R.check(dict(y=y.detach().cpu()), dict(y=exp), "functional")
    with pytest.raises(RuntimeError, match="float32"):
        norm.batch_norm(xd.double(), None, None, None, None, True, 0.1, 1e-5)
    with pytest.raises(RuntimeError, match="evaluation needs"):
        norm.batch_norm(xd, None, None, None, None, False, 0.1, 1e-5)


from tests.test_conv_backward_gpu import _Block  # noqa: E402  (the BasicBlock-shaped block of the convolution tests)


class _FusedBlock(_Block):
    """_Block after INTEGRATION.md's three-line edit: bn1.relu = bn2.relu = True, the residual goes into bn2."""

    def forward(self, x):
        res = x if self.project is None else self.project(x)
        out = self.bn1(self.conv1(x))
        return self.bn2(self.conv2(out), res)


@pytest.mark.parametrize("stride", [1, 2])
def test_basic_block_sgd_step_on_hip_convs_and_norms(device, stride):
    hip.set_default_precision("f32")
    torch.manual_seed(stride)
    ref = _Block(64, 64, stride).double()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 64, 32, 32, generator=g)
    target = torch.randn(4, 64, 32 // stride, 32 // stride, generator=g)
    lr = 0.1
    dnet = copy.deepcopy(ref).float().to(device)
    dnet.__class__ = _FusedBlock
    params = dict(dnet.named_parameters())
    converted, skipped = conv.use_hip_convs(dnet)
    assert converted == ["conv1", "conv2"] + (["project"] if stride == 2 else []) and not skipped
    assert norm.use_hip_norms(dnet) == (["bn1", "bn2"], {})
    dnet.bn1.relu = dnet.bn2.relu = True
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
    bufs = dict(dnet.named_buffers())
    for n, b in ref.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(bufs[n]) == int(b) == 1
            continue
        scale = float(b.abs().max())
        err = float((bufs[n].cpu().double() - b).abs().max())
        print("stride %d %s: err %.3g, max |ref| %.3g" % (stride, n, err, scale))
        assert scale > 0 and err <= 1e-4 * scale, n


def test_dcn_followed_by_converted_batchnorm_relu(device):
    """The mirror's DCN(64, 64, 3, 1, 1) -> BatchNorm2d -> ReLU (pose_dla_dcn.py:381, DeformConv) with the normalisation and
    the ReLU on the library, against the same pair on torch."""
    from centerpose_amd.lib.models.networks.DCNv2.dcn_v2 import DCN

    hip.set_default_precision("f32")
    torch.manual_seed(0)
    ref = nn.Sequential(DCN(64, 64, 3, 1, 1), nn.BatchNorm2d(64, momentum=0.1), nn.ReLU())
    with torch.no_grad():
        ref[0].conv_offset_mask.weight.normal_(0, 0.02)
        ref[0].conv_offset_mask.bias.normal_(0, 0.5)
        ref[1].weight.normal_(1, 0.3)
        ref[1].bias.normal_(0, 0.5)
    ref = ref.to(device)
    ours = copy.deepcopy(ref)
    assert norm.use_hip_norms(ours) == (["1"], {}) and type(ours[1]) is norm.BatchNorm2d and type(ref[1]) is nn.BatchNorm2d
    ours[1].relu = True
    ours[2] = nn.Identity()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 64, 24, 24, generator=g).to(device)
    go = torch.randn(2, 64, 24, 24, generator=g).to(device)
    res = []
    for net in (ours, ref):
        xi = x.clone().requires_grad_(True)
        h = net[0](xi)
        h.retain_grad()   # the normalisation's own grad_x
        y = net[2](net[1](h))
        y.backward(go)
        res.append([("out", y.detach()), ("grad_x", xi.grad), ("grad_h", h.grad)] + [(n, p.grad) for n, p in net.named_parameters()] +
                   [(n, b) for n, b in net.named_buffers() if "running" in n])
    # The DCN's bias feeds a training-mode BatchNorm, which removes every per-channel constant: its gradient, the sum of
    # grad_h over a channel's B*H*W values, is zero in exact arithmetic, and what either side holds is the float32 rounding of
    # that sum.  Its 1e-4 is therefore taken against the scale of the sum's operands, max over channels of sum |grad_h|
    # (against max |reference| it would compare two roundings of zero with each other); every other output against max |reference|.
    operands = float(res[1][2][1].abs().sum((0, 2, 3)).max())
    for (n, a), (_, e) in zip(*res):
        scale = operands if n == "0.bias" else float(e.abs().max())
        err = float((a - e).abs().max())
        print("dcn+bn %s: err %.3g, max |ref| %.3g, scale %.3g" % (n, err, float(e.abs().max()), scale))
        assert scale > 0 and err <= 1e-4 * scale, n
