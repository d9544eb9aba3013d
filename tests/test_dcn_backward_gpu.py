"""DCNv2 backward on the device (pytest -m gpu): cp_dcnv2_backward against the reference's own col2im / col2im_coord /
im2col (tests/dcn_backward_ref.py, backward_ref) where oracle/_ref exists, else against the float64 restatement of the same
semantics (backward_f64, which tests/test_dcn_backward_cpu.py checks against the reference).  Tolerance: max abs error
<= 1e-4 x max |reference| per gradient."""
import pytest
import torch
from torch import nn

from centerpose_amd import hip
from oracle import dcn as odcn
from tests import dcn_backward_ref as R

pytestmark = pytest.mark.gpu
NAMES = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")


def _expected(*args):
    return R.backward_ref(*args) if odcn.have_reference() else R.backward_f64(*args)


def _case(B, C, H, W, Co, geo, std, seed=0, zero_mask=False):
    kh, kw, sh, sw, ph, pw, dh, dw, dg = geo
    Ho, Wo = R.out_size(H, W, kh, kw, sh, sw, ph, pw, dh, dw)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, kh, kw, generator=g) / (C * kh * kw) ** 0.5
    b = torch.randn(Co, generator=g)
    off = std * torch.randn(B, dg * 2 * kh * kw, Ho, Wo, generator=g)
    mask = torch.zeros(B, dg * kh * kw, Ho, Wo) if zero_mask else torch.rand(B, dg * kh * kw, Ho, Wo, generator=g)
    go = torch.randn(B, Co, Ho, Wo, generator=g)
    return x, w, b, off, mask, go


def _run(device, x, w, b, off, mask, go, geo):
    return [t.cpu() for t in hip.dcn_v2_backward(*(t.to(device) for t in (x, w, b, off, mask, go)), *geo)]


def _compare(got, exp, tol=1e-4):
    for name, a, e in zip(NAMES, got, exp):
        assert a.shape == e.shape, name
        scale = float(e.abs().max())
        err = float((a.double() - e.double()).abs().max())
        assert err <= tol * scale + 1e-30, "%s: max err %.3g vs max |ref| %.3g" % (name, err, scale)


CP = (3, 3, 1, 1, 1, 1, 1, 1, 1)


@pytest.mark.parametrize("std", [0.5, 2.0, 6.0])
@pytest.mark.parametrize("C,Co,H", [(64, 64, 128), (128, 128, 64), (256, 256, 32), (512, 256, 16)])
def test_fast_path_centerpose_shapes(device, C, Co, H, std):
    args = _case(2, C, H, H, Co, CP, std)
    _compare(_run(device, *args, CP), _expected(*args, *CP))


GENERIC = [
    (2, 2, 4, 4, 2, CP, 2.0, False),                       # testcuda.py's check_gradient_dconv shape
    (1, 8, 9, 11, 5, (5, 5, 1, 1, 2, 2, 1, 1, 1), 1.0, False),
    (2, 6, 7, 10, 4, (1, 3, 1, 1, 0, 1, 1, 1, 1), 1.0, False),
    (2, 8, 12, 13, 7, (3, 3, 2, 2, 1, 1, 1, 1, 1), 1.5, False),   # stride 2, odd H, W, Co % 16 != 0
    (1, 16, 11, 9, 20, (3, 3, 1, 1, 2, 2, 2, 2, 1), 1.0, False),  # dilation 2
    (2, 8, 10, 10, 6, (3, 3, 1, 1, 1, 1, 1, 1, 2), 2.0, False),   # deformable_group 2
    (1, 16, 9, 9, 16, (3, 3, 1, 1, 1, 1, 1, 1, 4), 2.0, False),   # deformable_group 4
    (2, 24, 8, 8, 33, CP, 1.0, False),                            # C % 16 != 0 on 3x3
    (2, 16, 10, 10, 16, CP, 1.0, True),                           # fast path, masks of zero
    (1, 6, 8, 8, 3, (3, 3, 1, 1, 1, 1, 1, 1, 2), 1.0, True),      # generic path, masks of zero
]


@pytest.mark.parametrize("i", range(len(GENERIC)))
def test_generic_path_shapes(device, i):
    B, C, H, W, Co, geo, std, zm = GENERIC[i]
    args = _case(B, C, H, W, Co, geo, std, seed=i, zero_mask=zm)
    got = _run(device, *args, geo)
    exp = _expected(*args, *geo)
    if zm:  # zero masks: no input / offset / weight gradient, a mask gradient all the same
        for t in (got[0], got[1], got[3]):
            assert float(t.abs().max()) == 0.0
    _compare(got, exp)


def test_pad_h_differs_from_pad_w_keeps_reference_quirk(device):
    geo = (3, 3, 1, 1, 2, 1, 1, 1, 1)
    args = _case(2, 4, 8, 9, 3, geo, 1.0, seed=5)
    got = _run(device, *args, geo)
    _compare(got, _expected(*args, *geo))
    fixed = R.backward_f64(*args, *geo, quirk=False)
    assert float((got[0].double() - fixed[0]).abs().max()) > 1e-2 * float(fixed[0].abs().max())


@pytest.mark.parametrize("scale", [1e-6, 1e3])
def test_grad_output_range(device, scale):
    x, w, b, off, mask, go = _case(2, 64, 32, 32, 64, CP, 2.0, seed=7)
    go = go * scale
    _compare(_run(device, x, w, b, off, mask, go, CP), _expected(x, w, b, off, mask, go, *CP))


def test_reproducible_outputs_are_bit_identical(device):
    args = _case(2, 64, 48, 48, 64, CP, 2.0, seed=9)
    runs = [_run(device, *args, CP) for _ in range(3)]
    for k in (1, 2, 3, 4):
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), NAMES[k]
    exp = _expected(*args, *CP)
    for r in runs:
        _compare(r, exp)


def test_workspace_too_small_is_an_error(device):
    x, w, b, off, mask, go = (t.to(device) for t in _case(1, 16, 8, 8, 16, CP, 1.0))
    small = torch.empty(1024, dtype=torch.uint8, device=device)
    with pytest.raises(RuntimeError, match="workspace too small"):
        hip.dcn_v2_backward(x, w, b, off, mask, go, *CP, workspace=small)


class _RefDCN(torch.autograd.Function):
    """The CPU stand-in: the oracle's forward, the reference harness (or its float64 restatement) as backward."""

    @staticmethod
    def forward(ctx, x, off, mask, w, b):
        ctx.save_for_backward(x, off, mask, w, b)
        return odcn.dcn_v2_forward(x, w, b, off, mask, *CP)

    @staticmethod
    def backward(ctx, go):
        x, off, mask, w, b = ctx.saved_tensors
        gi, goff, gm, gw, gb = (t.float() for t in _expected(x, w, b, off, mask, go.contiguous(), *CP))
        return gi, goff, gm, gw, gb


def test_autograd_sgd_step_matches_cpu(device):
    """conv -> DCN(64, 64, 3, 1, 1) -> conv, one SGD step on the device and on the CPU; the DCN's own output under grad mode
    is bit-identical to hip.dcn_v2_forward.  Fails on a forward-only mirror (no grad_fn, _ext.dcn_v2_backward raises)."""
    from centerpose_amd.lib.models.networks.DCNv2.dcn_v2 import DCN

    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(8, 64, 3, 1, 1), DCN(64, 64, 3, 1, 1), nn.Conv2d(64, 4, 3, 1, 1))
    with torch.no_grad():
        net[1].conv_offset_mask.weight.normal_(0, 0.02)
        net[1].conv_offset_mask.bias.normal_(0, 0.5)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 8, 24, 24, generator=g)
    target = torch.randn(2, 4, 24, 24, generator=g)
    cpu = [p.detach().clone() for p in net.parameters()]
    lr = 0.1

    dnet = net.to(device)
    opt = torch.optim.SGD(dnet.parameters(), lr=lr)
    h = dnet[0](x.to(device))
    y = dnet[1](h)
    assert y.grad_fn is not None
    # the forward under grad mode is the inference kernel's output, bit for bit
    from centerpose_amd.lib.models.networks.DCNv2.dcn_v2 import dcn_v2_conv
    hd = h.detach().requires_grad_(True)
    off = (torch.randn(2, 18, 24, 24, generator=g) * 2).to(device).requires_grad_(True)
    m = torch.rand(2, 9, 24, 24, generator=g).to(device).requires_grad_(True)
    yg = dcn_v2_conv(hd, off, m, dnet[1].weight, dnet[1].bias, 1, 1, 1, 1)
    with torch.no_grad():
        fwd = hip.dcn_v2_forward(hd, dnet[1].weight, dnet[1].bias, off, m, *CP)
    assert yg.grad_fn is not None and torch.equal(yg.detach(), fwd)
    loss = ((dnet[2](y) - target.to(device)) ** 2).mean()
    opt.zero_grad()
    loss.backward()
    dev_grads = [p.grad.detach().cpu() for p in dnet.parameters()]
    opt.step()

    # the same step on the CPU
    ps = [p.clone().requires_grad_(True) for p in cpu]
    c0w, c0b, dw_, db_, omw, omb, c2w, c2b = ps
    h = nn.functional.conv2d(x, c0w, c0b, 1, 1)
    om = nn.functional.conv2d(h, omw, omb, 1, 1)
    y = _RefDCN.apply(h, om[:, :18].contiguous(), torch.sigmoid(om[:, 18:]), dw_, db_)
    loss_c = ((nn.functional.conv2d(y, c2w, c2b, 1, 1) - target) ** 2).mean()
    grads = torch.autograd.grad(loss_c, ps)
    names = [n for n, _ in net.named_parameters()]
    assert names == ["0.weight", "0.bias", "1.weight", "1.bias", "1.conv_offset_mask.weight", "1.conv_offset_mask.bias",
                     "2.weight", "2.bias"]
    for n, gd, gc in zip(names, dev_grads, grads):
        assert float(gc.abs().max()) > 0, n
        assert float((gd - gc).abs().max()) <= 1e-3 * float(gc.abs().max()), n
    for n, p, p0, gc in zip(names, dnet.parameters(), cpu, grads):
        stepped = p0 - lr * gc
        assert float((p.detach().cpu() - stepped).abs().max()) <= 1e-3 * lr * float(gc.abs().max()) + 1e-6, n


def test_reference_gradcheck_runs_through_the_shim(device, capsys):
    """testcuda.py:69-97 `check_gradient_dconv`, float32, through dcn_v2_conv.  Its result is recorded, not gated: a float32
    finite difference at eps 1e-3 across a bilinear kink is not a sound gate."""
    from torch.autograd import gradcheck

    from centerpose_amd.lib.models.networks.DCNv2.dcn_v2 import dcn_v2_conv

    torch.manual_seed(0)
    N, inC, inH, inW, outC, kH, kW, dg = 2, 2, 4, 4, 2, 3, 3, 1
    inp = (torch.rand(N, inC, inH, inW, device=device) * 0.01).requires_grad_()
    offset = (torch.randn(N, dg * 2 * kW * kH, inH, inW, device=device) * 2).requires_grad_()
    mask = torch.sigmoid(torch.rand(N, dg * kW * kH, inH, inW, device=device).requires_grad_())
    weight = torch.randn(outC, inC, kH, kW, device=device).requires_grad_()
    bias = torch.rand(outC, device=device).requires_grad_()
    ok = gradcheck(dcn_v2_conv, (inp, offset, mask, weight, bias, 1, 1, 1, dg), eps=1e-3, atol=1e-4, rtol=1e-2,
                   raise_exception=False)
    with capsys.disabled():
        print("\ncheck_gradient_dconv (float32, testcuda.py:69-97): %s" % ok)
    assert isinstance(ok, bool)
