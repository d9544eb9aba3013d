"""GPU tests of the hourglass merge (centerpose_amd/upsample.py; cp_upsample2_add_nhwc / cp_upsample2_add_backward_nhwc).

Reference: ``up1 + F.interpolate(low, scale_factor=2)`` under CPU autograd in float64.  The bounds are derived, not tuned:
* dyadic inputs (integers in [-2, 2]): the forward and grad_low are EXACT (every sum is a small integer);
* Gaussian inputs: the forward is one float32 addition, so within one rounding, 2^-24 |out| per element; grad_low is three
  float32 additions in a fixed order, (g00 + g01) + (g10 + g11), so within 3 x 2^-24 x (|g00| + |g01| + |g10| + |g11|) per
  element;
* the gradient of up1 is the incoming gradient tensor itself (no kernel, no copy);
* NCHW-contiguous and channels_last inputs give the same bits, and so do two calls.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, H, W, C) of low.  The launch caps its grid at 256 * 16 workgroups of 256 lanes (grid_for in csrc/ewise.hip), one float4
# per lane and trip: the last case has 2 * 64 * 66 * 128 = 1 081 344 float4 of grad_low, above 256 * 16 * 256 = 1 048 576, so
# the backward's grid-stride loop runs twice for some lanes (and the forward's, over four times as many, five times).
CASES = [(1, 1, 1, 4),
         (2, 3, 5, 4),       # lanes cross pixels
         (1, 2, 3, 36),      # a channel count that is not a multiple of a 128-byte line
         (2, 4, 6, 256),
         (1, 5, 7, 384),
         (2, 64, 66, 512)]
EPS = 2.0 ** -24


def _id(t):
    return "B%d_%dx%d_C%d" % t


def _inputs(t, seed, dyadic):
    B, H, W, C = t
    g = torch.Generator().manual_seed(seed)
    draw = (lambda *s: torch.randint(-2, 3, s, generator=g).float()) if dyadic else (lambda *s: torch.randn(*s, generator=g))
    return draw(B, C, 2 * H, 2 * W), draw(B, C, H, W), draw(B, C, 2 * H, 2 * W)   # up1, low, grad_out


def _reference(up1, low, go):
    a, b = up1.double().requires_grad_(True), low.double().requires_grad_(True)
    out = a + F.interpolate(b, scale_factor=2)
    ga, gb = torch.autograd.grad(out, [a, b], go.double())
    return out.detach(), ga, gb


def _device(device, up1, low, go, channels_last):
    from centerpose_amd import upsample

    fmt = torch.channels_last if channels_last else torch.contiguous_format
    a = up1.to(device).contiguous(memory_format=fmt).requires_grad_(True)
    b = low.to(device).contiguous(memory_format=fmt).requires_grad_(True)
    g = go.to(device).contiguous(memory_format=fmt)
    out = upsample.upsample2_add(a, b)
    assert out.is_contiguous(memory_format=torch.channels_last)
    ga, gb = torch.autograd.grad(out, [a, b], g)
    assert ga.data_ptr() == g.data_ptr() and ga.stride() == g.stride()   # the grad_out tensor itself
    assert gb.is_contiguous(memory_format=torch.channels_last)
    return out.detach().cpu(), ga.cpu(), gb.cpu()


@pytest.mark.parametrize("t", CASES, ids=_id)
def test_dyadic_exact(device, t):
    up1, low, go = _inputs(t, 10 + CASES.index(t), True)
    out_ref, ga_ref, gb_ref = _reference(up1, low, go)
    out, ga, gb = _device(device, up1, low, go, True)
    assert torch.equal(out.double(), out_ref) and torch.equal(gb.double(), gb_ref) and torch.equal(ga.double(), ga_ref)


@pytest.mark.parametrize("t", CASES, ids=_id)
def test_gaussian_within_the_rounding_bounds(device, t):
    up1, low, go = _inputs(t, 20 + CASES.index(t), False)
    out_ref, ga_ref, gb_ref = _reference(up1, low, go)
    out, ga, gb = _device(device, up1, low, go, True)
    assert bool(((out.double() - out_ref).abs() <= EPS * out_ref.abs()).all())
    four = F.avg_pool2d(go.double().abs(), 2) * 4   # |g00| + |g01| + |g10| + |g11| per grad_low element
    err = (gb.double() - gb_ref).abs()
    print("%s grad_low: max err / bound %.3f" % (_id(t), float((err / (3 * EPS * four)).max())))
    assert bool((err <= 3 * EPS * four).all())
    assert torch.equal(ga, go)
    # the memory format of the inputs does not change a bit, nor does a second call
    out2, _, gb2 = _device(device, up1, low, go, False)
    out3, _, gb3 = _device(device, up1, low, go, True)
    assert torch.equal(out, out2) and torch.equal(gb, gb2) and torch.equal(out, out3) and torch.equal(gb, gb3)


def test_module_and_unrequested_gradients(device):
    from centerpose_amd import upsample

    up1, low, go = _inputs(CASES[3], 30, False)
    m = upsample.UpsampleAdd().to(device)
    a, b = up1.to(device).requires_grad_(True), low.to(device)
    out = m(a, b)
    out.backward(go.to(device))
    assert torch.equal(a.grad.cpu(), go) and b.grad is None
    with torch.no_grad():
        assert torch.equal(m(a, b), out)
    with pytest.raises(RuntimeError, match="expected"):
        m(a, up1.to(device))
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        m(torch.zeros(1, 6, 4, 4, device=device), torch.zeros(1, 6, 2, 2, device=device))
