"""GPU tests of the training max-pool (centerpose_amd/pool.py over cp_maxpool2d_forward_nhwc / _backward_nhwc).

Max-pooling only selects and copies, so forward and backward must be BITWISE equal to CPU torch float32 -- including which tap
of a tied window receives the gradient (torch: the first maximum in row-major order).  Ties are the normal case in the
network (the pooled tensors are ReLU outputs), so every input here is ``relu(randn)``, all zeros or a constant.
"""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

B = 2
# (kernel, stride, padding) -> sizes H x W: odd sizes (floor drops the last row / column), the smallest output, one window
# per image, several rows of windows
SIZES = {(2, 2, 0): [(7, 9), (2, 2), (8, 8)], (3, 2, 1): [(5, 6), (1, 1)]}
CASES = [(geo, hw, C) for geo, sizes in SIZES.items() for hw in sizes for C in (4, 36)]


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _inputs(kind, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "relu":
        x = torch.relu(torch.randn(B, C, H, W, generator=g))
    elif kind == "zero":
        x = torch.zeros(B, C, H, W)
    else:
        x = torch.full((B, C, H, W), 1.5)
    return x, g


def _reference(x, go, geo):
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, *geo)
    gx, = torch.autograd.grad(y, xr, go)
    return y.detach(), gx


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("kind", ["relu", "zero", "const"])
@pytest.mark.parametrize("geo,hw,C", CASES, ids=_id)
def test_forward_backward_bitwise(device, geo, hw, C, kind, layout):
    from centerpose_amd import pool

    H, W = hw
    x, g = _inputs(kind, C, H, W, 1000 * H + 10 * W + C)
    Ho, Wo = (H + 2 * geo[2] - geo[0]) // 2 + 1, (W + 2 * geo[2] - geo[0]) // 2 + 1
    go = torch.randn(B, C, Ho, Wo, generator=g)
    y_ref, gx_ref = _reference(x, go, geo)
    if kind == "relu" and H * W > 4:
        assert bool((x == 0).any())  # ties exist
    xd = x.to(device)
    if layout == "channels_last":
        xd = xd.contiguous(memory_format=torch.channels_last)
    outs = []
    for _ in range(2):
        xg = xd.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y = pool.max_pool2d(xg, *geo)
        assert Ho * Wo == 1 or y.is_contiguous(memory_format=torch.channels_last)
        gx, = torch.autograd.grad(y, xg, go.to(device))
        outs.append((y.detach().cpu(), gx.cpu()))
    assert tuple(outs[0][0].shape) == tuple(y_ref.shape)
    assert torch.equal(outs[0][0], y_ref)
    assert torch.equal(outs[0][1], gx_ref)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])  # call to call


def test_tie_rule_and_dropped_rows(device):
    """The two facts the backward's tie rule was taken from (CPU torch), on the device: an all-zero 4x4 under (2, 2, 0) sends
    the gradient to the even (row, column) positions; an all-zero 5x5 under (3, 2, 1) to rows and columns {0, 1, 3}.  And the
    row and column that flooring drops get exact zeros."""
    from centerpose_amd import pool

    x = torch.zeros(1, 4, 4, 4, device=device, requires_grad=True)
    pool.max_pool2d(x, 2, 2).sum().backward()
    want = torch.zeros(4, 4)
    want[0::2, 0::2] = 1
    assert torch.equal(x.grad.cpu()[0, 0], want)
    x = torch.zeros(1, 4, 5, 5, device=device, requires_grad=True)
    pool.max_pool2d(x, 3, 2, 1).sum().backward()
    sel = torch.zeros(5)
    sel[[0, 1, 3]] = 1
    assert torch.equal(x.grad.cpu()[0, 0], sel.view(5, 1) * sel.view(1, 5))
    x = torch.relu(torch.randn(2, 8, 7, 9, generator=torch.Generator().manual_seed(3))).to(device).requires_grad_(True)
    pool.max_pool2d(x, 2, 2).sum().backward()
    assert bool((x.grad[:, :, 6, :] == 0).all()) and bool((x.grad[:, :, :, 8] == 0).all())
    assert float(x.grad.sum()) == 2 * 8 * 3 * 4


@pytest.mark.parametrize("C", [4, 36])
def test_empty_output_is_refused(device, C):
    """1 x 5 under (2, 2, 0) has no output row: torch raises, and so does the library (before any launch)."""
    from centerpose_amd import pool

    x = torch.relu(torch.randn(B, C, 1, 5))
    with pytest.raises(RuntimeError):
        F.max_pool2d(x, 2, 2)
    with pytest.raises(RuntimeError, match="empty output"):
        pool.max_pool2d(x.to(device), 2, 2)


def test_refusals(device):
    from centerpose_amd import pool

    x = torch.zeros(1, 4, 8, 8, device=device)
    for args in ((3, 1, 1), (2, 1, 0), (3, 2, 0), (2, 2, 1)):
        with pytest.raises(NotImplementedError, match="geometry"):
            pool.max_pool2d(x, *args)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        pool.max_pool2d(torch.zeros(1, 6, 8, 8, device=device), 2, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        pool.max_pool2d(x.cpu(), 2, 2)


def test_module_and_use_hip_pools(device):
    from centerpose_amd import pool

    g = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randn(B, 8, 13, 10, generator=g))
    ref = nn.Sequential(nn.MaxPool2d(3, stride=2, padding=1), nn.MaxPool2d(2, 2))
    net = nn.Sequential(nn.MaxPool2d(3, stride=2, padding=1), nn.MaxPool2d(2, 2)).to(device)
    converted, skipped = pool.use_hip_pools(net)
    assert converted == ["0", "1"] and skipped == {}
    assert all(type(m) is pool.MaxPool2d for m in net)
    xr = x.clone().requires_grad_(True)
    yr = ref(xr)
    go = torch.randn(yr.shape, generator=g)
    gr, = torch.autograd.grad(yr, xr, go)
    xd = x.to(device).requires_grad_(True)
    yd = net(xd)
    gd, = torch.autograd.grad(yd, xd, go.to(device))
    assert torch.equal(yd.detach().cpu(), yr.detach()) and torch.equal(gd.cpu(), gr)
    direct = pool.MaxPool2d(2, 2)
    assert torch.equal(direct(x.to(device)).cpu(), F.max_pool2d(x, 2, 2))
