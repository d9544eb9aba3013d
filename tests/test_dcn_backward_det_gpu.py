"""The deterministic DCNv2 backward on the device (pytest -m gpu): cp_dcnv2_backward_det through
hip.dcn_v2_backward(..., deterministic=True) and through the process-wide switches.

What holds with it, and is asserted here: all five gradients are bit-identical from call to call (grad_input included, which
the default call sums with float atomics); an image's grad_input / grad_offset / grad_mask do not depend on the batch it is
in, nor on how the call chunks the batch; the values meet the bound of tests/test_dcn_backward_gpu.py against the same
reference (max abs error <= 1e-4 x max |reference| per gradient)."""
import pytest
import torch
from torch import nn

from centerpose_amd import hip
from tests import dcn_det_cases as D
from tests.test_dcn_backward_gpu import _case, _compare, _expected

pytestmark = pytest.mark.gpu
CP, NAMES = D.CP, D.NAMES


def _run(device, x, w, b, off, mask, go, deterministic=True, **kw):
    return [t.cpu() for t in hip.dcn_v2_backward(*(t.to(device) for t in (x, w, b, off, mask, go)), *CP,
                                                 deterministic=deterministic, **kw)]


def _report(got, exp):
    for name, a, e in zip(NAMES, got, exp):
        print("%s: max err %.3g, max |ref| %.3g" % (name, float((a.double() - e.double()).abs().max()), float(e.abs().max())))


@pytest.mark.parametrize("std", D.PARITY_STDS)
@pytest.mark.parametrize("shape", D.PARITY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_reference(device, shape, std):
    args = _case(*shape, CP, std)
    got, exp = _run(device, *args), _expected(*args, *CP)
    _report(got, exp)
    _compare(got, exp)


def test_integer_positions(device):
    """std 0: every sample sits on a cell, the high corners carry weight 0."""
    args = _case(*D.SMALL, CP, 0.0)
    got, exp = _run(device, *args), _expected(*args, *CP)
    _report(got, exp)
    _compare(got, exp)


def test_zero_masks(device):
    args = _case(*D.SMALL, CP, 1.0, zero_mask=True)
    got = _run(device, *args)
    for t in (got[0], got[1], got[3]):
        assert float(t.abs().max()) == 0.0
    _compare(got, _expected(*args, *CP))


def _assert_identical(runs):
    for k, name in enumerate(NAMES):
        for r in runs[1:]:
            assert torch.equal(runs[0][k], r[k]), name


def test_three_calls_are_bit_identical(device):
    args = _case(*D.REPRO, CP, 2.0, seed=9)
    runs = [_run(device, *args) for _ in range(3)]
    _assert_identical(runs)
    _compare(runs[0], _expected(*args, *CP))


def test_one_cell_receives_every_sample(device):
    """Four cells with 2304 entries each: lists past the 64 and the 512 boundaries (chunks of 512 summed by separate waves
    and added in order).  The reference is checked on the CPU first: finite and non-zero in those cells."""
    args = D.one_cell_case()
    exp = _expected(*args, *CP)
    gi = exp[0].double()
    assert bool(torch.isfinite(gi).all())
    y, x = int(D.ONE_CELL_POS[0]), int(D.ONE_CELL_POS[1])
    hot = torch.zeros_like(gi, dtype=torch.bool)
    hot[:, :, y:y + 2, x:x + 2] = True
    assert float(gi[hot].abs().min()) > 0 and float(gi[~hot].abs().max()) == 0
    runs = [_run(device, *args) for _ in range(3)]
    _assert_identical(runs)
    _report(runs[0], exp)
    _compare(runs[0], exp)
    assert float(runs[0][0][~hot].abs().max()) == 0


def _assert_images_independent(device, args, batch_grads):
    for b in range(args[0].shape[0]):
        x, w, bias, off, mask, go = args
        one = _run(device, x[b:b + 1], w, bias, off[b:b + 1], mask[b:b + 1], go[b:b + 1])
        for k in (0, 1, 2):
            assert torch.equal(batch_grads[k][b], one[k][0]), (NAMES[k], b)


def test_an_image_does_not_depend_on_its_batch(device):
    args = _case(*D.BATCH, CP, 2.0, seed=3)
    _assert_images_independent(device, args, _run(device, *args))


def test_across_grad_col_chunks(device):
    """B = 2 at 512 x 512, C = 16: one image per grad_col chunk.  Each image equals its own B = 1 call bit for bit; all five
    gradients are within the parity bound of the default call (itself tested against the reference)."""
    assert D.plan(*D.CHUNKED).nb == 1 < D.CHUNKED[0]
    args = _case(*D.CHUNKED, CP, 2.0, seed=4)
    got = _run(device, *args)
    _assert_images_independent(device, args, got)
    default = _run(device, *args, deterministic=False)
    _report(got, default)
    _compare(got, default)


def test_workspace_canary(device):
    shape = D.PARITY_SHAPES[0]
    x, w, b, off, mask, go = (t.to(device) for t in _case(*shape, CP, 2.0))
    B, C, H, W, Co = shape
    need = hip.lib().cp_dcnv2_backward_det_workspace_bytes(B, C, H, W, Co, *CP)
    assert need == D.det_workspace_bytes(*shape) and need % 4 == 0
    guard = 1024
    buf = torch.full((need // 4 + guard,), 0x5A5A5A5A, dtype=torch.int32, device=device)
    ws = buf.view(torch.uint8)[:need]
    got = [t.cpu() for t in hip.dcn_v2_backward(x, w, b, off, mask, go, *CP, workspace=ws, deterministic=True)]
    assert bool((buf[need // 4:] == 0x5A5A5A5A).all()), "the call wrote past its queried workspace"
    _assert_identical([got, _run(device, *(t.cpu() for t in (x, w, b, off, mask, go)))])
    with pytest.raises(RuntimeError, match="workspace too small"):
        hip.dcn_v2_backward(x, w, b, off, mask, go, *CP, workspace=ws[:need - 256], deterministic=True)


@pytest.fixture
def flags():
    own = hip.deterministic()
    t, w = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    cd = torch.backends.cudnn.deterministic
    yield
    hip.set_deterministic(own)
    torch.use_deterministic_algorithms(t, warn_only=w)
    torch.backends.cudnn.deterministic = cd


def _net_and_input(device, dcn):
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(8, 64, 3, 1, 1), dcn, nn.Conv2d(64, 4, 3, 1, 1))
    with torch.no_grad():
        net[1].conv_offset_mask.weight.normal_(0, 0.02)
        net[1].conv_offset_mask.bias.normal_(0, 0.5)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 8, 24, 24, generator=g)
    target = torch.randn(2, 4, 24, 24, generator=g)
    return net.to(device), x.to(device), target.to(device)


def _backward(net, x, target):
    """Gradients of the input and of every parameter, from the same state."""
    net.zero_grad(set_to_none=True)
    xi = x.detach().clone().requires_grad_(True)
    loss = ((net(xi) - target) ** 2).mean()
    loss.backward()
    return [xi.grad.detach().clone()] + [p.grad.detach().clone() for p in net.parameters()]


def _assert_two_backwards_identical(net, x, target):
    _backward(net, x, target)   # torch picks its convolution algorithms on the first pass
    a, b = _backward(net, x, target), _backward(net, x, target)
    names = ["input"] + [n for n, _ in net.named_parameters()]
    assert len(a) == len(names) == 9
    for n, u, v in zip(names, a, b):
        assert float(u.abs().max()) > 0, n
        assert torch.equal(u, v), n


def test_autograd_is_bit_identical_under_the_library_switch(device, flags):
    from centerpose_amd.lib.models.networks.DCNv2.dcn_v2 import DCN

    net, x, target = _net_and_input(device, DCN(64, 64, 3, 1, 1))
    hip.set_deterministic(True)
    # The library's switch governs the library's operators.  The three nn.Conv2d of this block are torch's: their weight
    # gradient (torch's convolution backward-weight; it feeds 0.weight, 1.conv_offset_mask.weight and 2.weight) was seen to
    # differ between two passes when torch chose its algorithms freely (0.weight, with the DCN's input gradient and
    # `input` identical), so torch is told to choose deterministic convolution algorithms: its flag, nothing of the DCN's.
    torch.backends.cudnn.deterministic = True
    _assert_two_backwards_identical(net, x, target)


def test_autograd_is_bit_identical_under_torch_flag_alone(device, flags):
    from centerpose_amd.lib.models.networks.DCNv2.dcn_v2 import DCN

    net, x, target = _net_and_input(device, DCN(64, 64, 3, 1, 1))
    assert hip.deterministic() is False
    torch.use_deterministic_algorithms(True)
    _assert_two_backwards_identical(net, x, target)


def test_two_deformable_groups_raise_under_the_flag_and_run_without(device, flags):
    from centerpose_amd.lib.models.networks.DCNv2.dcn_v2 import DCN

    net, x, target = _net_and_input(device, DCN(64, 64, 3, 1, 1, deformable_groups=2))
    grads = _backward(net, x, target)
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    hip.set_deterministic(True)
    with pytest.raises(RuntimeError, match="deformable_group 2"):
        _backward(net, x, target)
