"""The f16x3 DCNv2 backward, CPU side (no device): the premises of the exactness tests of tests/test_dcn_backward_f16x3_gpu.py
on the float64 reference alone, the mask and workspace queries of cp_dcnv2_backward_prec over fast and non-fast shapes, its
refusals that need no launch, and resolve_deterministic beside the precision argument."""
import ctypes
import inspect

import pytest
import torch

from centerpose_amd import hip
from tests import dcn_backward_f16x3_cases as F
from tests import dcn_det_cases as D

CP = F.CP
F32, F16X3 = hip.PRECISIONS["f32"], hip.PRECISIONS["f16x3"]


@pytest.fixture(scope="module")
def built():
    L = hip.lib()
    for name in ("cp_dcnv2_backward_prec_workspace_bytes", "cp_dcnv2_backward_prec", "cp_dcnv2_backward_prec_mask"):
        assert hasattr(L, name), name
    return L


# ---- the premises of the dyadic tests ----
@pytest.mark.parametrize("lo", (None,) + F.LO_OPERANDS, ids=lambda v: v or "one-level")
@pytest.mark.parametrize("shape", F.SHAPES, ids=F.shape_id)
def test_dyadic_reference_is_float32_and_every_partial_sum_fits(shape, lo):
    args, exp = F.reference("dyadic", shape, lo)
    for name, e in zip(F.NAMES, exp):
        assert torch.equal(e.float().double(), e), "%s does not round-trip through float32" % name
        assert float(e.abs().max()) > 0, name
    for name, bound, unit, e in zip(F.NAMES, F.abs_bounds(*args), F.dyadic_units(lo), exp):
        scaled = e * 2.0 ** -unit
        assert torch.equal(scaled, scaled.round()), "%s is not a multiple of 2^%d" % (name, unit)
        assert bound * 2.0 ** -unit < 2 ** 24, "%s: a partial sum may need %.1f bits" % (name, torch.tensor(bound * 2.0 ** -unit).log2())
    x, w, b, off, mask, go = args
    assert torch.equal(off * 2, (off * 2).round()) and set((mask * 4).flatten().tolist()) <= {1.0, 2.0, 3.0, 4.0}
    # some samples leave (-1, H) x (-1, W), some land on its border
    B, C, H, W, Co = shape
    ho = torch.arange(H).view(1, 1, H, 1).float()
    sy = torch.stack([ho - 1 + t // 3 + off[:, 2 * t:2 * t + 1] for t in range(9)])
    assert bool((sy <= -1).any()) and bool((sy >= H).any()) and bool((sy == H - 1).any()) and bool((sy == -0.5).any())
    if lo:  # the operand has a non-zero second level: hi alone cannot hold it
        t = {"w": w, "go": go, "x": x}[lo]
        assert bool(((t * 4096) % 4096 != 0).any()) and bool((t.abs() >= 1).any())
        assert torch.equal(t.half().float(), t) is False


# ---- the queries ----
def _q(L, shape, geo, det, prec):
    return L.cp_dcnv2_backward_prec_workspace_bytes(*shape, *geo, det, prec)


def _mask(L, shape, geo, det, prec):
    return L.cp_dcnv2_backward_prec_mask(*shape, *geo, det, prec)


@pytest.mark.parametrize("shape", F.SHAPES + [F.CHUNKED] + D.PARITY_SHAPES, ids=F.shape_id)
def test_fast_shapes(built, shape):
    for det, old in ((0, built.cp_dcnv2_backward_workspace_bytes), (1, built.cp_dcnv2_backward_det_workspace_bytes)):
        f32 = _q(built, shape, CP, det, F32)
        assert f32 == old(*shape, *CP) > 0
        assert _mask(built, shape, CP, det, F32) == 0
        assert _mask(built, shape, CP, det, F16X3) == 3
        assert _q(built, shape, CP, det, F16X3) >= f32


def test_workspace_is_at_least_the_float32_one_over_a_sweep(built):
    for C in (16, 32, 64, 128, 256):
        for Co in (16, 24, 64, 256):
            for B, H in ((1, 8), (4, 32), (16, 128), (3, 200)):
                for det in (0, 1):
                    s = (B, C, H, H, Co)
                    assert _q(built, s, CP, det, F16X3) >= _q(built, s, CP, det, F32) > 0, (s, det)
                    assert _mask(built, s, CP, det, F16X3) & 1


@pytest.mark.parametrize("name", sorted(D.NON_FAST))
def test_generic_shapes(built, name):
    C, H, W, Co, geo = D.NON_FAST[name]
    shape = (2, C, H, W, Co)
    assert _mask(built, shape, geo, 0, F16X3) == 0 and _mask(built, shape, geo, 0, F32) == 0
    assert _q(built, shape, geo, 0, F16X3) == _q(built, shape, geo, 0, F32) == built.cp_dcnv2_backward_workspace_bytes(*shape, *geo) > 0
    # a deterministic request outside the fast geometry is refused as cp_dcnv2_backward_det refuses it
    assert _q(built, shape, geo, 1, F16X3) == built.cp_dcnv2_backward_det_workspace_bytes(*shape, *geo) == 0
    assert _mask(built, shape, geo, 1, F16X3) == hip.CP_ERR_INVALID
    assert b"outside the deterministic path" in built.cp_last_error()


def _call(L, shape, geo, det, prec, ws_bytes):
    fake = [ctypes.c_void_p(4096)] * 11
    return L.cp_dcnv2_backward_prec(ctypes.c_void_p(0), *fake[:10], *shape, *geo, det, prec, fake[10], ws_bytes)


def test_refusals_before_any_launch(built):
    shape = F.SHAPES[0]
    for det in (0, 1):
        assert _call(built, shape, CP, det, 7, 1 << 40) == hip.CP_ERR_INVALID
        assert b"unknown precision" in built.cp_last_error()
        assert _q(built, shape, CP, det, 7) == 0 and b"unknown precision" in built.cp_last_error()
        assert _mask(built, shape, CP, det, 7) == hip.CP_ERR_INVALID and b"unknown precision" in built.cp_last_error()
        for prec in (F32, F16X3):
            need = _q(built, shape, CP, det, prec)
            assert _call(built, shape, CP, det, prec, need - 1) == hip.CP_ERR_INVALID
            assert b"workspace too small" in built.cp_last_error()
    C, H, W, Co, geo = D.NON_FAST["two_groups"]
    assert _call(built, (1, C, H, W, Co), geo, 1, F16X3, 1 << 40) == hip.CP_ERR_INVALID
    assert b"deformable_group 2" in built.cp_last_error()
    assert _call(built, (0,) + shape[1:], CP, 0, F16X3, 1 << 40) == hip.CP_ERR_INVALID


# ---- Python ----
def test_python_surface():
    from centerpose_amd.lib.models.networks.DCNv2 import _ext, dcn_v2

    sig = inspect.signature(hip.ops.dcn_v2_backward)
    assert sig.parameters["precision"].default == "f32" and list(sig.parameters)[-1] == "precision"
    assert inspect.signature(_ext.dcn_v2_backward_prec).parameters["precision"].kind is inspect.Parameter.KEYWORD_ONLY
    assert dcn_v2.DCNv2.backward_precision == "f32" and dcn_v2.DCN.backward_precision == "f32"
    assert "backward_precision" not in vars(dcn_v2.DCN)   # inherited
    assert hip.ops.dcn_backward_precision_mask(*F.SHAPES[0]) == 3
    assert hip.ops.dcn_backward_precision_mask(*F.SHAPES[0], precision="f32") == 0
    assert hip.ops.dcn_backward_precision_mask(2, *D.NON_FAST["C24"][:4], *D.NON_FAST["C24"][4]) == 0
    with pytest.raises(ValueError, match="precision must be one of"):
        hip.ops.dcn_backward_precision_mask(*F.SHAPES[0], precision="bf16")
    x = torch.zeros(1, 16, 4, 4)
    with pytest.raises(ValueError, match="precision must be one of"):
        hip.ops.dcn_v2_backward(x, torch.zeros(16, 16, 3, 3), torch.zeros(16), torch.zeros(1, 18, 4, 4), torch.zeros(1, 9, 4, 4),
                                x, *CP, precision="bf16")


def test_set_backward_precision_walks_dcn_layers_only():
    from torch import nn

    from centerpose_amd import conv
    from centerpose_amd.lib.models.networks.DCNv2 import dcn_v2

    net = nn.Sequential(dcn_v2.DCN(16, 16, 3, 1, 1), nn.Sequential(dcn_v2.DCNv2(16, 8, 3, 1, 1)), nn.Conv2d(16, 16, 3, 1, 1))
    conv.use_hip_convs(net)
    assert dcn_v2.set_backward_precision(net, "f16x3") == 2
    assert net[0].backward_precision == net[1][0].backward_precision == "f16x3"
    assert net[0].conv_offset_mask.backward_precision == net[2].backward_precision == "f32"   # the two switches are not coupled
    assert conv.set_backward_precision(net, "f16x3") == 2 and net[0].backward_precision == "f16x3"
    assert dcn_v2.set_backward_precision(net, "f32") == 2 and net[0].conv_offset_mask.backward_precision == "f16x3"
    with pytest.raises(ValueError, match="backward_precision must be one of"):
        dcn_v2.set_backward_precision(net, "fp16")
    assert dcn_v2.DCNv2.backward_precision == "f32" and "backward_precision" in vars(net[0])
    with pytest.raises(ValueError, match="backward_precision must be one of"):
        dcn_v2.dcn_v2_conv(torch.zeros(1, 16, 4, 4), torch.zeros(1, 18, 4, 4), torch.zeros(1, 9, 4, 4), net[0].weight, net[0].bias,
                           1, 1, 1, 1, "fp16")


def test_resolve_deterministic_beside_the_precision(monkeypatch):
    """The deterministic resolution is what it was, whatever the precision: the precision only chooses the entry point."""
    seen = []

    class _Reached(Exception):
        pass

    def record(requested, fast, own_flag, *rest):
        seen.append((requested, fast, own_flag))
        raise _Reached()

    monkeypatch.setattr(hip._abi, "lib", lambda: None)
    monkeypatch.setattr(hip._abi, "_dev", lambda t: t)
    monkeypatch.setattr(hip.ops, "resolve_deterministic", record)
    B, C, Co, H, W = 1, 16, 4, 5, 6
    args = (torch.zeros(B, C, H, W), torch.zeros(Co, C, 3, 3), torch.zeros(Co), torch.zeros(B, 18, H, W), torch.zeros(B, 9, H, W),
            torch.zeros(B, Co, H, W), *CP)
    for prec in ("f32", "f16x3"):
        for det in (None, True, False):
            with pytest.raises(_Reached):
                hip.ops.dcn_v2_backward(*args, deterministic=det, precision=prec)
    assert seen == [(d, True, False) for _ in range(2) for d in (None, True, False)]
    for requested, fast, own, torch_flag, want in ((None, True, False, False, False), (True, True, False, False, True),
                                                   (None, True, True, False, True), (None, True, False, True, True)):
        assert hip.resolve_deterministic(requested, fast, own, torch_flag, False) == (want, False)
    with pytest.raises(RuntimeError, match="does not have a deterministic implementation"):
        hip.resolve_deterministic(True, False, False, False, False)
