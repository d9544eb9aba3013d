"""The f16x3 DCNv2 backward on the device (pytest -m gpu): cp_dcnv2_backward_prec with CP_PREC_F16X3 through
hip.ops.dcn_v2_backward(..., precision="f16x3"), on the float-atomic path and on the deterministic one.

What is asserted: dyadic inputs give the float64 reference bit for bit, also where one operand needs both binary16 halves (a
dropped hi*lo or lo*hi term cannot); Gaussian inputs, inputs scaled by 1e-6 / 1e3 and masks that are no sigmoid's output stay
within 1e-4 x max |reference| per gradient (the f16x3 convolution backward's bound); the split-binary16 kernels did run
(other bits than float32's, except grad_bias's); gradients are equivariant, bit for bit, under power-of-two scalings of the four
tensors; calls repeat bit for bit; the refusals and the CP_PREC_F32 contract of the entry point; the modules.  Every test first
asserts through the mask query that both contractions of its case run in f16x3.  The references (tests/dcn_backward_ref.py,
backward_f64) are computed once per case and shared."""
import ctypes

import pytest
import torch
from torch import nn

from centerpose_amd import hip
from tests import dcn_backward_f16x3_cases as F
from tests import dcn_det_cases as D

pytestmark = pytest.mark.gpu
CP, NAMES, TOL = F.CP, F.NAMES, F.TOL
PATHS = pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
SHAPES = pytest.mark.parametrize("shape", F.SHAPES, ids=F.shape_id)


def _run(device, args, det, precision="f16x3"):
    x, w, b, off, mask, go = (t.to(device) for t in args)
    if precision == "f16x3":
        assert hip.ops.dcn_backward_precision_mask(*x.shape, w.shape[0], *CP, deterministic=det) == 3
    return [t.cpu() for t in hip.ops.dcn_v2_backward(x, w, b, off, mask, go, *CP, deterministic=det, precision=precision)]


def _assert_equal(got, exp, names=NAMES):
    for name, a, e in zip(NAMES, got, exp):
        if name in names:
            bad = int((a.double() != e.double()).sum())
            assert bad == 0, "%s: %d of %d elements differ, max |diff| %.3g" % (name, bad, a.numel(), float((a.double() - e.double()).abs().max()))


def _assert_close(got, exp, what=""):
    for name, a, err in zip(NAMES, got, F.errors(got, exp)):
        assert bool(torch.isfinite(a).all()), (what, name)
        assert err <= TOL, "%s %s: max err %.3g x max |ref|" % (what, name, err)


# 1, 2
@PATHS
@pytest.mark.parametrize("lo", (None,) + F.LO_OPERANDS, ids=lambda v: v or "one-level")
@SHAPES
def test_dyadic_inputs_are_exact(device, shape, lo, det):
    """All five gradients equal the float64 reference bit for bit -- grad_input on the atomic path too: exact sums have no
    order.  (Premises: tests/test_dcn_backward_f16x3_cpu.py.)"""
    args, exp = F.reference("dyadic", shape, lo)
    _assert_equal(_run(device, args, det), exp)


# 3
@PATHS
@pytest.mark.parametrize("std", F.STDS)
@SHAPES
def test_gaussian_inputs(device, shape, std, det):
    args, exp = F.reference("gaussian", shape, std)
    got, f32 = _run(device, args, det), _run(device, args, det, "f32")
    e16, e32 = F.errors(got, exp), F.errors(f32, exp)
    for name, a, b in zip(NAMES, e16, e32):
        print("%s: f16x3 %.3g, f32 %.3g (x max |ref|)" % (name, a, b))
    assert max(e32) <= TOL, "the float32 mode misses the bound: the case is wrong"
    _assert_close(got, exp)


# 4
@PATHS
@SHAPES
def test_the_other_kernels_ran(device, shape, det):
    args, _ = F.reference("gaussian", shape, 2.0)
    got, f32 = _run(device, args, det), _run(device, args, det, "f32")
    for k in (0, 1, 2, 3):
        assert not torch.equal(got[k], f32[k]), NAMES[k]
    assert torch.equal(got[4], f32[4])


# 5
@PATHS
@pytest.mark.parametrize("factor", [1e-6, 1e3])
@SHAPES
def test_input_range(device, shape, factor, det):
    args, exp = F.reference("range", shape, factor)
    assert float(args[4].min()) < -2.5 and float(args[4].max()) > 2.5
    got, f32 = _run(device, args, det), _run(device, args, det, "f32")
    for name, a, b in zip(NAMES, F.errors(got, exp), F.errors(f32, exp)):
        print("%s: f16x3 %.3g, f32 %.3g (x max |ref|)" % (name, a, b))
    _assert_close(got, exp)


# 6
@PATHS
@pytest.mark.parametrize("pows", F.POW2, ids=lambda p: "_".join(map(str, p)))
@SHAPES
def test_power_of_two_equivariance(device, shape, pows, det):
    """x 2^a, w 2^c, grad_output 2^b, mask 2^m: every gradient scales by the exact power of two of the tensors it contains as
    factors.  The claim is made where the scaled value is finite and above 2^-120 (no overflow, no underflow of the claim
    itself).  On the atomic path grad_input's sum has no fixed order: it is checked to the tolerance."""
    (x, w, b, off, mask, go), _ = F.reference("gaussian", shape, 2.0)
    a, c, bb, m = pows
    base = _run(device, (x, w, b, off, mask, go), det)
    got = _run(device, (x * 2.0 ** a, w * 2.0 ** c, b, off, mask * 2.0 ** m, go * 2.0 ** bb), det)
    for name, g0, g1 in zip(NAMES, base, got):
        p = sum(f * e for f, e in zip(F.POW2_FACTORS[name], (a, c, bb, m)))
        want = g0.double() * 2.0 ** p
        claim = torch.isfinite(want.float()) & ((want.abs() > 2.0 ** -120) | (want == 0))   # (samples outside give exact zeros)
        assert float(claim.float().mean()) > 0.99, name
        if name == "grad_input" and not det:
            assert float((g1.double() - want).abs().max()) <= TOL * float(want.abs().max()), name
        else:
            assert torch.equal(g1.double()[claim], want[claim]), name


# 7
@PATHS
def test_three_calls_are_bit_identical(device, det):
    args, exp = F.reference("gaussian", F.SHAPES[2], 2.0)
    runs = [_run(device, args, det) for _ in range(3)]
    for k, name in enumerate(NAMES):
        if name == "grad_input" and not det:
            continue
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), name
    _assert_close(runs[0], exp)


def test_an_image_agrees_with_its_own_call(device):
    """Deterministic path, B = 3 against three B = 1 calls.  The |max| slots are per call, so the agreement is to the tolerance,
    not to the bit (include/centerpose_hip.h)."""
    (x, w, b, off, mask, go), exp = F.reference("gaussian", F.BATCH, 2.0)
    got = _run(device, (x, w, b, off, mask, go), True)
    for i in range(x.shape[0]):
        one = _run(device, (x[i:i + 1], w, b, off[i:i + 1], mask[i:i + 1], go[i:i + 1]), True)
        for k in (0, 1, 2):
            err = float((got[k][i].double() - one[k][0].double()).abs().max())
            assert err <= TOL * float(exp[k].abs().max()), (NAMES[k], i, err)


def test_across_chunks(device):
    """B = 2 at 512 x 512, C = 16: one image per chunk, so the column buffer is refilled, the second chunk adds to the slabs of
    the first, and the per-call scales serve both.  A float64 reference of this size costs more than the whole file; the
    float32 mode of the same call (tested against the reference where it is affordable, and here to be the parent's bits by the
    CP_PREC_F32 contract) stands in, with the same bound.  Both paths in one test: the inputs are built once."""
    assert D.plan(*F.CHUNKED).nb == 1 < F.CHUNKED[0]
    args = F.gaussian_case(F.CHUNKED, 2.0, seed=4)
    for det in (False, True):
        got, f32 = _run(device, args, det), _run(device, args, det, "f32")
        for name, e in zip(NAMES, F.errors(got, f32)):
            print("%s (%s): %.3g x max |f32|" % (name, "det" if det else "atomic", e))
        _assert_close(got, f32, "det" if det else "atomic")
        assert not torch.equal(got[3], f32[3]) and torch.equal(got[4], f32[4])


# 8
def _raw(device, args, geo, det, prec, short=0, canary=None):
    """cp_dcnv2_backward_prec itself; returns (rc, gradients, queried bytes)."""
    L = hip.lib()
    x, w, b, off, mask, go = (t.to(device).contiguous() for t in args)
    B, C, H, W = x.shape
    Co = w.shape[0]
    grads = [torch.empty_like(t) if canary is None else torch.full_like(t, canary) for t in (x, off, mask, w, b)]
    need = L.cp_dcnv2_backward_prec_workspace_bytes(B, C, H, W, Co, *geo, det, prec)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.cp_dcnv2_backward_prec(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), P(x), P(w), P(off), P(mask), P(go),
                                  *[P(t) for t in grads], B, C, H, W, Co, *geo, det, prec, P(ws), need - short)
    torch.cuda.synchronize()
    return rc, [t.cpu() for t in grads], need


@PATHS
def test_refusals_leave_the_outputs_alone(device, det):
    args, _ = F.reference("gaussian", F.SHAPES[0], 2.0)
    L = hip.lib()
    assert L.cp_dcnv2_backward_prec_mask(*F.SHAPES[0], *CP, int(det), 1) == 3
    rc, grads, need = _raw(device, args, CP, int(det), 1, short=1, canary=7.5)
    assert rc == -1 and b"workspace too small" in L.cp_last_error() and need > 0
    assert all(bool((g == 7.5).all()) for g in grads)
    rc, grads, _ = _raw(device, args, CP, int(det), 7, canary=7.5)
    assert rc == -1 and b"unknown precision" in L.cp_last_error()
    assert all(bool((g == 7.5).all()) for g in grads)


def test_f32_through_the_new_entry_is_the_old_call(device):
    L = hip.lib()
    args, _ = F.reference("gaussian", F.SHAPES[1], 2.0)
    for det, old_q in ((0, L.cp_dcnv2_backward_workspace_bytes), (1, L.cp_dcnv2_backward_det_workspace_bytes)):
        rc, new, need = _raw(device, args, CP, det, 0)
        assert rc == 0 and need == old_q(*F.SHAPES[1], *CP)
        old = [t.cpu() for t in hip.dcn_v2_backward(*(t.to(device) for t in args), *CP, deterministic=bool(det))]
        _assert_equal(new, old, NAMES if det else NAMES[1:])
        assert max(F.errors(new[:1], old[:1])) <= TOL
    # a generic shape: float32 bits in either precision, mask 0, the old workspace
    C, H, W, Co, geo = D.NON_FAST["dilation2"]
    from tests.test_dcn_backward_gpu import _case
    gargs = _case(2, C, H, W, Co, geo, 1.0)
    old = [t.cpu() for t in hip.dcn_v2_backward(*(t.to(device) for t in gargs), *geo)]
    for prec in (0, 1):
        assert L.cp_dcnv2_backward_prec_mask(2, C, H, W, Co, *geo, 0, prec) == 0
        rc, new, need = _raw(device, gargs, geo, 0, prec)
        assert rc == 0 and need == L.cp_dcnv2_backward_workspace_bytes(2, C, H, W, Co, *geo)
        _assert_equal(new, old, NAMES[1:])
        assert max(F.errors(new[:1], old[:1])) <= TOL
    via_ops = [t.cpu() for t in hip.ops.dcn_v2_backward(*(t.to(device) for t in gargs), *geo, precision="f16x3")]
    _assert_equal(via_ops, old, NAMES[1:])


# 9
def _restated(x, w, b, off, mask):
    """the DCNv2 forward in float64 on the CPU (tests/dcn_backward_ref.py), for autograd"""
    from tests.dcn_backward_ref import _forward_f64

    return _forward_f64(x, w, b, off, mask, 3, 3, 1, 1, 1, 1, 1, 1, 1, x.shape[2], x.shape[3])


def _built(kind, C, Co):
    """A DCNv2 that runs its backward in f16x3, set in one of the three ways; returns (module, the functional argument)."""
    from centerpose_amd.lib.models.networks.DCNv2 import dcn_v2

    m = dcn_v2.DCNv2(C, Co, 3, 1, 1)
    if kind == "attribute":
        m.backward_precision = "f16x3"
    elif kind == "walk":
        assert dcn_v2.set_backward_precision(nn.Sequential(nn.Sequential(m)), "f16x3") == 1
    return m, ("f16x3" if kind == "functional" else None)


@pytest.mark.parametrize("kind", ["attribute", "walk", "functional"])
def test_dcnv2_module(device, kind):
    from centerpose_amd.lib.models.networks.DCNv2 import dcn_v2

    shape = F.SHAPES[0]
    B, C, H, W, Co = shape
    assert hip.ops.dcn_backward_precision_mask(*shape) == 3
    for case, exact in (("dyadic", True), ("gaussian", False)):
        (x, w, b, off, mask, go), _ = F.reference(case, shape, None if exact else 2.0)
        m, fn_arg = _built(kind, C, Co)
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
        m = m.to(device)
        leaves = [t.to(device).requires_grad_(True) for t in (x, off, mask)]
        if fn_arg:
            y = dcn_v2.dcn_v2_conv(leaves[0], leaves[1], leaves[2], m.weight, m.bias, 1, 1, 1, 1, fn_arg)
        else:
            y = m(*leaves)
        y.backward(go.to(device))
        got = [leaves[0].grad, leaves[1].grad, leaves[2].grad, m.weight.grad, m.bias.grad]
        want = hip.ops.dcn_v2_backward(*(t.to(device) for t in (x, w, b, off, mask, go)), *CP, precision="f16x3")
        _assert_equal([t.cpu() for t in got], [t.cpu() for t in want], NAMES[1:])
        if exact:
            ref = [t.detach().double().requires_grad_(True) for t in (x, w, b, off, mask)]
            _restated(*ref).backward(go.double())
            _assert_equal([t.cpu() for t in got], [ref[0].grad, ref[3].grad, ref[4].grad, ref[1].grad, ref[2].grad])
        # a layer left at the default gives the old entry's bits
        d = dcn_v2.DCNv2(C, Co, 3, 1, 1)
        with torch.no_grad():
            d.weight.copy_(w)
            d.bias.copy_(b)
        d = d.to(device)
        dl = [t.to(device).requires_grad_(True) for t in (x, off, mask)]
        d(*dl).backward(go.to(device))
        old = hip.dcn_v2_backward(*(t.to(device) for t in (x, w, b, off, mask, go)), *CP)
        _assert_equal([t.cpu() for t in (dl[0].grad, dl[1].grad, dl[2].grad, d.weight.grad, d.bias.grad)], [t.cpu() for t in old], NAMES[1:])
    assert dcn_v2.DCNv2.backward_precision == "f32" and dcn_v2.DCN.backward_precision == "f32"


@pytest.mark.parametrize("kind", ["attribute", "walk"])
def test_dcn_module_with_its_offset_convolution(device, kind):
    """DCN on dyadic inputs: conv_offset_mask has zero weights and a bias of half-integers (offsets) and zeros (mask logits:
    sigmoid(0) = 1/2 exactly), so the whole block is dyadic; the offset convolution runs on the library's float32 Conv2d, whose
    sums have a fixed order and are exact here.  All gradients, conv_offset_mask's included, equal float64 autograd of the
    CPU restatement."""
    from centerpose_amd import conv
    from centerpose_amd.lib.models.networks.DCNv2 import dcn_v2

    shape = F.SHAPES[0]
    B, C, H, W, Co = shape
    (x, w, b, _, _, go), _ = F.reference("dyadic", shape, None)
    g = torch.Generator().manual_seed(3)
    ob = torch.cat([torch.randint(-4, 5, (18,), generator=g).float() / 2, torch.zeros(9)])
    m = dcn_v2.DCN(C, Co, 3, 1, 1)
    conv.use_hip_convs(m)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
        m.conv_offset_mask.bias.copy_(ob)
    if kind == "attribute":
        m.backward_precision = "f16x3"
    else:
        assert dcn_v2.set_backward_precision(nn.Sequential(m), "f16x3") == 1
    assert m.conv_offset_mask.backward_precision == "f32"
    assert hip.ops.dcn_backward_precision_mask(*shape) == 3
    m = m.to(device)
    xi = x.to(device).requires_grad_(True)
    m(xi).backward(go.to(device))
    # float64 restatement
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    cw = torch.zeros(27, C, 3, 3, dtype=torch.float64, requires_grad=True)
    cb = ob.double().requires_grad_(True)
    om = torch.nn.functional.conv2d(xr, cw, cb, 1, 1)
    _restated(xr, wr, br, om[:, :18], torch.sigmoid(om[:, 18:])).backward(go.double())
    got = {"input": xi.grad, "weight": m.weight.grad, "bias": m.bias.grad, "conv_offset_mask.weight": m.conv_offset_mask.weight.grad,
           "conv_offset_mask.bias": m.conv_offset_mask.bias.grad}
    want = {"input": xr.grad, "weight": wr.grad, "bias": br.grad, "conv_offset_mask.weight": cw.grad, "conv_offset_mask.bias": cb.grad}
    for name in got:
        assert float(want[name].abs().max()) > 0, name
        assert torch.equal(got[name].cpu().double(), want[name]), name
    assert dcn_v2.DCN.backward_precision == "f32"
