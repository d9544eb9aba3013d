"""CPU tests (no GPU) of the f16x3 mode of the ConvTranspose2d backward: the premises of tests/deconv_backward_f16x3_cases.py,
the host arithmetic of the *_prec entries (mask, workspace) and their refusals, and the parity of the plain entries with the
*_prec entries at CP_PREC_F32 -- the same return value and the same cp_last_error() bytes over the refused geometries, the null
arguments, a misaligned pointer and a short workspace, as tests/test_backward_entry_parity_cpu.py checks for the other three
operators.  Nothing launches: every refusal comes before the first use of a pointer."""
import ctypes

import pytest
import torch
from torch import nn

import __graft_entry__ as ge
from centerpose_amd import deconv, hip
from tests import deconv_backward_f16x3_cases as C
from tests import deconv_backward_ref as R
from tests import f16x3_common as X

F32, F16X3 = hip.PRECISIONS["f32"], hip.PRECISIONS["f16x3"]
P = ctypes.c_void_p(0x1000)     # never dereferenced

# tests/test_deconv_backward_cpu.py's refused geometries
REFUSED = [((0, 8, 8, 16, 16, 4, 2, 1, 16), b"at least 1"), ((2, 0, 8, 16, 16, 4, 2, 1, 16), b"at least 1"),
           ((2, 8, 0, 32, 32, 4, 2, 1, 1), b"at least 1"), ((2, 8, 8, 16, 16, 4, 2, 1, 2), b"unsupported geometry"),
           ((2, 8, 8, 16, 16, 2, 2, 0, 16), b"unsupported geometry"), ((2, 8, 8, 16, 16, 4, 2, 0, 16), b"unsupported geometry"),
           ((2, 8, 8, 16, 16, 16, 8, 4, 16), b"unsupported geometry"), ((2, 8, 8, 6, 6, 4, 2, 1, 6), b"unsupported geometry"),
           ((2, 8, 8, 0, 0, 4, 2, 1, 0), b"unsupported geometry"), ((2, 8, 8, 964, 964, 4, 2, 1, 964), b"unsupported geometry"),
           ((2, 8, 8, 32, 32, 3, 2, 1, 1), b"unsupported geometry"), ((2, 8, 8, 32, 32, 4, 1, 1, 1), b"unsupported geometry"),
           ((2, 8, 8, 48, 32, 4, 2, 1, 1), b"unsupported geometry"), ((2, 8, 8, 32, 16, 4, 2, 1, 1), b"unsupported geometry"),
           ((64, 512, 512, 32, 32, 4, 2, 1, 1), b"2^31 elements"), ((1, 4096, 4096, 32, 32, 4, 2, 1, 1), b"2^31 elements"),
           ((64, 512, 512, 64, 64, 4, 2, 1, 64), b"elements or more")]
OK = [(2, 8, 8, 64, 32, 4, 2, 1, 1), (2, 8, 8, 64, 64, 4, 2, 1, 64)]   # dense, depth-wise


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def test_case_premises():
    assert [(c.B, c.Cin, c.Cout, c.H, c.W) for c in C.CASES[:4]] == [(2, 256, 256, 2, 3), (1, 64, 32, 5, 7), (2, 32, 96, 8, 8),
                                                                      (3, 128, 64, 3, 17)]
    assert all(c.K == 4 and c.stride == 2 and c.pad == 1 and c.groups == 1 for c in C.CASES)
    assert max(C.wgrad_plan(c)[2] for c in C.CASES) >= 9      # more slabs than the slab sum has lanes
    assert len(C.TWO_LEVEL_CASES) == 4 and C.CASES[0] not in C.TWO_LEVEL_CASES
    for c in C.TWO_LEVEL_CASES:
        assert c.B * c.H * c.W <= X.TWO_LEVEL_MAX_SUM and 16 * c.Cout <= X.TWO_LEVEL_MAX_SUM
    # dyadic sums are integers far below 2^24
    assert max(max(c.B * c.H * c.W, 16 * c.Cout) for c in C.CASES) < 2 ** 24
    # two-level inputs are two-level values, and a wrong result would show: both levels occur
    inp = C.cached_inputs("two_xw", 5, C.CASES[1])
    assert set(inp.x.double().unique().tolist()) <= set(X.TWO_LEVEL_VALUES) and len(inp.x.unique()) == 9
    assert set(inp.go.unique().tolist()) == {-1.0, 0.0, 1.0}
    inp = C.cached_inputs("two_go", 5, C.CASES[1])
    assert len(inp.go.unique()) == 9 and set(inp.w.unique().tolist()) == {-1.0, 0.0, 1.0}
    # the float64 reference of such inputs is representable in float32 (the exactness claim is about float32 outputs)
    for t in C.cached_reference("two_xw", 5, C.CASES[1]):
        assert torch.equal(t.float().double(), t)


def test_mask_and_workspace(built):
    L = built
    for c in C.CASES:
        geo = R.geo(c)
        assert L.cp_conv_transpose2d_backward_prec_mask(*geo, F16X3) == 3 and L.cp_conv_transpose2d_backward_prec_mask(*geo, F32) == 0
        for nx in (0, 1):
            f32 = L.cp_conv_transpose2d_backward_workspace_bytes(*geo, nx)
            assert L.cp_conv_transpose2d_backward_prec_workspace_bytes(*geo, nx, F32) == f32 > 0
            # at least the two split copies on top of the float32 slabs
            assert L.cp_conv_transpose2d_backward_prec_workspace_bytes(*geo, nx, F16X3) >= f32 * (1 - nx) + 4 * c.B * c.H * c.W * (
                c.Cin + 4 * c.Cout)
        # monotone in B
        sizes = [L.cp_conv_transpose2d_backward_prec_workspace_bytes(b, *geo[1:], 1, F16X3) for b in (1, 2, 3, 5, 8)]
        assert sizes == sorted(sizes)
    for c in (R.DW_CASES[1], R.DW_CASES[4]):
        geo = R.geo(c)
        assert L.cp_conv_transpose2d_backward_prec_mask(*geo, F16X3) == 0
        assert (L.cp_conv_transpose2d_backward_prec_workspace_bytes(*geo, 1, F16X3)
                == L.cp_conv_transpose2d_backward_workspace_bytes(*geo, 1))
    # a grad_out of 0xf0000000 bytes or more: the data gradient stays float32 (32-bit byte offsets), the weight gradient does not
    big = (8, 512, 512, 32, 128, 4, 2, 1, 1)
    assert 8 * 1024 * 1024 * 128 * 4 >= 0xf0000000 and L.cp_conv_transpose2d_backward_prec_mask(*big, F16X3) == 1
    assert hip.ops.conv_transpose2d_backward_precision_mask(2, 2, 3, 256, 256) == 3
    for geo, text in REFUSED:
        assert L.cp_conv_transpose2d_backward_prec_mask(*geo, F16X3) == hip.CP_ERR_INVALID and text in L.cp_last_error()


def _call(fn, geo, tail, x=P, w=P, go=P, gx=P, gw=P, ws=P, nbytes=1 << 40):
    return fn(None, x, w, go, gx, gw, *geo, *tail, ws, nbytes)


def _same(L, old, new):
    """Both thunks start from the same recorded error, one no backward entry emits; returns the common (value, cp_last_error())."""
    seen = []
    for f in (old, new):
        assert L.cp_set_default_precision(-1) == hip.CP_ERR_INVALID and L.cp_last_error() == b"precision must be 0 or 1"
        seen.append((f(), L.cp_last_error()))
    assert seen[0] == seen[1], seen
    return seen[0]


def test_plain_entries_are_the_prec_entries_at_f32(built):
    L = built
    old_q, new_q, old, new = (L.cp_conv_transpose2d_backward_workspace_bytes, L.cp_conv_transpose2d_backward_prec_workspace_bytes,
                              L.cp_conv_transpose2d_backward_nhwc, L.cp_conv_transpose2d_backward_prec_nhwc)
    for geo, text in REFUSED:
        for nx in (0, 1):
            v, e = _same(L, lambda: old_q(*geo, nx), lambda: new_q(*geo, nx, F32))
            assert v == 0 and text in e, (geo, e)
        v, e = _same(L, lambda: _call(old, geo, ()), lambda: _call(new, geo, (F32,)))
        assert v == hip.CP_ERR_INVALID and text in e, (geo, e)
    for geo in OK:
        need = [_same(L, lambda: old_q(*geo, nx), lambda: new_q(*geo, nx, F32)) for nx in (0, 1)]
        assert 0 < need[0][0] <= need[1][0] and {e for _, e in need} == {b"precision must be 0 or 1"}   # a success records nothing
        n = need[1][0]
        for kw in (dict(x=None), dict(w=None), dict(go=None), dict(gw=None), dict(ws=None), dict(x=None, gx=None)):
            v, e = _same(L, lambda: _call(old, geo, (), nbytes=n, **kw), lambda: _call(new, geo, (F32,), nbytes=n, **kw))
            assert v == hip.CP_ERR_INVALID and e == b"conv_transpose2d_backward: null argument", kw
        for kw in (dict(x=ctypes.c_void_p(0x1004)), dict(gx=ctypes.c_void_p(0x1008)), dict(ws=ctypes.c_void_p(0x1001))):
            v, e = _same(L, lambda: _call(old, geo, (), nbytes=n, **kw), lambda: _call(new, geo, (F32,), nbytes=n, **kw))
            assert v == hip.CP_ERR_INVALID and e == b"conv_transpose2d_backward: tensors must be 16-byte aligned", kw
        for nbytes in (n - 1, 0):
            v, e = _same(L, lambda: _call(old, geo, (), nbytes=nbytes), lambda: _call(new, geo, (F32,), nbytes=nbytes))
            assert v == hip.CP_ERR_INVALID and e == b"conv_transpose2d_backward: workspace too small", nbytes


def test_precision_argument(built):
    L = built
    text = b"conv_transpose2d_backward: unknown precision (CP_PREC_F32 or CP_PREC_F16X3)"
    for geo in OK:
        for prec in (-1, 2, 7):
            assert L.cp_conv_transpose2d_backward_prec_workspace_bytes(*geo, 1, prec) == 0 and L.cp_last_error() == text
            assert _call(L.cp_conv_transpose2d_backward_prec_nhwc, geo, (prec,)) == hip.CP_ERR_INVALID and L.cp_last_error() == text
            assert L.cp_conv_transpose2d_backward_prec_mask(*geo, prec) == hip.CP_ERR_INVALID and L.cp_last_error() == text
        # the f16x3 workspace is what the f16x3 call asks for: one byte less is refused before any launch
        n = L.cp_conv_transpose2d_backward_prec_workspace_bytes(*geo, 1, F16X3)
        assert _call(L.cp_conv_transpose2d_backward_prec_nhwc, geo, (F16X3,), nbytes=n - 1) == hip.CP_ERR_INVALID
        assert L.cp_last_error() == b"conv_transpose2d_backward: workspace too small"
    # the shape is checked before the precision
    assert L.cp_conv_transpose2d_backward_prec_workspace_bytes(*REFUSED[3][0], 1, 7) == 0 and b"unsupported geometry" in L.cp_last_error()
    c = C.CASES[1]
    inp = C.cached_inputs("dyadic", 1, c)
    with pytest.raises(ValueError, match="precision must be one of"):
        hip.ops.conv_transpose2d_backward(R.nhwc(inp.x), inp.w, R.nhwc(inp.go), 2, 1, 1, precision="f16")
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.ops.conv_transpose2d_backward(R.nhwc(inp.x), inp.w, R.nhwc(inp.go), 2, 1, 1, precision="f16x3")


class _Tree(nn.Module):
    def __init__(self):
        super().__init__()
        self.up = nn.ConvTranspose2d(32, 32, 4, stride=2, padding=1, groups=32, bias=False)
        self.stack = nn.Sequential(nn.ConvTranspose2d(64, 32, 4, stride=2, padding=1, bias=False), nn.ReLU())
        self.biased = nn.ConvTranspose2d(32, 32, 4, stride=2, padding=1)


def test_layer_switches():
    tree = _Tree()
    assert deconv.set_backward_precision(tree, "f16x3") == 0      # nothing is a deconv.ConvTranspose2d yet
    assert deconv.use_hip_deconvs(tree)[0] == ["up", "stack.0"]
    assert tree.up.backward_precision == tree.stack[0].backward_precision == "f32" and not hasattr(tree.biased, "backward_precision")
    assert deconv.set_backward_precision(tree, "f16x3") == 2 and tree.stack[0].backward_precision == "f16x3"
    assert deconv.set_backward_precision(tree.stack, "f32") == 1 and tree.up.backward_precision == "f16x3"
    tree2 = _Tree()
    assert deconv.use_hip_deconvs(tree2, backward_precision="f16x3")[0] == ["up", "stack.0"]
    assert tree2.up.backward_precision == tree2.stack[0].backward_precision == "f16x3"
    assert deconv.ConvTranspose2d(32, 32, 4, 2, 1, bias=False).backward_precision == "f32"
    for bad in ("f16", None, 1):
        with pytest.raises(ValueError, match="backward_precision must be one of"):
            deconv.set_backward_precision(tree, bad)
    fresh = _Tree()
    with pytest.raises(ValueError, match="backward_precision must be one of"):
        deconv.use_hip_deconvs(fresh, backward_precision="f16")
    assert type(fresh.up) is nn.ConvTranspose2d      # refused before anything was re-classed
    x = torch.zeros(1, 64, 2, 2)
    with pytest.raises(ValueError, match="backward_precision must be one of"):
        deconv.conv_transpose2d(x, torch.zeros(64, 32, 4, 4), 2, 1, backward_precision="bf16")
    with pytest.raises(RuntimeError, match="HIP device"):
        deconv.conv_transpose2d(x, torch.zeros(64, 32, 4, 4), 2, 1, backward_precision="f16x3")
