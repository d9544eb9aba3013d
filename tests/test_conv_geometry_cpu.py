"""CPU tests (no GPU) of the conv2d geometry sweep: the premise behind the GPU test's zero tolerance
(tests/conv_geometry_cases.py), the one geometry rule of centerpose_amd.conv against the library's (cp_conv2d_backward_path,
host arithmetic), and that every case of the table sits on the generic backward kernels."""
import pytest
import torch
from torch import nn

import __graft_entry__ as ge
from centerpose_amd import conv, hip
from tests import conv_geometry_cases as G


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def test_case_table():
    assert len(set(G.CASES)) == len(G.CASES) >= 28 and len(set(map(G.case_id, G.CASES))) == len(G.CASES)
    for c in G.CASES:
        Ho, Wo = G.out_size(c)
        assert G.in_domain(c) and Ho >= 1 and Wo >= 1, c
    # the groups are what their names say
    assert all(G.f16x3_eligible(c) and G.aligned(c) and c.KH != c.KW for c in G.RECT_F16_CASES)
    assert all(not G.f16x3_eligible(c) and G.aligned(c) and c.KH != c.KW for c in G.RECT_F32_CASES)
    assert all(c.KH == c.KW and G.aligned(c) for c in G.SQUARE_CASES)
    assert all(not G.aligned(c) for c in G.UNALIGNED_CASES)
    assert {c.KH * c.KW > 32 for c in G.UNALIGNED_CASES} == {True, False} == {c.Cin % 16 != 0 for c in G.UNALIGNED_CASES}
    assert all(G.out_size(c) == (1, 1) for c in G.WINDOW_CASES)
    # what the sweep is for: both orientations, even kernels, every stride, pad above k // 2, every N tile of the forward
    assert any(c.KH < c.KW for c in G.CASES) and any(c.KH > c.KW for c in G.CASES)
    assert {c.stride for c in G.CASES} == {1, 2, 3, 4}
    assert any(c.KH % 2 == 0 and c.KW % 2 == 0 for c in G.CASES) and any(c.pad > min(c.KH, c.KW) // 2 for c in G.CASES)
    tile = lambda co: 16 if co <= 16 else 32 if co <= 32 else 128 if co % 128 == 0 else 64
    assert {tile(c.Cout) for c in G.CASES} == {16, 32, 64, 128}
    assert any(c.Cout % tile(c.Cout) for c in G.CASES)


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_premise_holds_and_float32_autograd_is_exact(c):
    Ho, Wo = G.out_size(c)
    for relu in (False, True):
        for has_bias in (False, True):
            inp, r64 = G.dyadic_reference(c, relu, has_bias)   # the generator asserts its premise inside
            assert inp.x.shape == (c.B, c.Cin, c.H, c.W) and inp.w.shape == (c.Cout, c.Cin, c.KH, c.KW)
            assert inp.go.shape == (c.B, c.Cout, Ho, Wo) == inp.y.shape == r64[0].shape
            r32 = G.reference(inp.x, inp.w, inp.bias if has_bias else None, inp.go, c.stride, c.pad, relu, dtype=torch.float32)
            for a, b in zip(r32, r64):
                assert a.dtype == torch.float32 and b.dtype == torch.float64
                assert torch.equal(a.double(), b)
                assert torch.equal(b, b.round()) and float(b.abs().max()) < 2 ** 24
            # a test that compares zeros with zeros checks nothing
            assert all(float(t.abs().max()) > 0 for t in r64)
    _, (out, gx, _, _) = G.dyadic_reference(c, False, True)
    assert bool((out < 0).any()) and bool((out > 0).any())   # the ReLU gates some and passes some
    if c == G.GeoCase(2, 32, 48, 9, 11, 2, 2, 2, 0):
        assert not gx[:, :, -1, :].any() and not gx[:, :, :, -1].any() and bool(gx[:, :, :-1, :-1].any())


def test_python_rule_agrees_with_the_library(built):
    """conv._geometry_refusal accepts exactly what cp_conv2d_backward_path does, inside the domain and all around it."""
    accepted = 0
    for cin in (4, 6, 32):
        for kh in range(9):
            for kw in range(9):
                for stride in range(6):
                    for pad in range(9):
                        ours = conv._geometry_refusal(cin, kh, kw, stride, pad) is None
                        lib = built.cp_conv2d_backward_path(2, 16, 16, cin, 8, kh, kw, stride, pad) >= 0
                        assert ours == lib, (cin, kh, kw, stride, pad)
                        assert ours == G.in_domain(G.GeoCase(2, cin, 8, 16, 16, kh, kw, stride, pad))
                        accepted += ours
    # kernel 1..7 per axis with pad < min(KH, KW): sum of min(kh, kw) = 140 (kh, kw, pad) triples, 4 strides, 2 channel counts
    assert accepted == 140 * 4 * 2
    for cin in (0, -4, 2):
        assert conv._geometry_refusal(cin, 3, 3, 1, 1) and built.cp_conv2d_backward_path(2, 16, 16, cin, 8, 3, 3, 1, 1) < 0
    assert conv._geometry_refusal(32, 3, 3, 1, -1) and built.cp_conv2d_backward_path(2, 16, 16, 32, 8, 3, 3, 1, -1) < 0


def test_module_and_functional_form_share_the_rule():
    for kw in (dict(kernel_size=(8, 3)), dict(kernel_size=3, stride=5), dict(kernel_size=(3, 1), padding=1), dict(kernel_size=2, padding=2)):
        with pytest.raises(NotImplementedError, match="geometry outside"):
            conv.Conv2d(32, 32, **kw)
        assert "geometry outside" in conv.use_hip_convs(nn.Conv2d(32, 32, **kw))[1][""]
    for c in G.CASES:
        m = nn.Conv2d(c.Cin, c.Cout, (c.KH, c.KW), c.stride, c.pad)
        assert conv.use_hip_convs(m) == ([""], {}) and type(m) is conv.Conv2d, c
    # the functional form checks the device and the ranks first, the geometry next; without a device only the order shows
    with pytest.raises(RuntimeError, match="HIP device"):
        conv.conv2d(torch.zeros(1, 32, 9, 9), torch.zeros(8, 32, 9, 9))


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_every_case_is_on_the_generic_backward(built, c):
    assert hip.conv2d_backward_path(c.B, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad) == hip.CONV_BWD_GENERIC
    assert built.cp_conv2d_backward_workspace_bytes(c.B, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad, 1) > 0
