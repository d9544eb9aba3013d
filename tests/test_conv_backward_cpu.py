"""CPU tests (no GPU) of the Conv2d backward: the C ABI's declarations, workspace arithmetic and refusals
(cp_conv2d_backward_*), the Conv2d module and use_hip_convs, and the premise of the dyadic generator the GPU tests rest on
(tests/conv_backward_ref.py)."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import __graft_entry__ as ge
from centerpose_amd import hip
from tests import conv_backward_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_conv2d_backward_workspace_bytes", "cp_conv2d_backward_nhwc")


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def _geo(c):
    return (c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.stride, c.pad)


def test_symbols_declared_exported_and_listed(built):
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    testing = open(os.path.join(REPO, "include", "centerpose_hip_testing.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and hasattr(built, name) and name in hip.exported_symbols(), name
        assert name not in testing
    assert int(re.search(r"#define\s+CP_ABI_VERSION\s+(\d+)", header).group(1)) == 7 == built.cp_abi_version()
    assert built.cp_num_kernel_variants() == 46 and built.cp_num_roles() == 10
    # what the operator replaces is cited where it is declared
    for cite in ("pose_dla_dcn.py:48-62", "dcn_v2.py:118-128", "Root"):
        assert cite in header


def test_workspace_query_is_host_arithmetic(built):
    q = built.cp_conv2d_backward_workspace_bytes
    for c in R.CASES + R.dla34_shapes(64):
        for need_x in (0, 1):
            assert q(*_geo(c), need_x) > 0, c
        assert q(*_geo(c), 1) >= q(*_geo(c), 0)
    assert 0 < q(64, 128, 128, 64, 64, 3, 3, 1, 1, 1) < 512 << 20
    for geo in ((128, 128, 64, 64, 3, 3, 1, 1), (64, 64, 128, 27, 3, 3, 1, 1), (50, 50, 16, 32, 3, 3, 2, 1), (31, 31, 64, 128, 1, 1, 2, 0)):
        sizes = [q(B, *geo, 1) for B in (1, 2, 3, 8, 16, 17, 32, 64)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], geo


def test_refusals_without_a_device(built):
    q, call = built.cp_conv2d_backward_workspace_bytes, built.cp_conv2d_backward_nhwc

    def refused(args, text):
        assert q(*args, 1) == 0
        assert text in built.cp_last_error(), (args, built.cp_last_error())

    ok = (2, 16, 16, 64, 64, 3, 3, 1, 1)
    refused((0,) + ok[1:], b"at least 1")
    refused((2, 0) + ok[2:], b"at least 1")
    refused((2, 16, 0) + ok[3:], b"at least 1")
    refused((2, 16, 16, 64, 0, 3, 3, 1, 1), b"at least 1")
    refused((2, 16, 16, 6, 64, 3, 3, 1, 1), b"Cin must be")
    refused((2, 16, 16, 3, 64, 7, 7, 2, 3), b"Cin must be")
    refused((2, 16, 16, 0, 64, 3, 3, 1, 1), b"Cin must be")
    refused((2, 16, 16, 64, 64, 8, 8, 1, 1), b"unsupported geometry")
    refused((2, 16, 16, 64, 64, 3, 3, 5, 1), b"unsupported geometry")
    refused((2, 16, 16, 64, 64, 3, 3, 1, 3), b"unsupported geometry")
    refused((2, 2, 16, 64, 64, 5, 5, 1, 1), b"empty output")
    refused((2, 16, 1, 64, 64, 3, 3, 1, 0), b"empty output")
    refused((64, 1024, 1024, 64, 64, 3, 3, 1, 1), b"2^31 elements")      # x and grad_out: 2^32 elements
    refused((1, 8192, 8192, 32, 4, 1, 1, 1, 0), b"2^31 elements")        # grad_out staged to 32 channels: 2^31
    # the call itself: refused before any launch (no device is touched; the pointers are never dereferenced)
    p = ctypes.c_void_p(0x1000)
    need = q(*ok, 1)
    assert need > 0

    def bwd(x=p, w=p, y=None, go=p, gx=p, gw=p, gb=p, geo=ok, ws=p, nbytes=need):
        return call(None, x, w, y, go, gx, gw, gb, *geo, ws, nbytes)

    for kw in (dict(x=None), dict(w=None), dict(go=None), dict(gw=None), dict(ws=None)):
        assert bwd(**kw) == -1 and b"null argument" in built.cp_last_error(), kw
    assert bwd(nbytes=need - 1) == -1 and b"workspace too small" in built.cp_last_error()
    assert bwd(nbytes=q(*ok, 0)) == -1 and b"workspace too small" in built.cp_last_error()   # the query without grad_x is smaller
    assert bwd(geo=(2, 16, 16, 6, 64, 3, 3, 1, 1)) == -1 and b"Cin must be" in built.cp_last_error()
    assert bwd(geo=(2, 16, 16, 64, 0, 3, 3, 1, 1)) == -1 and b"at least 1" in built.cp_last_error()
    assert bwd(geo=(2, 2, 2, 64, 64, 5, 5, 1, 0)) == -1 and b"empty output" in built.cp_last_error()
    assert bwd(geo=(64, 1024, 1024, 64, 64, 3, 3, 1, 1)) == -1 and b"2^31 elements" in built.cp_last_error()


def test_no_cpu_path(built):
    from centerpose_amd import conv

    c = R.Case(1, 8, 8, 5, 5, 3, 1, 1)
    inp = R.dyadic_inputs(0, c)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.conv2d_backward(R.nhwc(inp.x), inp.w, R.nhwc(inp.go), stride=1, pad=1)
    with pytest.raises(RuntimeError, match="HIP device"):
        conv.conv2d(inp.x, inp.w, inp.bias, 1, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        conv.Conv2d(8, 8, 3, padding=1)(inp.x)


def test_conv2d_module_is_nn_conv2d_but_for_forward():
    from centerpose_amd import conv

    for args, kwargs in (((64, 27, 3), dict(padding=1)), ((8, 16, 1), dict(stride=2, bias=False)), ((4, 16, 7), dict(stride=1, padding=3))):
        torch.manual_seed(3)
        ours = conv.Conv2d(*args, **kwargs)
        torch.manual_seed(3)
        theirs = nn.Conv2d(*args, **kwargs)
        a, b = ours.state_dict(), theirs.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        assert [n for n, _ in ours.named_parameters()] == [n for n, _ in theirs.named_parameters()]
        assert repr(ours) == repr(theirs) and isinstance(ours, nn.Conv2d) and ours.relu is False
    assert {"forward", "relu"} <= set(vars(conv.Conv2d))
    assert not {"reset_parameters", "_conv_forward", "extra_repr"} & set(vars(conv.Conv2d))
    for bad in (dict(dilation=2), dict(groups=2), dict(padding_mode="reflect"), dict(padding="same"), dict(stride=(1, 2)),
                dict(padding=(1, 0)), dict(in_channels=6)):
        kw = {**dict(in_channels=8, out_channels=8, kernel_size=3, padding=1), **bad}
        with pytest.raises(NotImplementedError):
            conv.Conv2d(**kw)


class _Tree(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(8, 16, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(16)
        self.block = nn.Sequential(nn.Conv2d(16, 16, 1), nn.ReLU(), nn.Conv2d(16, 16, 3, padding=2, dilation=2))
        self.up = nn.ConvTranspose2d(16, 16, 4, stride=2, padding=1, groups=16, bias=False)
        self.depthwise = nn.Conv2d(16, 16, 3, padding=1, groups=16)
        self.stem = nn.Conv2d(3, 8, 7, padding=3)


def test_use_hip_convs_reclasses_in_place():
    from centerpose_amd import conv

    torch.manual_seed(0)
    tree = _Tree()
    params = dict(tree.named_parameters())
    keys = list(tree.state_dict())
    converted, skipped = conv.use_hip_convs(tree)
    assert converted == ["conv1", "block.0"]
    assert sorted(skipped) == ["block.2", "depthwise", "stem", "up"]
    assert "dilation" in skipped["block.2"] and "groups" in skipped["depthwise"] and "ConvTranspose2d" in skipped["up"]
    assert "multiple of 4" in skipped["stem"]
    assert type(tree.conv1) is conv.Conv2d and type(tree.block[0]) is conv.Conv2d
    assert type(tree.block[2]) is nn.Conv2d and type(tree.depthwise) is nn.Conv2d and type(tree.stem) is nn.Conv2d
    assert type(tree.up) is nn.ConvTranspose2d and type(tree.bn1) is nn.BatchNorm2d
    after = dict(tree.named_parameters())
    assert list(after) == list(params) and all(after[k] is params[k] for k in params)
    assert list(tree.state_dict()) == keys
    assert tree.conv1.relu is False
    again, skipped2 = conv.use_hip_convs(tree)
    assert again == [] and skipped2 == skipped
    # a lone convolution is converted too (the root module itself)
    lone = nn.Conv2d(4, 4, 1)
    assert conv.use_hip_convs(lone) == ([""], {}) and type(lone) is conv.Conv2d
    # a subclass keeps its own forward, with this reason; a subclassed transposed convolution is a transposed convolution
    derived, derived_up = _DerivedConv(4, 4, 1), _DerivedUp(4, 4, 2)
    assert conv.use_hip_convs(derived) == ([], {"": "subclass _DerivedConv of nn.Conv2d keeps its own forward"})
    assert conv.use_hip_convs(derived_up) == ([], {"": "ConvTranspose2d is not built"})
    assert type(derived) is _DerivedConv and type(derived_up) is _DerivedUp


class _DerivedConv(nn.Conv2d):
    pass


class _DerivedUp(nn.ConvTranspose2d):
    pass


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_dyadic_generator_premise_holds(c):
    inp = R.dyadic_inputs(sum(c), c)   # asserts inside
    Ho, Wo = R.out_size(c)
    assert inp.x.shape == (c.B, c.Cin, c.H, c.W) and inp.go.shape == (c.B, c.Cout, Ho, Wo) == inp.y.shape
    assert R.is_mfma(c) == (c in R.MFMA_CASES + R.PADDED_CASES)


@pytest.mark.parametrize("i", [1, 5, 8, 10, 15])
def test_float32_and_float64_autograd_agree_on_dyadic_inputs(i):
    c = R.CASES[i]
    inp = R.dyadic_inputs(sum(c), c)
    for y in (None, inp.y):
        g32 = R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, y, dtype=torch.float32)
        g64 = R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, y)
        for a, b in zip(g32, g64):
            assert torch.equal(a.double(), b)
            assert torch.equal(b, b.round()) and float(b.abs().max()) < 2 ** 24
