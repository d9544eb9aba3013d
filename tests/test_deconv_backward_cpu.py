"""CPU tests (no GPU) of the ConvTranspose2d training path: the C ABI's declarations, workspace arithmetic and refusals
(cp_conv_transpose2d_dw_nhwc, cp_conv_transpose2d_backward_*), the deconv.ConvTranspose2d module and use_hip_deconvs."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import __graft_entry__ as ge
from centerpose_amd import conv, deconv, hip, norm
from tests import deconv_backward_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_conv_transpose2d_dw_nhwc", "cp_conv_transpose2d_backward_workspace_bytes", "cp_conv_transpose2d_backward_nhwc")


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


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
    for cite in ("pose_dla_dcn.py:402-417", "resnet_dcn.py:232-240"):
        assert cite in header
    assert "deconv_bwd.hip" in open(os.path.join(REPO, "centerpose_amd", "csrc", "Makefile")).read()


def test_workspace_query_is_host_arithmetic(built):
    q = built.cp_conv_transpose2d_backward_workspace_bytes
    for c in R.DW_CASES + R.DENSE_CASES:
        for need_x in (0, 1):
            assert q(*R.geo(c), need_x) > 0, c
        assert q(*R.geo(c), 0) <= q(*R.geo(c), 1), c
    # the workload's layers at batch 16
    for C, H, f in ((256, 16, 2), (128, 32, 2), (64, 64, 2), (64, 32, 4)):
        assert 0 < q(16, H, H, C, C, 2 * f, f, f // 2, C, 1) < 64 << 20
    for C, H in ((256, 16), (128, 32), (64, 64)):
        assert 0 < q(16, H, H, C, C, 4, 2, 1, 1, 1) < 256 << 20
    for rest in ((1, 1, 4, 4, 4, 2, 1, 4), (7, 9, 20, 20, 4, 2, 1, 20), (33, 31, 64, 64, 8, 4, 2, 64), (64, 64, 64, 64, 4, 2, 1, 64),
                 (16, 16, 256, 256, 4, 2, 1, 256), (1, 1, 32, 32, 4, 2, 1, 1), (13, 11, 64, 96, 4, 2, 1, 1), (64, 64, 64, 64, 4, 2, 1, 1)):
        for need_x in (0, 1):
            sizes = [q(B, *rest, need_x) for B in (1, 2, 3, 8, 16, 17, 32, 64)]
            assert sizes == sorted(sizes) and sizes[0] > 0, rest


def test_refusals_without_a_device(built):
    q, fwd, bwd = (built.cp_conv_transpose2d_backward_workspace_bytes, built.cp_conv_transpose2d_dw_nhwc,
                   built.cp_conv_transpose2d_backward_nhwc)

    def refused(geo, text):
        for need_x in (0, 1):
            assert q(*geo, need_x) == 0
            assert text in built.cp_last_error(), (geo, built.cp_last_error())

    #        B  H  W  Cin Cout K  s  p  groups
    refused((0, 8, 8, 16, 16, 4, 2, 1, 16), b"at least 1")
    refused((2, 0, 8, 16, 16, 4, 2, 1, 16), b"at least 1")
    refused((2, 8, 0, 32, 32, 4, 2, 1, 1), b"at least 1")
    refused((2, 8, 8, 16, 16, 4, 2, 1, 2), b"unsupported geometry")     # grouped, not depth-wise
    refused((2, 8, 8, 16, 16, 2, 2, 0, 16), b"unsupported geometry")    # k = 2 / s = 2
    refused((2, 8, 8, 16, 16, 4, 2, 0, 16), b"unsupported geometry")    # pad != stride / 2
    refused((2, 8, 8, 16, 16, 16, 8, 4, 16), b"unsupported geometry")   # f = 8
    refused((2, 8, 8, 16, 16, 6, 3, 1, 16), b"unsupported geometry")    # f = 3
    refused((2, 8, 8, 6, 6, 4, 2, 1, 6), b"unsupported geometry")       # C % 4
    refused((2, 8, 8, 0, 0, 4, 2, 1, 0), b"unsupported geometry")
    refused((2, 8, 8, 964, 964, 4, 2, 1, 964), b"unsupported geometry")  # the weight table: C <= 960 at stride 2
    refused((2, 8, 8, 244, 244, 8, 4, 2, 244), b"unsupported geometry")  # ... and C <= 240 at stride 4
    refused((2, 8, 8, 32, 32, 3, 2, 1, 1), b"unsupported geometry")     # dense: another kernel
    refused((2, 8, 8, 32, 32, 4, 1, 1, 1), b"unsupported geometry")
    refused((2, 8, 8, 48, 32, 4, 2, 1, 1), b"unsupported geometry")     # dense: channels % 32
    refused((2, 8, 8, 32, 16, 4, 2, 1, 1), b"unsupported geometry")
    refused((64, 512, 512, 32, 32, 4, 2, 1, 1), b"2^31 elements")
    refused((1, 4096, 4096, 32, 32, 4, 2, 1, 1), b"2^31 elements")
    refused((64, 512, 512, 64, 64, 4, 2, 1, 64), b"elements or more")
    assert q(2, 8, 8, 960, 960, 4, 2, 1, 960, 1) > 0 and q(2, 8, 8, 240, 240, 8, 4, 2, 240, 1) > 0
    # the calls themselves: refused before any launch (no device is touched; the pointers are never dereferenced)
    p = ctypes.c_void_p(0x1000)
    for ok in ((2, 8, 8, 16, 16, 4, 2, 1, 16), (2, 8, 8, 32, 64, 4, 2, 1, 1)):
        need = q(*ok, 1)
        assert need > 0

        def b(x=p, w=p, go=p, gx=p, gw=p, geo=ok, ws=p, nbytes=need):
            return bwd(None, x, w, go, gx, gw, *geo, ws, nbytes)

        for kw in (dict(x=None), dict(w=None), dict(go=None), dict(gw=None), dict(ws=None)):
            assert b(**kw) == -1 and b"null argument" in built.cp_last_error(), kw
        assert b(nbytes=need - 1) == -1 and b"workspace too small" in built.cp_last_error()
        assert b(geo=(0,) + ok[1:]) == -1 and b"at least 1" in built.cp_last_error()
        assert b(geo=ok[:2] + (0,) + ok[3:]) == -1 and b"at least 1" in built.cp_last_error()
        assert b(geo=ok[:5] + (2, 2, 0) + ok[8:]) == -1 and b"unsupported geometry" in built.cp_last_error()
        assert b(geo=ok[:8] + (2,)) == -1 and b"unsupported geometry" in built.cp_last_error()
        assert b(geo=(64, 1024, 1024) + ok[3:]) == -1 and b"elements or more" in built.cp_last_error()
        for kw in (dict(x=ctypes.c_void_p(0x1004)), dict(w=ctypes.c_void_p(0x1008)), dict(go=ctypes.c_void_p(0x100c)),
                   dict(gx=ctypes.c_void_p(0x1004)), dict(gw=ctypes.c_void_p(0x1008)), dict(ws=ctypes.c_void_p(0x1004))):
            assert b(**kw) == -1 and b"16-byte aligned" in built.cp_last_error(), kw

    def f(x=p, w=p, add=p, out=p, geo=(2, 8, 8, 16, 2)):
        return fwd(None, x, w, add, out, *geo)

    for kw in (dict(x=None), dict(w=None), dict(out=None)):
        assert f(**kw) == -1 and b"null argument" in built.cp_last_error(), kw
    for geo in ((0, 8, 8, 16, 2), (2, 0, 8, 16, 2), (2, 8, 0, 16, 2)):
        assert f(geo=geo) == -1 and b"at least 1" in built.cp_last_error(), geo
    for geo in ((2, 8, 8, 6, 2), (2, 8, 8, 16, 3), (2, 8, 8, 16, 8), (2, 8, 8, 16, 0), (2, 8, 8, 16, 1), (2, 8, 8, 964, 2),
                (2, 8, 8, 244, 4)):
        assert f(geo=geo) == -1 and b"unsupported geometry" in built.cp_last_error(), geo
    assert f(geo=(64, 1024, 1024, 16, 2)) == -1 and b"elements or more" in built.cp_last_error()
    for kw in (dict(x=ctypes.c_void_p(0x1004)), dict(add=ctypes.c_void_p(0x1008)), dict(out=ctypes.c_void_p(0x100c))):
        assert f(**kw) == -1 and b"16-byte aligned" in built.cp_last_error(), kw


def test_no_cpu_path(built):
    for c in (R.DW_CASES[1], R.DENSE_CASES[1]):
        inp = R.inputs(0, c)
        with pytest.raises(RuntimeError, match="HIP device"):
            hip.conv_transpose2d_backward(R.nhwc(inp.x), inp.w, R.nhwc(inp.go), c.stride, c.pad, c.groups)
        with pytest.raises(RuntimeError, match="HIP device"):
            deconv.conv_transpose2d(inp.x, inp.w, c.stride, c.pad, c.groups)
        with pytest.raises(RuntimeError, match="HIP device"):
            deconv.ConvTranspose2d(c.Cin, c.Cout, c.K, c.stride, c.pad, groups=c.groups, bias=False)(inp.x)
    c = R.DW_CASES[1]
    inp = R.inputs(0, c)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.conv_transpose2d_dw(R.nhwc(inp.x), inp.w, c.stride, add=R.nhwc(inp.add))
    with pytest.raises(RuntimeError, match="HIP device"):
        deconv.ConvTranspose2d(c.Cin, c.Cout, c.K, c.stride, c.pad, groups=c.groups, bias=False)(inp.x, inp.add)


MODULE_ARGS = [((16, 16, 4), dict(stride=2, padding=1, groups=16, bias=False)),
               ((64, 64, 8), dict(stride=4, padding=2, groups=64, bias=False)),
               ((32, 64, 4), dict(stride=2, padding=1, bias=False)),
               ((256, 256, 4, 2, 1, 0, 256, False), {})]


def test_conv_transpose2d_module_is_nn_conv_transpose2d_but_for_forward():
    for args, kwargs in MODULE_ARGS:
        torch.manual_seed(3)
        ours = deconv.ConvTranspose2d(*args, **kwargs)
        torch.manual_seed(3)
        theirs = nn.ConvTranspose2d(*args, **kwargs)
        a, b = ours.state_dict(), theirs.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        assert [n for n, _ in ours.named_parameters()] == [n for n, _ in theirs.named_parameters()]
        assert repr(ours) == repr(theirs) and isinstance(ours, nn.ConvTranspose2d)
    # the class body adds `forward` and nothing else (its __init__ only refuses what the library does not run)
    assert {n for n in vars(deconv.ConvTranspose2d) if not n.startswith("__")} == {"forward"}
    assert {n for n in vars(deconv.ConvTranspose2d) if n.startswith("__")} <= {"__module__", "__doc__", "__init__", "__firstlineno__",
                                                                               "__static_attributes__", "__parameters__"}
    for args, kwargs, text in (((16, 16, 4), dict(stride=2, padding=1, groups=16), "bias"),
                               ((16, 16, 4), dict(stride=2, padding=1, groups=16, bias=False, output_padding=1), "output_padding"),
                               ((16, 16, 4), dict(stride=2, padding=1, groups=2, bias=False), "geometry"),
                               ((16, 16, 2), dict(stride=2, groups=16, bias=False), "geometry"),
                               ((6, 6, 4), dict(stride=2, padding=1, groups=6, bias=False), "multiple of 4"),
                               ((32, 48, 4), dict(stride=2, padding=1, bias=False), "multiples of 32"),
                               ((16, 16, 16), dict(stride=8, padding=4, groups=16, bias=False), "geometry"),
                               ((16, 16, 4), dict(stride=2, padding=1, groups=16, bias=False, dtype=torch.float64), "float64"),
                               ((32, 32, 4), dict(stride=2, padding=2, dilation=2, bias=False), "dilation")):
        with pytest.raises(NotImplementedError, match=text):
            deconv.ConvTranspose2d(*args, **kwargs)


class _Derived(nn.ConvTranspose2d):
    pass


class _Tree(nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = nn.Conv2d(64, 32, 1, bias=False)
        self.bn = nn.BatchNorm2d(32)
        self.up2 = nn.ConvTranspose2d(32, 32, 4, stride=2, padding=1, groups=32, bias=False)
        self.up4 = nn.ConvTranspose2d(64, 64, 8, stride=4, padding=2, groups=64, bias=False)
        self.stack = nn.Sequential(nn.ConvTranspose2d(64, 32, 4, stride=2, padding=1, bias=False), nn.ReLU())
        self.biased = nn.ConvTranspose2d(32, 32, 4, stride=2, padding=1, groups=32)
        self.outpad = nn.ConvTranspose2d(32, 32, 4, stride=2, padding=1, output_padding=1, groups=32, bias=False)
        self.grouped = nn.ConvTranspose2d(32, 32, 4, stride=2, padding=1, groups=2, bias=False)
        self.k2s2 = nn.ConvTranspose2d(32, 32, 2, stride=2, groups=32, bias=False)
        self.c6 = nn.ConvTranspose2d(6, 6, 4, stride=2, padding=1, groups=6, bias=False)
        self.f64 = nn.ConvTranspose2d(32, 32, 4, stride=2, padding=1, groups=32, bias=False).double()
        self.derived = _Derived(32, 32, 4, stride=2, padding=1, groups=32, bias=False)


def test_use_hip_deconvs_reclasses_in_place():
    torch.manual_seed(0)
    tree = _Tree()
    params = dict(tree.named_parameters())
    keys = list(tree.state_dict())
    values = {k: v.clone() for k, v in tree.state_dict().items()}
    text = repr(tree)
    converted, skipped = deconv.use_hip_deconvs(tree)
    assert converted == ["up2", "up4", "stack.0"]
    assert sorted(skipped) == ["biased", "c6", "derived", "f64", "grouped", "k2s2", "outpad"]
    assert "bias" in skipped["biased"] and "output_padding" in skipped["outpad"] and "float64" in skipped["f64"]
    assert "geometry outside the table" in skipped["grouped"] and "groups = 2" in skipped["grouped"]
    assert "geometry outside the table" in skipped["k2s2"] and "kernel 2" in skipped["k2s2"]
    assert "geometry outside the table" in skipped["c6"] and "multiple of 4" in skipped["c6"]
    assert skipped["derived"] == "subclass _Derived of nn.ConvTranspose2d keeps its own forward"
    for m in (tree.up2, tree.up4, tree.stack[0]):
        assert type(m) is deconv.ConvTranspose2d
    for m in (tree.biased, tree.outpad, tree.grouped, tree.k2s2, tree.c6, tree.f64):
        assert type(m) is nn.ConvTranspose2d
    assert type(tree.derived) is _Derived and type(tree.proj) is nn.Conv2d and type(tree.bn) is nn.BatchNorm2d
    assert type(tree.stack[1]) is nn.ReLU
    after = dict(tree.named_parameters())
    assert list(after) == list(params) and all(after[k] is params[k] for k in params)
    assert list(tree.state_dict()) == keys and all(torch.equal(tree.state_dict()[k], values[k]) for k in keys)
    assert repr(tree) == text
    again, skipped2 = deconv.use_hip_deconvs(tree)
    assert again == [] and skipped2 == skipped
    # a lone layer is converted too (the root module itself)
    lone = nn.ConvTranspose2d(8, 8, 4, stride=2, padding=1, groups=8, bias=False)
    assert deconv.use_hip_deconvs(lone) == ([""], {}) and type(lone) is deconv.ConvTranspose2d
    # dilation is a reason of its own
    dil = nn.ConvTranspose2d(32, 32, 4, stride=2, padding=2, dilation=2, bias=False)
    assert "dilation" in deconv.use_hip_deconvs(dil)[1][""]
    # use_hip_convs and use_hip_norms still convert their own layers of the tree, and leave the transposed ones alone
    got, left = conv.use_hip_convs(tree)
    assert got == ["proj"] and type(tree.proj) is conv.Conv2d and type(tree.up2) is deconv.ConvTranspose2d
    assert all("ConvTranspose2d" in why for why in left.values())
    assert norm.use_hip_norms(tree) == (["bn"], {}) and type(tree.bn) is norm.BatchNorm2d
    assert deconv.use_hip_deconvs(tree) == ([], skipped)
