"""CPU tests (no GPU) of the hourglass merge's C ABI (cp_upsample2_add_nhwc / cp_upsample2_add_backward_nhwc), the wide stem
pair beside them, and the Python layer's refusals: declarations, exports, the binding table, and every shape rule refused on
the host with its message before any launch."""
import ctypes
import os
import re

import pytest
import torch

import __graft_entry__ as ge
from centerpose_amd import hip, stem, upsample

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_upsample2_add_nhwc", "cp_upsample2_add_backward_nhwc", "cp_conv2d_stem_wide_backward_workspace_bytes",
       "cp_conv2d_stem_wide_backward")


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
    assert header.count("large_hourglass.py:95-112") >= 1 and "large_hourglass.py:209-212" in header
    ops = open(os.path.join(REPO, "centerpose_amd", "csrc", "ops.hip")).read()
    assert "cp_upsample2_add_nhwc" in ops and "cp_upsample2_add_backward_nhwc" in ops


def test_merge_refusals_before_any_launch(built):
    """Shape errors are found on the host (there is no device here): code and text, null pointers included."""
    a = ctypes.c_void_p(256)   # never dereferenced: every call below is refused before a launch
    fwd = lambda *geo, p=(a, a, a): built.cp_upsample2_add_nhwc(None, *p, *geo)
    bwd = lambda *geo, p=(a, a): built.cp_upsample2_add_backward_nhwc(None, *p, *geo)
    for geo, word in (((0, 4, 4, 8), b"at least 1"), ((1, 0, 4, 8), b"at least 1"), ((1, 4, 0, 8), b"at least 1"),
                      ((1, 4, 4, 6), b"multiple of 4"), ((1, 4, 4, 0), b"multiple of 4"), ((1, 4, 4, 2), b"multiple of 4"),
                      ((1, 4, 4, -4), b"multiple of 4"),
                      ((2, 2048, 2048, 64), b"2^31"),       # low has 2^29 elements, out 2^31
                      ((64, 4096, 4096, 256), b"2^31"), ((2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30), b"2^31")):
        assert fwd(*geo) == -1 and word in built.cp_last_error(), geo
        assert bwd(*geo) == -1 and word in built.cp_last_error(), geo
    # the largest tensor just below 2^31 elements passes the shape rules: refused for its pointers instead
    assert fwd(1, 2048, 2048, 124, p=(None, a, a)) == -1 and b"null" in built.cp_last_error()
    for p in ((None, a, a), (a, None, a), (a, a, None)):
        assert fwd(1, 2, 2, 4, p=p) == -1 and b"null" in built.cp_last_error(), p
    for p in ((None, a), (a, None)):
        assert bwd(1, 2, 2, 4, p=p) == -1 and b"null" in built.cp_last_error(), p
    odd = ctypes.c_void_p(260)
    assert fwd(1, 2, 2, 4, p=(a, odd, a)) == -1 and b"aligned" in built.cp_last_error()
    assert bwd(1, 2, 2, 4, p=(odd, a)) == -1 and b"aligned" in built.cp_last_error()


def test_wide_stem_refusals_before_any_launch(built):
    q, q64 = built.cp_conv2d_stem_wide_backward_workspace_bytes, built.cp_conv2d_stem_backward_workspace_bytes
    # same rule as the narrow pair: slabs of [Cout][49 Cin + 1] floats, at most 512 of them, rounded to 256 bytes
    assert q(1, 8, 64, 3, 128, 1) == (1 * 128 * 148 * 4 + 255) // 256 * 256
    assert q(64, 512, 512, 3, 128, 2) == 512 * 128 * 148 * 4
    for cout in (16, 32, 48, 64):
        assert q(2, 64, 96, 3, cout, 2) == q64(2, 64, 96, 3, cout, 2) > 0
    for cout in (80, 96, 112, 128):
        assert q(2, 64, 96, 1, cout, 1) > 0 and q64(2, 64, 96, 1, cout, 1) == 0
    for geo, word in (((2, 64, 96, 4, 128, 1), b"Cin"), ((2, 64, 96, 3, 144, 1), b"Cout"), ((2, 64, 96, 3, 120, 1), b"Cout"),
                      ((2, 64, 96, 3, 0, 1), b"Cout"), ((2, 64, 96, 3, 128, 3), b"stride"), ((0, 64, 96, 3, 128, 1), b"at least 1"),
                      ((64, 4096, 4096, 3, 128, 1), b"2^31")):
        assert q(*geo) == 0 and word in built.cp_last_error(), geo
    null = None
    assert built.cp_conv2d_stem_wide_backward(null, null, null, null, null, null, null, 0, 2, 64, 96, 3, 128, 2) == -1
    assert b"null" in built.cp_last_error()


def test_python_layer_refusals():
    with pytest.raises(RuntimeError, match="HIP device"):
        upsample.upsample2_add(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 2, 2))
    with pytest.raises(RuntimeError, match="HIP device"):
        upsample.UpsampleAdd()(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 2, 2))
    assert not list(upsample.UpsampleAdd().parameters())
    # the eligibility rule is split: a directly constructed StemConv2d takes the wider set, use_hip_stems does not
    for cout in (16, 64, 80, 128):
        assert type(stem.StemConv2d(3, cout, 7, stride=2, padding=3, bias=False)) is stem.StemConv2d
    for cout in (24, 144):
        with pytest.raises(NotImplementedError):
            stem.StemConv2d(3, cout, 7, stride=2, padding=3)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 64, 7, padding=3), torch.nn.Conv2d(3, 128, 7, stride=2, padding=3),
                              torch.nn.Conv2d(3, 80, 7, padding=3))
    assert stem.use_hip_stems(net) == (["0"], {})
    assert type(net[1]) is torch.nn.Conv2d and type(net[2]) is torch.nn.Conv2d
