"""CPU tests (no GPU) of the Conv2d backward's precision argument: the declarations of cp_conv2d_backward_prec_*, their host
arithmetic and refusals, the Python switches, and the premises of the generators the GPU tests rest on
(tests/conv_backward_f16x3_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import __graft_entry__ as ge
from centerpose_amd import conv, hip
from tests import conv_backward_f16x3_cases as C
from tests import conv_backward_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_conv2d_backward_prec_workspace_bytes", "cp_conv2d_backward_prec_nhwc", "cp_conv2d_backward_prec_mask")
F32, F16X3 = 0, 1


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def test_symbols_declared_exported_and_listed(built):
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", text))
    for name in NEW + ("cp_conv2d_backward_workspace_bytes", "cp_conv2d_backward_nhwc", "cp_conv2d_backward_path"):
        assert name in declared and hasattr(built, name) and name in hip.exported_symbols(), name
    assert int(re.search(r"#define\s+CP_ABI_VERSION\s+(\d+)", header).group(1)) == 7 == built.cp_abi_version() == hip.ABI_VERSION
    assert "Arithmetic is float32 whatever cp_set_default_precision says" in header   # the old calls keep their meaning
    assert hip.PRECISIONS == {"f32": F32, "f16x3": F16X3}


def test_f32_query_is_the_old_query(built):
    old, new = built.cp_conv2d_backward_workspace_bytes, built.cp_conv2d_backward_prec_workspace_bytes
    for c in R.CASES + C.KSTEP_CASES + R.dla34_shapes(64):
        for need_x in (0, 1):
            assert new(*C.geo(c), need_x, F32) == old(*C.geo(c), need_x) > 0, c


def test_f16x3_query_is_host_arithmetic(built):
    old, new = built.cp_conv2d_backward_workspace_bytes, built.cp_conv2d_backward_prec_workspace_bytes
    for c in R.CASES + C.KSTEP_CASES + R.dla34_shapes(64):
        mask = built.cp_conv2d_backward_prec_mask(*C.geo(c), F16X3)
        assert mask == (3 if R.is_mfma(c) else 0), c
        for need_x in (0, 1):
            # the split copies of grad_out and (but for 1x1 layers) x come on top on the MFMA path; nothing changes off it
            extra = new(*C.geo(c), need_x, F16X3) - old(*C.geo(c), need_x)
            Ho, Wo = R.out_size(c)
            floor = 4 * c.B * Ho * Wo * C.cop(c) + (4 * c.B * c.H * c.W * c.Cin if c.k > 1 else 0)
            assert (extra > floor) if mask else extra == 0, c
        assert new(*C.geo(c), 1, F16X3) >= new(*C.geo(c), 0, F16X3)
    for g in ((128, 128, 64, 64, 3, 3, 1, 1), (64, 64, 128, 27, 3, 3, 1, 1), (31, 31, 64, 128, 1, 1, 2, 0), (64, 64, 64, 128, 3, 3, 2, 1)):
        sizes = [new(B, *g, 1, F16X3) for B in (1, 2, 3, 8, 16, 17, 32, 64)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], g


def test_mask(built):
    mask = built.cp_conv2d_backward_prec_mask
    for c in C.CASES + C.MODULE_CASES:
        assert mask(*C.geo(c), F16X3) == 3 and mask(*C.geo(c), F32) == 0, c
        assert hip.ops.conv2d_backward_precision_mask(*C.geo(c)) == 3 and hip.ops.conv2d_backward_precision_mask(*C.geo(c), precision="f32") == 0
    lowc = (8, 128, 128, 16, 16, 3, 3, 1, 1)
    assert built.cp_conv2d_backward_path(*lowc) == hip.CONV_BWD_LOWC and mask(*lowc, F16X3) == 0
    for c in R.GENERIC_CASES:
        assert built.cp_conv2d_backward_path(*C.geo(c)) != hip.CONV_BWD_MFMA and mask(*C.geo(c), F16X3) == 0, c
    # a stride-1 data gradient beyond the 32-bit byte offsets of the f16x3 implicit GEMM stays float32; the weight gradient does not
    big = (124, 512, 512, 32, 32, 3, 3, 1, 1)   # grad_out: below 2^31 elements, above 0xf0000000 bytes
    assert mask(*big, F16X3) == 1 and mask(*big[:7], 2, 1, F16X3) == 3
    with pytest.raises(RuntimeError, match="Cin must be"):
        hip.ops.conv2d_backward_precision_mask(2, 16, 16, 6, 64, 3, 3, 1, 1)
    with pytest.raises(ValueError, match="precision"):
        hip.ops.conv2d_backward_precision_mask(2, 16, 16, 64, 64, 3, 3, 1, 1, precision="bf16")


REFUSED = [((0, 16, 16, 64, 64, 3, 3, 1, 1), b"at least 1"), ((2, 0, 16, 64, 64, 3, 3, 1, 1), b"at least 1"),
           ((2, 16, 0, 64, 64, 3, 3, 1, 1), b"at least 1"), ((2, 16, 16, 64, 0, 3, 3, 1, 1), b"at least 1"),
           ((2, 16, 16, 6, 64, 3, 3, 1, 1), b"Cin must be"), ((2, 16, 16, 3, 64, 7, 7, 2, 3), b"Cin must be"),
           ((2, 16, 16, 0, 64, 3, 3, 1, 1), b"Cin must be"), ((2, 16, 16, 64, 64, 8, 8, 1, 1), b"unsupported geometry"),
           ((2, 16, 16, 64, 64, 3, 3, 5, 1), b"unsupported geometry"), ((2, 16, 16, 64, 64, 3, 3, 1, 3), b"unsupported geometry"),
           ((2, 2, 16, 64, 64, 5, 5, 1, 1), b"empty output"), ((2, 16, 1, 64, 64, 3, 3, 1, 0), b"empty output"),
           ((64, 1024, 1024, 64, 64, 3, 3, 1, 1), b"2^31 elements"), ((1, 8192, 8192, 32, 4, 1, 1, 1, 0), b"2^31 elements")]


def test_refusals_without_a_device(built):
    """Every refused geometry of tests/test_conv_backward_cpu.py, in both precisions, and an unknown precision."""
    q, call, mask = built.cp_conv2d_backward_prec_workspace_bytes, built.cp_conv2d_backward_prec_nhwc, built.cp_conv2d_backward_prec_mask
    p = ctypes.c_void_p(0x1000)
    ok = (2, 16, 16, 64, 64, 3, 3, 1, 1)

    def bwd(x=p, w=p, y=None, go=p, gx=p, gw=p, gb=p, geo=ok, prec=F16X3, ws=p, nbytes=1 << 40):
        return call(None, x, w, y, go, gx, gw, gb, *geo, prec, ws, nbytes)

    for prec in (F32, F16X3):
        for geo, text in REFUSED:
            assert q(*geo, 1, prec) == 0 and text in built.cp_last_error(), (geo, built.cp_last_error())
            assert mask(*geo, prec) == -1 and text in built.cp_last_error(), (geo, built.cp_last_error())
            assert bwd(geo=geo, prec=prec) == -1 and text in built.cp_last_error(), (geo, built.cp_last_error())
    for prec in (-1, 2, 7):
        assert q(*ok, 1, prec) == 0 and b"unknown precision" in built.cp_last_error()
        assert mask(*ok, prec) == -1 and b"unknown precision" in built.cp_last_error()
        assert bwd(prec=prec) == -1 and b"unknown precision" in built.cp_last_error()
    # the call itself: refused before any launch (no device is touched; the pointers are never dereferenced)
    for prec in (F32, F16X3):
        need = q(*ok, 1, prec)
        assert need > 0
        for kw in (dict(x=None), dict(w=None), dict(go=None), dict(gw=None), dict(ws=None)):
            assert bwd(prec=prec, nbytes=need, **kw) == -1 and b"null argument" in built.cp_last_error(), kw
        assert bwd(prec=prec, nbytes=need - 1) == -1 and b"workspace too small" in built.cp_last_error()
        assert bwd(prec=prec, nbytes=q(*ok, 0, prec)) == -1 and b"workspace too small" in built.cp_last_error()
    # the float32 workspace does not serve the f16x3 call
    assert bwd(nbytes=q(*ok, 1, F32)) == -1 and b"workspace too small" in built.cp_last_error()


def test_python_switches():
    c = R.Case(1, 8, 8, 5, 5, 3, 1, 1)
    inp = R.dyadic_inputs(0, c)
    with pytest.raises(ValueError, match="precision"):
        hip.ops.conv2d_backward_prec(R.nhwc(inp.x), inp.w, R.nhwc(inp.go), stride=1, pad=1, precision="fp8")
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.ops.conv2d_backward_prec(R.nhwc(inp.x), inp.w, R.nhwc(inp.go), stride=1, pad=1, precision="f16x3")
    with pytest.raises(ValueError, match="backward_precision"):
        conv.conv2d(inp.x, inp.w, inp.bias, 1, 1, backward_precision="fp8")
    # hip.conv2d_backward keeps its recorded signature; the precision is the argument of ops.conv2d_backward_prec
    import inspect
    old, new = inspect.signature(hip.conv2d_backward).parameters, inspect.signature(hip.ops.conv2d_backward_prec).parameters
    assert list(new) == list(old) + ["precision"] and new["precision"].default == "f32"
    assert all(new[k].default == old[k].default for k in old)
    assert not hasattr(hip, "conv2d_backward_prec") and not hasattr(hip, "conv2d_backward_precision_mask")
    assert conv.Conv2d.backward_precision == "f32" and "backward_precision" in vars(conv.Conv2d)
    tree = nn.Sequential(nn.Conv2d(8, 16, 3, padding=1), nn.ReLU(), nn.Sequential(conv.Conv2d(16, 16, 1), nn.Conv2d(16, 16, 3, dilation=2)))
    assert conv.set_backward_precision(tree, "f16x3") == 1 and tree[2][0].backward_precision == "f16x3"
    converted, skipped = conv.use_hip_convs(tree)                       # None leaves the attribute alone
    assert converted == ["0"] and list(skipped) == ["2.1"]
    assert tree[0].backward_precision == "f32" and tree[2][0].backward_precision == "f16x3"
    assert conv.use_hip_convs(tree, backward_precision="f16x3") == ([], skipped)
    assert tree[0].backward_precision == "f16x3" and type(tree[2][1]) is nn.Conv2d and not hasattr(tree[2][1], "backward_precision")
    assert conv.set_backward_precision(tree, "f32") == 2 and tree[0].backward_precision == tree[2][0].backward_precision == "f32"
    assert "backward_precision" not in tree.state_dict() and repr(tree[0]) == repr(nn.Conv2d(8, 16, 3, padding=1))
    with pytest.raises(ValueError, match="backward_precision"):
        conv.set_backward_precision(tree, "bf16")
    with pytest.raises(ValueError, match="backward_precision"):
        conv.use_hip_convs(tree, backward_precision="bf16")


def test_cases_cover_what_they_should():
    assert len(set(C.CASES)) == len(C.CASES)
    for k, s in ((3, 1), (3, 2), (1, 2)):
        assert sorted(R.out_size(c)[1] for c in C.KSTEP_CASES if (c.k, c.stride) == (k, s)) == [15, 16, 17, 31, 33]
    assert all(c.Cin == 32 and c.Cout == 40 for c in C.KSTEP_CASES)
    assert [c for c in R.MFMA_CASES if c not in C.CASES] == [R.MFMA_CASES[0]]   # only the 128 x 128 map is left out
    for c in C.TWO_LEVEL_CASES:
        Ho, Wo = R.out_size(c)
        assert max(c.B * Ho * Wo, c.k * c.k * C.cop(c)) * (1 + 2.0 ** -12) < 2 ** 12
    assert {(c.k, c.stride) for c in C.TWO_LEVEL_CASES} == {(3, 1), (3, 2), (1, 1), (1, 2)}


def test_split_premise_of_the_two_level_values():
    """hi + lo == the scaled value for every value the two-level generator emits, lo == 0 for the integers, and lo != 0 where both
    parts are there -- so a kernel that drops hi*lo or lo*hi cannot reproduce the reference."""
    vals = np.array(C.TWO_LEVEL_VALUES, dtype=np.float32)
    assert len(vals) == 9 and np.all(vals.astype(np.float64) == np.array(C.TWO_LEVEL_VALUES))
    for amax in (1.0, 1.0 + 2.0 ** -12):            # the |max| of a tensor of such values
        s = C.np_scale(amax)
        assert s == 2.0 ** 14
        hi, lo = C.np_split(vals * np.float32(s))
        assert np.all(hi + lo == vals.astype(np.float64) * s)
        for v, l in zip(C.TWO_LEVEL_VALUES, lo):
            a = round(v)
            assert (l == 0) == (a == 0 or v == a), (v, l)
    for amax in (1.0, 2.0):                         # the dyadic generator: integers in [-2, 2]
        ints = np.arange(-2, 3, dtype=np.float32)
        hi, lo = C.np_split(ints * np.float32(C.np_scale(amax)))
        assert np.all(lo == 0) and np.all(hi == ints * C.np_scale(amax))


@pytest.mark.parametrize("which", ["xw", "go"])
def test_two_level_generator(which):
    for c in C.TWO_LEVEL_CASES:
        inp = C.two_level_inputs(sum(c) + 3, c, which)   # asserts inside
        fine = (inp.x, inp.w) if which == "xw" else (inp.go,)
        if min(t.numel() for t in fine) >= 256:
            assert all(bool(((t != t.round()) & (t.round() != 0)).any()) for t in fine), c   # values with both parts
    # the float64 reference of a two-level case is not the reference of its integer parts: the cross terms carry weight
    c = C.KSTEP_CASES[2]
    inp = C.two_level_inputs(sum(c) + 3, c, "xw")
    full = R.reference(inp.x, inp.w, inp.go, c.stride, c.pad)
    part = R.reference(inp.x.round(), inp.w.round(), inp.go, c.stride, c.pad)
    assert not torch.equal(full[0], part[0]) and not torch.equal(full[1], part[1])
    # ... and float32 autograd reproduces it exactly: the sums are exact in float32 in any order
    for a, b in zip(R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, inp.y, dtype=torch.float32), R.reference(inp.x, inp.w, inp.go, c.stride, c.pad, inp.y)):
        assert torch.equal(a.double(), b)
