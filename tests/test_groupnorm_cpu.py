"""CPU tests (no GPU) of the training GroupNorm: the C ABI's declarations, workspace arithmetic and refusals (cp_groupnorm_*),
the group_norm.GroupNorm module and use_hip_group_norms."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import __graft_entry__ as ge
from centerpose_amd import group_norm, hip, norm
from tests import groupnorm_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_groupnorm_workspace_bytes", "cp_groupnorm_forward_nhwc", "cp_groupnorm_backward_nhwc")


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def test_symbols_declared_exported_and_listed(built):
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and hasattr(built, name) and name in hip.exported_symbols(), name
    assert int(re.search(r"#define\s+CP_ABI_VERSION\s+(\d+)", header).group(1)) == 7 == built.cp_abi_version()
    assert "pose_dla_dcn.py:491-521" in header and "GN.py" in header


def test_workspace_query_is_host_arithmetic(built):
    q = built.cp_groupnorm_workspace_bytes
    for c in R.CASES + R.LARGE_MEAN_CASES:
        assert q(*c) > 0, c
    assert 0 < q(16, 128, 128, 256, 32) < 64 << 20
    for geo in ((1, 2, 4, 1), (7, 9, 40, 2), (128, 128, 64, 32), (16, 16, 512, 32), (33, 31, 4096, 32)):
        sizes = [q(B, *geo) for B in (1, 2, 3, 8, 16, 17, 32, 64)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], geo


def test_refusals_without_a_device(built):
    q, fwd, bwd = built.cp_groupnorm_workspace_bytes, built.cp_groupnorm_forward_nhwc, built.cp_groupnorm_backward_nhwc

    def refused(geo, text):
        assert q(*geo) == 0
        assert text in built.cp_last_error(), (geo, built.cp_last_error())

    shape_refusals = [((0, 8, 8, 16, 4), b"at least 1"), ((2, 0, 8, 16, 4), b"at least 1"), ((2, 8, 0, 16, 4), b"at least 1"),
                      ((2, 8, 8, 6, 2), b"multiple of 4"), ((2, 8, 8, 0, 1), b"multiple of 4"), ((2, 8, 8, 4100, 4), b"4..4096"),
                      ((2, 8, 8, 16, 0), b"divide C"), ((2, 8, 8, 16, -2), b"divide C"), ((2, 8, 8, 16, 3), b"divide C"),
                      ((2, 8, 8, 16, 32), b"divide C"), ((2, 8, 8, 48, 16), b"1, 2 or a multiple of 4"),
                      ((2, 8, 8, 24, 4), b"1, 2 or a multiple of 4"), ((64, 1024, 1024, 32, 8), b"2^31 elements"),
                      ((1, 8192, 8192, 32, 32), b"2^31 elements")]
    for geo, text in shape_refusals:
        refused(geo, text)
    # the calls themselves: refused before any launch (no device is touched; the pointers are never dereferenced)
    p = ctypes.c_void_p(0x1000)
    ok = (2, 8, 8, 16, 4)
    need = q(*ok)
    assert need > 0

    def f(x=p, gamma=p, beta=p, y=ctypes.c_void_p(0x2000), mean=p, invstd=p, geo=ok, eps=1e-5, act=1, ws=p, nbytes=need):
        return fwd(None, x, gamma, beta, y, mean, invstd, *geo, eps, act, ws, nbytes)

    def b(x=p, y=p, go=p, gamma=p, mean=p, invstd=p, gx=p, gg=p, gb=p, geo=ok, ws=p, nbytes=need):
        return bwd(None, x, y, go, gamma, mean, invstd, gx, gg, gb, *geo, ws, nbytes)

    for kw in (dict(x=None), dict(y=None), dict(mean=None), dict(invstd=None), dict(ws=None)):
        assert f(**kw) == -1 and b"null argument" in built.cp_last_error(), kw
    for kw in (dict(x=None), dict(go=None), dict(mean=None), dict(invstd=None), dict(ws=None)):
        assert b(**kw) == -1 and b"null argument" in built.cp_last_error(), kw
    for call in (f, b):
        assert call(nbytes=need - 1) == -1 and b"workspace too small" in built.cp_last_error()
        for geo, text in shape_refusals:
            assert call(geo=geo) == -1 and text in built.cp_last_error(), geo
    for act in (-1, 2, 3):
        assert f(act=act) == -1 and b"act must be" in built.cp_last_error()
    assert f(eps=-1e-5) == -1 and b"eps must not be negative" in built.cp_last_error()
    assert f(eps=float("nan")) == -1 and b"eps must not be negative" in built.cp_last_error()
    assert f(y=p) == -1 and b"must not alias" in built.cp_last_error()
    assert f(x=ctypes.c_void_p(0x1004)) == -1 and b"16-byte aligned" in built.cp_last_error()
    assert f(mean=ctypes.c_void_p(0x1008)) == -1 and b"16-byte aligned" in built.cp_last_error()
    assert b(go=ctypes.c_void_p(0x1008)) == -1 and b"16-byte aligned" in built.cp_last_error()
    assert b(gg=ctypes.c_void_p(0x100c)) == -1 and b"16-byte aligned" in built.cp_last_error()


def test_no_cpu_path(built):
    c = R.Case(2, 4, 4, 8, 2)
    inp = R.inputs(0, c)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.group_norm_forward(R.nhwc(inp.x), c.G, inp.gamma, inp.beta)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.group_norm_backward(R.nhwc(inp.x), R.nhwc(inp.go), c.G, torch.zeros(2, 2), torch.ones(2, 2), gamma=inp.gamma)
    with pytest.raises(RuntimeError, match="HIP device"):
        group_norm.group_norm(inp.x, c.G, inp.gamma, inp.beta, relu=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        group_norm.GroupNorm(2, 8)(inp.x)


def test_groupnorm_module_is_nn_groupnorm_but_for_forward():
    for args, kwargs in (((4, 16), {}), ((32, 64), dict(eps=1e-3)), ((2, 40), dict(affine=False))):
        ours, theirs = group_norm.GroupNorm(*args, **kwargs), nn.GroupNorm(*args, **kwargs)
        a, b = ours.state_dict(), theirs.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        assert [n for n, _ in ours.named_parameters()] == [n for n, _ in theirs.named_parameters()]
        assert repr(ours) == repr(theirs) and isinstance(ours, nn.GroupNorm) and ours.relu is False
    assert {n for n in vars(group_norm.GroupNorm) if not n.startswith("__")} == {"forward", "relu"}


class _Tree(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(8, 16, 3, padding=1, bias=False)
        self.gn1 = nn.GroupNorm(4, 16)
        self.block = nn.Sequential(nn.Conv2d(16, 64, 1), nn.GroupNorm(32, 64, affine=False), nn.ReLU(), nn.GroupNorm(3, 6))
        self.odd = nn.GroupNorm(16, 48)     # the reference's head_conv = 48 case: three channels per group
        self.bn = nn.BatchNorm2d(16)
        self.ln = nn.LayerNorm(16)
        self.f64 = nn.GroupNorm(4, 16).double()
        self.one = nn.GroupNorm(16, 16)


class _Derived(nn.GroupNorm):
    pass


def test_use_hip_group_norms_reclasses_in_place():
    torch.manual_seed(0)
    tree = _Tree()
    tree.derived = _Derived(4, 16)
    params = dict(tree.named_parameters())
    keys = list(tree.state_dict())
    converted, skipped = group_norm.use_hip_group_norms(tree)
    assert converted == ["gn1", "block.1", "one"]
    assert sorted(skipped) == ["block.3", "derived", "f64", "odd"]
    assert "multiple of 4" in skipped["block.3"] and "float64" in skipped["f64"]
    assert skipped["derived"] == "subclass _Derived keeps its own forward"
    assert "3 channels per group" in skipped["odd"]
    G = group_norm.GroupNorm
    assert type(tree.gn1) is G and type(tree.block[1]) is G and type(tree.one) is G
    assert type(tree.block[3]) is nn.GroupNorm and type(tree.f64) is nn.GroupNorm and type(tree.odd) is nn.GroupNorm
    assert type(tree.derived) is _Derived and type(tree.bn) is nn.BatchNorm2d and type(tree.ln) is nn.LayerNorm
    assert type(tree.conv1) is nn.Conv2d
    after = dict(tree.named_parameters())
    assert list(after) == list(params) and all(after[k] is params[k] for k in params)
    assert list(tree.state_dict()) == keys and tree.gn1.relu is False
    assert repr(tree.gn1) == repr(nn.GroupNorm(4, 16))
    again, skipped2 = group_norm.use_hip_group_norms(tree)
    assert again == [] and skipped2 == skipped
    lone = nn.GroupNorm(2, 8)
    assert group_norm.use_hip_group_norms(lone) == ([""], {}) and type(lone) is group_norm.GroupNorm
    # use_hip_norms and use_hip_group_norms do not see each other's layers
    assert norm.use_hip_norms(tree) == (["bn"], {}) and type(tree.gn1) is G
