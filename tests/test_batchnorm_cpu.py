"""CPU tests (no GPU) of the training BatchNorm: the C ABI's declarations, workspace arithmetic and refusals (cp_batchnorm_*),
the norm.BatchNorm2d module and use_hip_norms."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import __graft_entry__ as ge
from centerpose_amd import hip, norm
from tests import batchnorm_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_batchnorm_workspace_bytes", "cp_batchnorm_forward_nhwc", "cp_batchnorm_backward_nhwc")


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
    for cite in ("pose_dla_dcn.py:40-62", "pose_dla_dcn.py:150-168", "pose_dla_dcn.py:381", "resnet_dcn.py"):
        assert cite in header


def test_workspace_query_is_host_arithmetic(built):
    q = built.cp_batchnorm_workspace_bytes
    for c in R.CASES + R.LARGE_MEAN_CASES:
        assert q(*c) > 0, c
    assert 0 < q(16, 512, 512, 16) < 64 << 20
    assert 0 < q(64, 128, 128, 4096 // 4) < 64 << 20
    for geo in ((1, 2, 4), (7, 9, 20), (128, 128, 16), (16, 16, 512), (33, 31, 4096), (512, 512, 16)):
        sizes = [q(B, *geo) for B in (1, 2, 3, 8, 16, 17, 32, 64)]
        assert sizes == sorted(sizes) and sizes[0] <= sizes[-1], geo
    assert q(1, 128, 128, 16) < q(64, 128, 128, 16)


def test_refusals_without_a_device(built):
    q, fwd, bwd = built.cp_batchnorm_workspace_bytes, built.cp_batchnorm_forward_nhwc, built.cp_batchnorm_backward_nhwc

    def refused(geo, text):
        assert q(*geo) == 0
        assert text in built.cp_last_error(), (geo, built.cp_last_error())

    refused((0, 8, 8, 16), b"at least 1")
    refused((2, 0, 8, 16), b"at least 1")
    refused((2, 8, 0, 16), b"at least 1")
    refused((2, 8, 8, 6), b"multiple of 4")
    refused((2, 8, 8, 0), b"multiple of 4")
    refused((2, 8, 8, 2), b"multiple of 4")
    refused((2, 8, 8, 4100), b"4..4096")
    refused((64, 1024, 1024, 32), b"2^31 elements")
    refused((1, 8192, 8192, 32), b"2^31 elements")
    # the calls themselves: refused before any launch (no device is touched; the pointers are never dereferenced)
    p = ctypes.c_void_p(0x1000)
    ok = (2, 8, 8, 16)
    need = q(*ok)
    assert need > 0

    def f(x=p, gamma=p, beta=p, res=p, rm=p, rv=p, y=ctypes.c_void_p(0x2000), mean=p, invstd=p, geo=ok, training=1, momentum=0.1,
          eps=1e-5, act=1, ws=p, nbytes=need):
        return fwd(None, x, gamma, beta, res, rm, rv, y, mean, invstd, *geo, training, momentum, eps, act, ws, nbytes)

    def b(x=p, y=p, go=p, gamma=p, mean=p, invstd=p, gx=p, gr=p, gg=p, gb=p, geo=ok, training=1, ws=p, nbytes=need):
        return bwd(None, x, y, go, gamma, mean, invstd, gx, gr, gg, gb, *geo, training, ws, nbytes)

    for kw in (dict(x=None), dict(y=None), dict(mean=None), dict(invstd=None), dict(ws=None)):
        assert f(**kw) == -1 and b"null argument" in built.cp_last_error(), kw
    for kw in (dict(x=None), dict(go=None), dict(mean=None), dict(invstd=None), dict(ws=None)):
        assert b(**kw) == -1 and b"null argument" in built.cp_last_error(), kw
    for call in (f, b):
        assert call(nbytes=need - 1) == -1 and b"workspace too small" in built.cp_last_error()
        assert call(geo=(0, 8, 8, 16)) == -1 and b"at least 1" in built.cp_last_error()
        assert call(geo=(2, 8, 0, 16)) == -1 and b"at least 1" in built.cp_last_error()
        assert call(geo=(2, 8, 8, 6)) == -1 and b"multiple of 4" in built.cp_last_error()
        assert call(geo=(2, 8, 8, 8192)) == -1 and b"4..4096" in built.cp_last_error()
        assert call(geo=(64, 1024, 1024, 32)) == -1 and b"2^31 elements" in built.cp_last_error()
        assert call(geo=(1, 1, 1, 16)) == -1 and b"B*H*W >= 2" in built.cp_last_error()
    for kw in (dict(rm=None), dict(rv=None), dict(rm=None, rv=None)):
        assert f(training=0, **kw) == -1 and b"evaluation needs running_mean" in built.cp_last_error(), kw
    for act in (-1, 2, 3):
        assert f(act=act) == -1 and b"act must be" in built.cp_last_error()
    assert f(eps=-1e-5) == -1 and b"eps must not be negative" in built.cp_last_error()
    assert f(eps=float("nan")) == -1 and b"eps must not be negative" in built.cp_last_error()
    assert f(y=p) == -1 and b"must not alias" in built.cp_last_error()
    assert f(x=ctypes.c_void_p(0x1004)) == -1 and b"16-byte aligned" in built.cp_last_error()
    assert b(go=ctypes.c_void_p(0x1008)) == -1 and b"16-byte aligned" in built.cp_last_error()


def test_no_cpu_path(built):
    c = R.Case(2, 4, 4, 8)
    inp = R.inputs(0, c)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.batch_norm_forward(R.nhwc(inp.x), inp.gamma, inp.beta)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.batch_norm_backward(R.nhwc(inp.x), R.nhwc(inp.go), inp.rmean, inp.rvar, gamma=inp.gamma)
    with pytest.raises(RuntimeError, match="HIP device"):
        norm.batch_norm(inp.x, inp.gamma, inp.beta, inp.rmean, inp.rvar, True, 0.1, 1e-5, residual=inp.res, relu=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        norm.BatchNorm2d(8)(inp.x)
    with pytest.raises(RuntimeError, match="HIP device"):
        norm.BatchNorm2d(8).eval()(inp.x, inp.res)


def test_batchnorm2d_module_is_nn_batchnorm2d_but_for_forward():
    for args, kwargs in (((16,), {}), ((8,), dict(momentum=None)), ((12,), dict(affine=False)), ((4,), dict(track_running_stats=False)),
                         ((64,), dict(eps=1e-3, momentum=0.01))):
        torch.manual_seed(3)
        ours = norm.BatchNorm2d(*args, **kwargs)
        torch.manual_seed(3)
        theirs = nn.BatchNorm2d(*args, **kwargs)
        a, b = ours.state_dict(), theirs.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        assert [n for n, _ in ours.named_parameters()] == [n for n, _ in theirs.named_parameters()]
        assert [n for n, _ in ours.named_buffers()] == [n for n, _ in theirs.named_buffers()]
        assert repr(ours) == repr(theirs) and isinstance(ours, nn.BatchNorm2d) and ours.relu is False
    assert {n for n in vars(norm.BatchNorm2d) if not n.startswith("__")} == {"forward", "relu"}


class _Tree(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(8, 16, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(16)
        self.block = nn.Sequential(nn.Conv2d(16, 16, 1), nn.BatchNorm2d(16, affine=False), nn.ReLU(), nn.BatchNorm2d(6))
        self.sync = nn.SyncBatchNorm(16)
        self.bn1d = nn.BatchNorm1d(16)
        self.bn3d = nn.BatchNorm3d(16)
        self.gn = nn.GroupNorm(4, 16)
        self.f64 = nn.BatchNorm2d(16).double()
        self.plain = nn.BatchNorm2d(32, momentum=None, track_running_stats=False)


class _Derived(nn.BatchNorm2d):
    pass


def test_use_hip_norms_reclasses_in_place():
    torch.manual_seed(0)
    tree = _Tree()
    tree.derived = _Derived(16)
    params = dict(tree.named_parameters())
    buffers = dict(tree.named_buffers())
    keys = list(tree.state_dict())
    converted, skipped = norm.use_hip_norms(tree)
    assert converted == ["bn1", "block.1", "plain"]
    assert sorted(skipped) == ["block.3", "derived", "f64", "sync"]
    assert "multiple of 4" in skipped["block.3"] and "float64" in skipped["f64"]
    assert skipped["sync"] == "subclass SyncBatchNorm keeps its own forward"
    assert skipped["derived"] == "subclass _Derived keeps its own forward"
    assert type(tree.bn1) is norm.BatchNorm2d and type(tree.block[1]) is norm.BatchNorm2d and type(tree.plain) is norm.BatchNorm2d
    assert type(tree.block[3]) is nn.BatchNorm2d and type(tree.f64) is nn.BatchNorm2d and type(tree.derived) is _Derived
    assert type(tree.sync) is nn.SyncBatchNorm and type(tree.bn1d) is nn.BatchNorm1d and type(tree.bn3d) is nn.BatchNorm3d
    assert type(tree.gn) is nn.GroupNorm and type(tree.conv1) is nn.Conv2d
    after, after_b = dict(tree.named_parameters()), dict(tree.named_buffers())
    assert list(after) == list(params) and all(after[k] is params[k] for k in params)
    assert list(after_b) == list(buffers) and all(after_b[k] is buffers[k] for k in buffers)
    assert list(tree.state_dict()) == keys
    assert tree.bn1.relu is False
    again, skipped2 = norm.use_hip_norms(tree)
    assert again == [] and skipped2 == skipped
    # a lone layer is converted too (the root module itself)
    lone = nn.BatchNorm2d(4)
    assert norm.use_hip_norms(lone) == ([""], {}) and type(lone) is norm.BatchNorm2d
    # use_hip_convs and use_hip_norms do not see each other's layers
    from centerpose_amd import conv

    assert conv.use_hip_convs(tree)[0] == ["conv1", "block.0"] and type(tree.bn1) is norm.BatchNorm2d
