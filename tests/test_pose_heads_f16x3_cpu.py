"""CPU tests (no GPU) of the PoseHeads backward's precision argument: the declarations of cp_pose_heads_backward_prec_*, their
host arithmetic and refusals, the Python switches, and the premises of the generators the GPU tests rest on
(tests/pose_heads_f16x3_cases.py)."""
import ctypes
import inspect
import os
import re

import pytest
import torch
from torch import nn

import __graft_entry__ as ge
from centerpose_amd import conv, hip, pose_heads
from centerpose_amd.pose_heads import PoseHeads
from tests import pose_heads_f16x3_cases as C
from tests import pose_heads_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_pose_heads_backward_prec_workspace_bytes", "cp_pose_heads_backward_prec", "cp_pose_heads_backward_prec_mask")
F32, F16X3 = 0, 1


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def _classes(classes):
    return len(classes), (ctypes.c_int * len(classes))(*classes)


def test_symbols_declared_exported_and_listed(built):
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", text))
    for name in NEW + ("cp_pose_heads_backward_workspace_bytes", "cp_pose_heads_backward"):
        assert name in declared and hasattr(built, name) and name in hip.exported_symbols(), name
    assert int(re.search(r"#define\s+CP_ABI_VERSION\s+(\d+)", header).group(1)) == 7 == built.cp_abi_version() == hip.ABI_VERSION
    assert "Backward arithmetic is exact float32" in header   # the old call keeps its meaning
    assert "pose_dla_dcn.py:491-521" in header.split("cp_pose_heads_backward_prec_*")[1].split("*/")[0]


def test_f32_query_is_the_old_query_and_f16x3_is_larger(built):
    old, new = built.cp_pose_heads_backward_workspace_bytes, built.cp_pose_heads_backward_prec_workspace_bytes
    for name, (B, Cin, hid, H, W, classes) in R.DYADIC_SHAPES.items():
        n, cls = _classes(classes)
        a = old(B, H, W, Cin, hid, n, cls)
        assert new(B, H, W, Cin, hid, n, cls, F32) == a > 0, name
        chunk = built.cp_pose_heads_chunk_images(B, H, W, hid)
        # on top: the split copies of the hidden chunk and of the whole feature map, the packs, two slot blocks
        extra = new(B, H, W, Cin, hid, n, cls, F16X3) - a
        assert extra > 4 * chunk * H * W * hid + 4 * B * H * W * Cin, name
    n, cls = _classes(R.DLA_CLASSES)
    for g in ((128, 128, 64, 256), (128, 128, 64, 64), (13, 19, 32, 96)):
        sizes = [new(B, *g, n, cls, F16X3) for B in (1, 2, 3, 8, 16, 17, 32, 64)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], g
        assert all(new(B, *g, n, cls, F16X3) > new(B, *g, n, cls, F32) for B in (1, 16, 17))


def test_mask_is_host_arithmetic(built):
    mask = built.cp_pose_heads_backward_prec_mask
    for name, (seed, B, Cin, hid, H, W, classes) in C.STRICT_SHAPES.items():
        for _ in range(2):   # deterministic
            assert mask(B, H, W, Cin, hid, F16X3) == C.MASK_ALL and mask(B, H, W, Cin, hid, F32) == 0, name
        assert hip.ops.pose_heads_backward_precision_mask(B, H, W, Cin, hid) == C.MASK_ALL
        assert hip.ops.pose_heads_backward_precision_mask(B, H, W, Cin, hid, precision="f32") == 0
    for B, Cin, hid, H, W, _ in list(C.TWO_LEVEL_SHAPES.values()) + [(17, 64, 256, 128, 128, None)]:
        assert mask(B, H, W, Cin, hid, F16X3) == C.MASK_ALL
    # a chunk of feature maps beyond the 32-bit byte offsets of the f16x3 implicit GEMM: the hidden layer stays float32, the two
    # gradients (their operand is the hidden chunk, at most 256 MiB) do not
    assert built.cp_pose_heads_chunk_images(128, 128, 128, 32) == 128
    assert 128 * 128 * 128 * 512 * 4 >= 0xf0000000 and 128 * 128 * 128 * 512 < 2 ** 31
    assert mask(128, 128, 128, 512, 32, F16X3) == 3 and mask(64, 128, 128, 512, 32, F16X3) == C.MASK_ALL
    with pytest.raises(RuntimeError, match="Cin must be"):
        hip.ops.pose_heads_backward_precision_mask(2, 16, 16, 48, 64)
    with pytest.raises(ValueError, match="precision"):
        hip.ops.pose_heads_backward_precision_mask(2, 16, 16, 64, 64, precision="bf16")


REFUSED = [((0, 16, 16, 64, 64), b"at least 1"), ((2, 0, 16, 64, 64), b"at least 1"), ((2, 16, 0, 64, 64), b"at least 1"),
           ((2, 16, 16, 48, 64), b"Cin must be"), ((2, 16, 16, 0, 64), b"Cin must be"), ((2, 16, 16, 64, 40), b"hidden width"),
           ((2, 16, 16, 64, 0), b"hidden width"), ((64, 1024, 1024, 64, 64), b"2^31 elements")]


def test_refusals_without_a_device(built):
    """Every refusal of the float32 call, in both precisions, an unknown precision, and a workspace one block short: before any
    launch (no device is touched; the placeholder pointers are never dereferenced)."""
    q, call, mask = built.cp_pose_heads_backward_prec_workspace_bytes, built.cp_pose_heads_backward_prec, built.cp_pose_heads_backward_prec_mask
    p = ctypes.c_void_p(0x1000)
    n, cls = _classes((2, 16))
    tab = (ctypes.c_void_p * n)(0x1000, 0x1000)
    hole = (ctypes.c_void_p * n)(0x1000, None)
    none = ctypes.cast(None, ctypes.POINTER(ctypes.c_void_p))
    ok = (2, 16, 16, 64, 64)

    def bwd(feat=p, w0=tab, b0=tab, w1=tab, b1=tab, classes=cls, go=tab, gw0=tab, gb0=tab, gw1=tab, gb1=tab, gf=p, geo=ok, prec=F16X3,
            ws=p, nbytes=1 << 40, heads=n):
        return call(None, feat, heads, w0, b0, w1, b1, classes, go, gw0, gb0, gw1, gb1, gf, *geo, prec, ws, nbytes)

    for prec in (F32, F16X3):
        for geo, text in REFUSED:
            assert q(*geo, n, cls, prec) == 0 and text in built.cp_last_error(), (geo, built.cp_last_error())
            assert mask(*geo, prec) == hip.CP_ERR_INVALID and text in built.cp_last_error(), (geo, built.cp_last_error())
            assert bwd(geo=geo, prec=prec) == hip.CP_ERR_INVALID and text in built.cp_last_error(), (geo, built.cp_last_error())
        bad_cls = _classes((2, 65))[1]
        assert q(*ok, n, bad_cls, prec) == 0 and b"classes must be" in built.cp_last_error()
        assert bwd(classes=bad_cls, prec=prec) == hip.CP_ERR_INVALID and b"classes must be" in built.cp_last_error()
        assert q(*ok, 0, cls, prec) == 0 and bwd(heads=0, prec=prec) == hip.CP_ERR_INVALID
    for prec in (-1, 2, 7):
        assert q(*ok, n, cls, prec) == 0 and b"unknown precision" in built.cp_last_error()
        assert mask(*ok, prec) == hip.CP_ERR_INVALID and b"unknown precision" in built.cp_last_error()
        assert bwd(prec=prec) == hip.CP_ERR_INVALID and b"unknown precision" in built.cp_last_error()
    for prec in (F32, F16X3):
        need = q(*ok, n, cls, prec)
        assert need > 0
        for kw in (dict(feat=None), dict(w0=none), dict(b1=none), dict(go=none), dict(gw0=none), dict(gb1=none), dict(ws=None),
                   dict(w1=hole), dict(gb0=hole)):
            assert bwd(prec=prec, nbytes=need, **kw) == hip.CP_ERR_INVALID and b"null argument" in built.cp_last_error(), kw
        assert bwd(prec=prec, nbytes=need - 1) == hip.CP_ERR_INVALID and b"workspace too small" in built.cp_last_error()
        assert bwd(prec=prec, nbytes=need - 256) == hip.CP_ERR_INVALID and b"workspace too small" in built.cp_last_error()
    # the float32 workspace does not serve the f16x3 call
    assert bwd(nbytes=q(*ok, n, cls, F32)) == hip.CP_ERR_INVALID and b"workspace too small" in built.cp_last_error()


def test_python_switches():
    case = R.dyadic_case(0, 1, 32, 32, 4, 4, (1,))
    with pytest.raises(ValueError, match="precision"):
        hip.ops.pose_heads_backward_prec(case.feat, case.params, case.grad_outs, precision="fp8")
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.ops.pose_heads_backward_prec(case.feat, case.params, case.grad_outs, precision="f16x3")
    # hip.pose_heads_backward keeps its signature; the precision is the argument of ops.pose_heads_backward_prec
    old, new = inspect.signature(hip.pose_heads_backward).parameters, inspect.signature(hip.ops.pose_heads_backward_prec).parameters
    assert list(new) == list(old) + ["precision"] and new["precision"].default == "f32"
    assert all(new[k].default == old[k].default for k in old)
    assert not hasattr(hip, "pose_heads_backward_prec") and not hasattr(hip, "pose_heads_backward_precision_mask")
    assert inspect.signature(hip.ops.pose_heads_backward_precision_mask).parameters["precision"].default == "f16x3"

    heads = {"hm": 1, "wh": 2}
    assert PoseHeads(heads, 64, 64).backward_precision == "f32"
    assert PoseHeads(heads, 64, 64, backward_precision="f16x3").backward_precision == "f16x3"
    with pytest.raises(ValueError, match="backward_precision"):
        PoseHeads(heads, 64, 64, backward_precision="bf16")
    assert "backward_precision" not in "".join(PoseHeads(heads, 64, 64, backward_precision="f16x3").state_dict())

    # a tree with two PoseHeads and some Conv2d: each switch counts and touches its own kind only
    tree = nn.Sequential(conv.Conv2d(8, 64, 3, padding=1), PoseHeads(heads, 64, 64),
                         nn.Sequential(conv.Conv2d(64, 64, 1), nn.ReLU(), PoseHeads({"hm": 1}, 64, 32)), nn.Conv2d(4, 4, 1))
    assert pose_heads.set_backward_precision(tree, "f16x3") == 2
    assert tree[1].backward_precision == tree[2][2].backward_precision == "f16x3"
    assert tree[0].backward_precision == tree[2][0].backward_precision == "f32" and not hasattr(tree[3], "backward_precision")
    assert conv.set_backward_precision(tree, "f16x3") == 2
    assert pose_heads.set_backward_precision(tree, "f32") == 2
    assert tree[1].backward_precision == tree[2][2].backward_precision == "f32"
    assert tree[0].backward_precision == tree[2][0].backward_precision == "f16x3"
    assert conv.set_backward_precision(tree, "f32") == 2 and tree[1].backward_precision == "f32"
    assert pose_heads.set_backward_precision(tree[1], "f16x3") == 1 and tree[2][2].backward_precision == "f32"   # itself included
    assert pose_heads.set_backward_precision(nn.ReLU(), "f16x3") == 0
    with pytest.raises(ValueError, match="backward_precision"):
        pose_heads.set_backward_precision(tree, "bf16")
    # a mistyped attribute is refused at the forward, before any launch
    tree[1].backward_precision = "fp8"
    with pytest.raises(ValueError, match="backward_precision"):
        tree[1](case.feat.repeat(1, 2, 1, 1))


def test_switch_reaches_the_nets_that_hold_their_heads():
    """PoseNet keeps its PoseHeads outside the sub-module tree; PoseNetHourglass runs the heads' function on its own parameters."""
    from centerpose_amd.pose_net import PoseNet
    from centerpose_amd.pose_net_hourglass import PoseNetHourglass

    net = PoseNet({"hm": 1, "wh": 2}, 64)
    assert net._head_block.backward_precision == "f32"
    assert pose_heads.set_backward_precision(net, "f16x3") == 1 and net._head_block.backward_precision == "f16x3"
    assert all(m.backward_precision == "f32" for m in net.modules() if isinstance(m, conv.Conv2d))
    n_conv = conv.set_backward_precision(net, "f16x3")
    assert n_conv > 10 and net._head_block.backward_precision == "f16x3"
    assert pose_heads.set_backward_precision(net, "f32") == 1 and net._head_block.backward_precision == "f32"
    hg = PoseNetHourglass({"hm": 1}, n=1, dims=[256, 256], modules=[1, 1], num_stacks=2)
    assert hg.heads_backward_precision == "f32"
    assert pose_heads.set_backward_precision(hg, "f16x3") == 1 and hg.heads_backward_precision == "f16x3"
    assert "heads_backward_precision" in vars(hg) and PoseNetHourglass.heads_backward_precision == "f32"
    assert conv.set_backward_precision(hg, "f32") > 0 and hg.heads_backward_precision == "f16x3"


def test_cases_cover_what_they_should():
    assert set(R.DYADIC_SHAPES) - set(C.STRICT_SHAPES) == {"dla_128"} and set(R.SHARED_CONV_CASES) <= set(C.STRICT_SHAPES)
    ks = [v for k, v in C.STRICT_SHAPES.items() if k.startswith("kstep")]
    assert sorted(v[5] for v in ks) == [15, 16, 17, 31, 33] and all(v[1:5] == (1, 32, 64, 5) and v[6] == (2,) for v in ks)
    assert {v[3] % 128 == 0 for v in C.STRICT_SHAPES.values()} == {True, False}
    assert list(C.TWO_LEVEL_SHAPES.values()) == [(1, 32, 64, 9, 7, (1,)), (2, 64, 256, 5, 3, (1,)), (1, 32, 32, 16, 17, (4,))]
    assert all(C.two_level_ok(s) for s in C.TWO_LEVEL_SHAPES.values())
    assert not C.two_level_ok((1, 32, 64, 64, 64, (1,))) and not C.two_level_ok((1, 32, 512, 4, 4, (1,)))


@pytest.mark.parametrize("name", sorted(C.STRICT_SHAPES))
def test_strict_generator(name):
    """pose_heads_ref.check_dyadic on every strict case and seed of the GPU file (asserted inside dyadic_case), and: feat and w0
    have no lo part under the device's scale and split."""
    case = C.cached_case("strict", name)
    R.check_dyadic(case)
    assert not C.split_is_exact(case.feat)
    for w0, _, _, _ in case.params:
        assert not C.split_is_exact(w0)
    for h, _ in C.grad_hidden64(case):
        assert not bool((h == 0).any())


@pytest.mark.parametrize("kind", C.TWO_LEVEL_KINDS)
@pytest.mark.parametrize("name", sorted(C.TWO_LEVEL_SHAPES))
def test_two_level_generator(name, kind):
    shape = C.TWO_LEVEL_SHAPES[name]
    case = C.cached_case("two_" + kind, name)
    C.check_two_level(case, shape, kind)
    ref = C.cached_reference("two_" + kind, name)
    # the float64 reference of a two-level case is not the reference of its coarse parts: the cross terms carry weight
    coarse = R.reference(case.feat.round(), case.params, [g.round() for g in case.grad_outs])
    assert not torch.equal(ref["grads"][0][0], coarse["grads"][0][0])
    if kind == "go":
        assert not torch.equal(ref["gfeat"], coarse["gfeat"])
    # ... float32 autograd reproduces the four exact gradients: their sums are exact in float32 in any order
    x = case.feat.clone().requires_grad_(True)
    ps = [t.clone().requires_grad_(True) for t in case.params[0]]
    out = torch.nn.functional.conv2d(torch.relu(torch.nn.functional.conv2d(x, ps[0], ps[1], padding=1)), ps[2], ps[3])
    (out * case.grad_outs[0]).sum().backward()
    for got, exp in ((x.grad, ref["gfeat"]), (ps[0].grad, ref["grads"][0][0]), (ps[1].grad, ref["grads"][0][1]), (ps[3].grad, ref["grads"][0][3])):
        assert torch.equal(got.double(), exp)
    # ... and the hand-written float64 backward agrees with autograd
    man = R.manual_backward64(case.feat, case.params, case.grad_outs)
    assert torch.equal(man["gfeat"], ref["gfeat"]) and all(torch.equal(a, b) for a, b in zip(man["grads"][0], ref["grads"][0]))


@pytest.mark.parametrize("arch", sorted(C.REALISTIC))
def test_realistic_case_condition(arch):
    """The share of hidden units inside the widened ambiguity threshold, for the float64 reference alone, is within the cap."""
    case = C.cached_case("realistic", arch)
    ref = C.cached_reference("realistic", arch)
    wide = C.f16x3_allowance(case.feat, case.params, case.grad_outs, ref["hidden"])
    base = R.allowance(case.feat, case.params, case.grad_outs, ref["hidden"])
    print("%s: ambiguous share %.3e (float32 threshold: %.3e; cap %.0e)" % (arch, wide["share"], base["share"], R.AMBIGUOUS_CAP))
    assert base["share"] <= wide["share"] <= R.AMBIGUOUS_CAP
    assert bool((wide["gfeat"] >= base["gfeat"]).all())
    assert float(case.feat.min()) == 0.0 and 0.2 < float((case.feat == 0).float().mean()) < 0.8
    man = R.manual_backward64(case.feat, case.params, case.grad_outs)
    for a, b in zip(man["grads"], ref["grads"]):
        for x, y in zip(a, b):
            assert float((x - y).abs().max()) <= 1e-9 * float(y.abs().max())


@pytest.mark.parametrize("name", ["dla_32", "ragged_13x19", "resdcn"])
def test_gaussian_cases_condition(name):
    """The Gaussian cases of the GPU file: about half of the hidden units active, the ambiguous share within the cap."""
    case = C.cached_case("gauss", name)
    ref = C.cached_reference("gauss", name)
    for h, _ in C.grad_hidden64(case):
        assert 0.3 <= float((h > 0).double().mean()) <= 0.7
    assert C.f16x3_allowance(case.feat, case.params, case.grad_outs, ref["hidden"])["share"] <= R.AMBIGUOUS_CAP
