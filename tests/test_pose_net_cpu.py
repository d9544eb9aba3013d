"""CPU tests (no GPU) of the trainable network and its two new layer families: the C ABI's declarations and refusals
(cp_maxpool2d_*, cp_conv2d_stem_backward*), PoseNet's state dict and its round trip through HipPoseNet, the re-class contract of
use_hip_pools / use_hip_stems, and the reference the GPU test rests on (tests/pose_net_ref.py): pinned to the oracle in
evaluation mode, and well conditioned in float32 for the very case the GPU test runs."""
import json
import os
import re

import pytest
import torch
from torch import nn

import __graft_entry__ as ge
from centerpose_amd import hip, pool, stem, synth
from centerpose_amd.lib.models.model import create_model
from centerpose_amd.pose_net import PoseNet
from tests import pose_net_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_maxpool2d_forward_nhwc", "cp_maxpool2d_backward_nhwc", "cp_conv2d_stem_backward_workspace_bytes",
       "cp_conv2d_stem_backward")


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


class _Opt:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_symbols_declared_exported_and_listed(built):
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    testing = open(os.path.join(REPO, "include", "centerpose_hip_testing.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and hasattr(built, name) and name in hip.exported_symbols(), name
        assert name not in testing
    assert int(re.search(r"#define\s+CP_ABI_VERSION\s+(\d+)", header).group(1)) == 7 == built.cp_abi_version()
    for cite in ("pose_dla_dcn.py:211-224", "pose_dla_dcn.py:247-271", "resnet_dcn.py"):
        assert cite in header


def test_refusals_before_any_launch(built):
    """Shape errors are found on the host (there is no device here): code, text, and a zero workspace query."""
    q = built.cp_conv2d_stem_backward_workspace_bytes
    assert q(2, 64, 96, 3, 16, 1) > 0 and q(2, 64, 96, 1, 64, 2) > 0
    for geo, word in (((2, 64, 96, 4, 16, 1), b"Cin"), ((2, 64, 96, 0, 16, 1), b"Cin"), ((2, 64, 96, 3, 24, 1), b"Cout"),
                      ((2, 64, 96, 3, 128, 1), b"Cout"), ((2, 64, 96, 3, 16, 3), b"stride"), ((0, 64, 96, 3, 16, 1), b"at least 1"),
                      ((64, 4096, 4096, 3, 16, 1), b"2^31")):
        assert q(*geo) == 0 and word in built.cp_last_error(), geo
    # the query is host arithmetic: slabs of [Cout][49 Cin + 1] floats, at most 512 of them, rounded to 256 bytes
    assert q(1, 8, 64, 3, 16, 1) == (1 * 16 * 148 * 4 + 255) // 256 * 256
    assert q(64, 512, 512, 3, 16, 1) == 512 * 16 * 148 * 4
    null = None
    assert built.cp_conv2d_stem_backward(null, null, null, null, null, null, null, 0, 2, 64, 96, 3, 16, 1) == -1
    assert b"null" in built.cp_last_error()
    for geo, word in (((1, 8, 8, 4, 2, 1, 0), b"geometry"), ((1, 8, 8, 4, 3, 2, 0), b"geometry"), ((1, 8, 8, 6, 2, 2, 0), b"multiple of 4"),
                      ((1, 1, 5, 4, 2, 2, 0), b"empty output"), ((0, 8, 8, 4, 2, 2, 0), b"at least 1")):
        assert built.cp_maxpool2d_forward_nhwc(null, null, null, *geo) == -1 and word in built.cp_last_error(), geo
        assert built.cp_maxpool2d_backward_nhwc(null, null, null, null, *geo) == -1 and word in built.cp_last_error(), geo
    assert built.cp_maxpool2d_forward_nhwc(null, null, null, 1, 1, 1, 4, 3, 2, 1) == -1 and b"null" in built.cp_last_error()


@pytest.mark.parametrize("tracking", [(False, False, False), (True, True, False), (True, True, True)], ids=["plain", "img_hm", "all"])
def test_state_dict_is_the_reference(built, tracking):
    heads = synth.HEADS_TRACK if all(tracking) else synth.HEADS_POSE
    opt = _Opt(pre_img=tracking[0], pre_hm=tracking[1], pre_hm_hp=tracking[2])
    net = PoseNet(heads, head_conv=256, opt=opt)
    sd = net.state_dict()
    spec = synth.param_spec("dla_34", heads, tracking, 256)
    assert list(sd) == list(spec)
    assert all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
    golden = json.load(open(os.path.join(REPO, "tests", "golden", "state_dict_keys.json")))
    if not any(tracking):
        assert {k: list(v.shape) for k, v in sd.items()} == {k: list(v) for k, v in golden["dla"].items()} and len(sd) == 414
    if all(tracking):
        assert {k: list(v.shape) for k, v in sd.items()} == {k: list(v) for k, v in golden["dla_track"].items()}
    # the reference's deterministic initial values
    for h in heads:
        last = getattr(getattr(net, h), "2").bias
        assert bool((last == (-2.19 if "hm" in h else 0.0)).all()), h
    assert torch.equal(net.ida_up.up_2.weight.detach(), synth._bilinear_up((64, 1, 8, 8)))
    assert all(float(m.conv.conv_offset_mask.weight.detach().abs().max()) == 0 for m in net.modules() if hasattr(m, "actf"))
    # the layers are the library's
    kinds = {type(m).__module__.split(".")[-1] for m in net.modules() if not list(m.children())}
    assert kinds == {"conv", "stem", "norm", "pool", "deconv", "pose_heads"}
    assert type(net.base.base_layer[0]) is stem.StemConv2d and type(net.base.level2.downsample) is pool.MaxPool2d
    # strict load of a reference-format checkpoint
    ref = synth.make_state_dict("dla_34", heads, tracking=tracking if any(tracking) else False, head_conv=256)
    net.load_state_dict(ref, strict=True)


def test_other_architectures_say_what_is_missing():
    for arch, word in (("dlav1_34", "ConvGRU"), ("hourglass", "hourglass"), ("resdcn_18", "ResNet-DCN")):
        with pytest.raises(NotImplementedError, match=word):
            PoseNet(synth.HEADS_POSE, arch=arch)
        m = create_model(arch, synth.HEADS_POSE, 256 if arch != "resdcn_18" else 64)
        with pytest.raises(NotImplementedError, match=word):
            m.train_module()


def test_round_trip_through_hip_pose_net(built):
    heads = synth.HEADS_POSE
    ref = synth.make_state_dict("dla_34", heads, head_conv=64)
    ref["base.level0.1.num_batches_tracked"] = torch.tensor(5)
    model = create_model("dla_34", heads, 64)
    model.load_state_dict(ref)
    with pytest.raises(NotImplementedError):
        model.train(True)  # unchanged: the engine itself does not train
    net = model.train_module()
    assert isinstance(net, PoseNet) and net.training
    other = create_model("dla_34", heads, 64)
    other.load_module(net)
    back = other.state_dict()
    assert list(back) == list(ref)
    for k in ref:
        assert back[k].dtype == ref[k].dtype and torch.equal(back[k], ref[k]), k
    # copies, not views: training the module does not reach into the model until load_module
    with torch.no_grad():
        net.base.level0[0].weight.add_(1.0)
    assert torch.equal(model.state_dict()["base.level0.0.weight"], ref["base.level0.0.weight"])
    with pytest.raises(RuntimeError, match="does not match"):
        create_model("dla_34", heads, 256).load_module(net)


def test_use_hip_pools_contract():
    class Mine(nn.MaxPool2d):
        pass

    net = nn.Sequential(nn.MaxPool2d(2, 2), nn.MaxPool2d(3, stride=2, padding=1), nn.MaxPool2d(2), nn.MaxPool2d((2, 2), (2, 2)),
                        nn.MaxPool2d(3, 2, 1, dilation=2), nn.MaxPool2d(2, 2, ceil_mode=True), nn.MaxPool2d(2, 2, return_indices=True),
                        nn.MaxPool2d(3, 1, 1), nn.MaxPool2d((2, 3), 2), Mine(2, 2), nn.AvgPool2d(2), nn.Conv2d(4, 4, 1))
    before = repr(net)
    converted, skipped = pool.use_hip_pools(net)
    assert converted == ["0", "1", "2", "3"]
    assert set(skipped) == {"4", "5", "6", "7", "8", "9"}
    for k, word in (("4", "dilation"), ("5", "ceil_mode"), ("6", "return_indices"), ("7", "geometry"), ("8", "geometry"), ("9", "subclass")):
        assert word in skipped[k], (k, skipped[k])
    assert skipped["9"] == "subclass Mine keeps its own forward"
    assert all(type(net[i]) is pool.MaxPool2d for i in range(4)) and type(net[4]) is nn.MaxPool2d and type(net[9]) is Mine
    assert repr(net) == before
    assert pool.use_hip_pools(net) == ([], skipped)   # idempotent: converted layers appear in neither
    with pytest.raises(NotImplementedError, match="ceil_mode"):
        pool.MaxPool2d(2, 2, ceil_mode=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        net[0](torch.zeros(1, 4, 4, 4))


def test_use_hip_stems_contract():
    class Mine(nn.Conv2d):
        pass

    net = nn.Sequential(nn.Conv2d(3, 16, 7, padding=3, bias=False), nn.Conv2d(1, 16, 7, padding=3), nn.Conv2d(3, 64, 7, stride=2, padding=3),
                        nn.Conv2d(4, 16, 7, padding=3), nn.Conv2d(3, 16, 3, padding=1), nn.Conv2d(3, 24, 7, padding=3),
                        nn.Conv2d(3, 16, 7, stride=4, padding=3), nn.Conv2d(3, 16, 7, padding=2), Mine(3, 16, 7, padding=3),
                        nn.Conv2d(3, 128, 7, padding=3), nn.BatchNorm2d(16))
    params = [p for p in net.parameters()]
    keys, before = list(net.state_dict()), repr(net)
    converted, skipped = stem.use_hip_stems(net)
    assert converted == ["0", "1", "2"] and skipped == {}
    assert all(type(net[i]) is stem.StemConv2d for i in range(3))
    assert all(type(net[i]) is nn.Conv2d for i in (3, 4, 5, 6, 7, 9)) and type(net[8]) is Mine
    assert all(a is b for a, b in zip(params, net.parameters())) and list(net.state_dict()) == keys and repr(net) == before
    assert stem.use_hip_stems(net) == ([], {})
    assert net[0].relu is False
    with pytest.raises(NotImplementedError):
        stem.StemConv2d(4, 16, 7, padding=3)
    with pytest.raises(RuntimeError, match="HIP device"):
        net[0](torch.zeros(1, 3, 8, 8))
    # use_hip_convs keeps skipping the stems with its own reason
    from centerpose_amd import conv
    plain = nn.Sequential(nn.Conv2d(3, 16, 7, padding=3))
    assert "multiple of 4" in conv.use_hip_convs(plain)[1]["0"]


def test_reference_eval_mode_equals_the_oracle():
    """tests/pose_net_ref.py in evaluation mode against oracle.backbone.dlaseg_forward (float32, its own C im2col) on a random
    state dict at 64 x 64.  Bound: 1e-4 x max |oracle| per head, the project's tolerance between two float32 evaluations of
    this graph (the float64 restatement itself is exact to 1e-12)."""
    from oracle import backbone as ob

    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("dla_34", heads, head_conv=64)
    x = synth.frames(1, seed=3, h=64, w=64)
    zo = ob.dlaseg_forward(sd, x, heads)
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        z = R.forward(sd64, x.double(), heads, False)
    assert list(z) == list(zo)
    for h in heads:
        err = float((z[h] - zo[h].double()).abs().max())
        assert err <= 1e-4 * float(zo[h].abs().max()), (h, err)
    assert all(int(v) == 0 for k, v in sd64.items() if k.endswith("num_batches_tracked"))  # evaluation touches no buffer


@pytest.mark.parametrize("tracking", [False, True], ids=["plain", "pre_img_pre_hm"])
def test_reference_case_is_well_conditioned(tracking):
    """The GPU test's case (tests/pose_net_ref.py: seed, shape, state dict) evaluated in float32 on the CPU: every parameter
    gradient within 1e-4 x max |float64 gradient| (a tenth of the GPU test's limit), the outputs within 1e-4 x max likewise.
    A case that fails this is replaced HERE (seed, size), never by looking at the device's result."""
    sd, inp, r64 = R.reference_case(tracking)
    r32 = R.run(sd, *inp, torch.float32)
    assert list(r64.grads) == [k for k, v in sd.items() if v.is_floating_point() and "running_" not in k]
    for h in r64.z:
        assert float((r32.z[h].double() - r64.z[h]).abs().max()) <= 1e-4 * float(r64.z[h].abs().max()), h
    for k, g in r64.grads.items():
        if g is None:
            assert R.unused(k) and r32.grads[k] is None, k
            continue
        assert not R.unused(k), k
        scale = float(r64.grads[R.companion_weight(k)].abs().max()) if R.is_pre_bn_bias(k) else float(g.abs().max())
        assert scale > 0, k
        err = float((r32.grads[k].double() - g).abs().max())
        assert err <= 1e-4 * scale, (k, err, scale)
    # offsets: fractional, inside +-0.5, away from zero -- the premise of comparing the offset convolutions' gradients
    for k, b in sd.items():
        if k.endswith("conv_offset_mask.bias"):
            assert 0.15 <= float(b[:18].abs().min()) and float(b[:18].abs().max()) <= 0.35
    # every BatchNorm the graph uses ran once; the two-level trees' own project layers never do
    for k, v in r64.buffers.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == (0 if R.unused(k) else 1), k
