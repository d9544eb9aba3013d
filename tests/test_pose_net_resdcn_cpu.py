"""CPU tests (no GPU) of ``centerpose_amd.pose_net_resdcn.PoseNetResDCN``: the module tree's keys, shapes and order for all five
depths, strict loading, the from_model / load_module round trip, the refusals, the backward-precision walkers' counts, and the
reference helper tests/resdcn_net_ref.py: its evaluation mode against tests/resdcn_ref.py and the conditioning of the case
tests/test_pose_net_resdcn_gpu.py uses."""
import json
import os

import pytest
import torch
from torch import nn

from centerpose_amd import conv, deconv, norm, pool, pose_heads, stem, synth
from centerpose_amd.lib.models.model import create_model
from centerpose_amd.lib.models.networks.DCNv2 import dcn_v2
from centerpose_amd.pose_net import PoseNet
from centerpose_amd.pose_net_resdcn import PoseNetResDCN
from tests import resdcn_net_ref as N
from tests.resdcn_ref import torch_resdcn_forward

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_dict_keys_resdcn.json")
GPU_LIMIT = 1e-3    # tests/test_pose_net_resdcn_gpu.py


@pytest.mark.parametrize("depth", sorted(synth.RESNET_SPEC))
def test_state_dict_is_the_reference_record(depth):
    with open(GOLD) as f:
        want = json.load(f)["resdcn_%d" % depth]
    net = PoseNetResDCN(depth, synth.HEADS_POSE, head_conv=64)
    assert net.arch == "resdcn_%d" % depth and PoseNetResDCN.arch == "resdcn_%d"
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == want
    assert list(net.state_dict()) == list(synth.param_spec("resdcn_%d" % depth, synth.HEADS_POSE, head_conv=64))
    sd = synth.make_state_dict("resdcn_%d" % depth)
    net.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    # the deconv stack's indices: parameters under 0, 1, 3, 4 (mod 6), none under the ReLU slots
    idx = sorted({int(k.split(".")[1]) for k in net.state_dict() if k.startswith("deconv_layers.")})
    assert idx == [0, 1, 3, 4, 6, 7, 9, 10, 12, 13, 15, 16] and len(net.deconv_layers) == 18
    # every layer is the library's
    heads = tuple(synth.HEADS_POSE)
    kinds = {type(m) for n, m in net.named_modules() if n.split(".")[0] not in heads and (not list(m.children()) or isinstance(m, dcn_v2.DCN))}
    assert kinds == {stem.StemConv2d, conv.Conv2d, norm.BatchNorm2d, pool.MaxPool2d, dcn_v2.DCN, deconv.ConvTranspose2d, nn.Identity}, kinds
    assert type(net.conv1) is stem.StemConv2d and type(net.maxpool) is pool.MaxPool2d
    assert all(type(net.deconv_layers[i]) is deconv.ConvTranspose2d for i in (3, 9, 15))
    assert all(type(net.deconv_layers[i].conv_offset_mask) is conv.Conv2d for i in (0, 6, 12))
    assert net.bn1.relu and net.layer1[0].bn2.relu and not net.layer2[0].downsample[1].relu and net.deconv_layers[16].relu


class _Opt:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_round_trip_with_the_engine_model():
    model = create_model("resdcn_18", synth.HEADS_POSE, 64, _Opt(precision="f32"))
    net = PoseNetResDCN.from_model(model)
    assert type(net) is PoseNetResDCN and net.arch == "resdcn_18" and net.head_conv == 64
    sd = model.state_dict()
    assert list(net.state_dict()) == list(sd) and all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    with torch.no_grad():
        net.layer3[0].bn1.running_mean += 0.5
        net.bn1.num_batches_tracked += 7
        net.deconv_layers[0].bias += 0.25          # the DCN bias the engine folds into the next BatchNorm's shift
        getattr(net.hm, "2").bias -= 1.0
    assert model.load_module(net) is model
    sd2 = model.state_dict()
    assert torch.equal(sd2["layer3.0.bn1.running_mean"], sd["layer3.0.bn1.running_mean"] + 0.5)
    assert int(sd2["bn1.num_batches_tracked"]) == int(sd["bn1.num_batches_tracked"]) + 7
    assert torch.equal(sd2["deconv_layers.0.bias"], sd["deconv_layers.0.bias"] + 0.25)
    assert torch.equal(sd2["hm.2.bias"], sd["hm.2.bias"] - 1.0)
    again = PoseNetResDCN.from_model(model).state_dict()
    assert all(torch.equal(v, again[k]) for k, v in net.state_dict().items())
    # a net of another depth or head width does not fit
    with pytest.raises(RuntimeError, match="does not match"):
        model.load_module(PoseNetResDCN(34, synth.HEADS_POSE, 64))
    with pytest.raises(RuntimeError, match="does not match"):
        model.load_module(PoseNetResDCN(18, synth.HEADS_POSE, 32))
    for arch, hc in (("dla_34", 256), ("hourglass", 256)):
        with pytest.raises(NotImplementedError, match="not resdcn"):
            PoseNetResDCN.from_model(create_model(arch, synth.HEADS_POSE, hc))


def test_refusals():
    for depth in (20, 0, "18"):
        with pytest.raises(NotImplementedError, match="depth must be one of"):
            PoseNetResDCN(depth, synth.HEADS_POSE)
    for hc in (0, 48, -32, 16):
        with pytest.raises(NotImplementedError, match="head_conv must be a positive multiple of 32"):
            PoseNetResDCN(18, synth.HEADS_POSE, head_conv=hc)
    with pytest.raises(ValueError, match="collides"):
        PoseNetResDCN(18, {"hm": 1, "layer1": 2})
    net = PoseNetResDCN(18, {"hm": 1, "wh": 2})
    for shape in ((1, 3, 64, 80), (1, 3, 48, 64)):
        with pytest.raises(NotImplementedError, match="multiples of 32"):
            net(torch.zeros(shape))
    with pytest.raises(RuntimeError, match=r"\[B,3,H,W\]"):
        net(torch.zeros(1, 4, 64, 64))
    with pytest.raises(RuntimeError, match="HIP device"):
        net(torch.zeros(1, 3, 64, 64))


def test_the_old_entry_points_still_refuse_and_name_the_class():
    with pytest.raises(NotImplementedError, match="ResNet-DCN") as e:
        PoseNet(synth.HEADS_POSE, arch="resdcn_18")
    assert "PoseNetResDCN.from_model" in str(e.value) and "load_module" in str(e.value)
    with pytest.raises(NotImplementedError, match="ResNet-DCN") as e:
        create_model("resdcn_18", synth.HEADS_POSE, 64).train_module()
    assert "PoseNetResDCN.from_model" in str(e.value)


def test_backward_precision_walkers():
    net = PoseNetResDCN(50, synth.HEADS_POSE)
    convs = sum(type(m) is conv.Conv2d for m in net.modules())
    assert convs == 16 * 3 + 4 + 3                  # bottleneck convolutions, down-samples, conv_offset_mask
    for name in ("f16x3", "f32"):
        assert conv.set_backward_precision(net, name) == convs
        assert deconv.set_backward_precision(net, name) == 3
        assert dcn_v2.set_backward_precision(net, name) == 3
        assert pose_heads.set_backward_precision(net, name) == 1
        assert all(net.deconv_layers[i].backward_precision == name for i in (3, 9, 15))
    for mod in (conv, deconv, dcn_v2, pose_heads):
        with pytest.raises(ValueError, match="backward_precision must be one of"):
            mod.set_backward_precision(net, "bf16")


@pytest.mark.parametrize("depth", N.DEPTHS)
def test_reference_eval_mode_is_the_oracle_restatement(depth):
    sd, (x, _), _ = N.reference_case(depth)
    with torch.no_grad():
        got = N.forward({k: v.double() if v.is_floating_point() else v.clone() for k, v in sd.items()}, x.double(), depth,
                        synth.HEADS_POSE, False)
        want = torch_resdcn_forward(sd, x, depth, synth.HEADS_POSE, dtype=torch.float64)
    for h in synth.HEADS_POSE:
        assert float((got[h] - want[h]).abs().max()) <= 1e-12 * float(want[h].abs().max()), h


@pytest.mark.parametrize("depth", N.DEPTHS)
def test_the_gpu_case_is_well_conditioned(depth):
    """float32 on the CPU stays within a tenth of the GPU test's limits against float64, and the zero-gradient-bias rule picks
    the biases it is meant for."""
    sd, inp, r64 = N.reference_case(depth)
    assert inp[0].shape == (2, 3, 64, 96) and N.HEAD_CONV == 32 and N.SEED == 11
    zero = N.zero_gradient_biases(r64)
    assert len(zero) == {18: 3, 50: 18}[depth]
    assert {"deconv_layers.%d.bias" % i for i in (0, 6, 12)} <= set(zero)
    out, fam, stat = N.compare(N.run(sd, depth, *inp, torch.float32), r64)
    print("resdcn_%d float32 CPU: outputs %.2e, running statistics %.2e, gradients %s" % (
        depth, out, stat, {f: "%.2e (%s)" % v for f, v in fam.items()}))
    assert set(fam) == set(N.FAMILIES)
    assert out <= GPU_LIMIT / 10 and stat <= GPU_LIMIT / 10
    assert max(e for e, _ in fam.values()) <= GPU_LIMIT / 10, fam
    assert all(int(v) == 1 for k, v in r64.buffers.items() if k.endswith("num_batches_tracked"))
    # every gate is exercised: some ReLU inputs of the last BatchNorm are negative, and the float64 loss depends on every parameter
    assert all(float(g.abs().max()) > 0 or k in zero for k, g in r64.grads.items())


def test_sync_batchnorm_walker_takes_every_batchnorm():
    """data_parallel.DataParallel(net, sync_batchnorm=True) re-classes through sync_norm.use_hip_sync_norms: every BatchNorm of the
    net, with its fused ReLU kept, and the keys unchanged."""
    from centerpose_amd import sync_norm

    net = PoseNetResDCN(18, synth.HEADS_POSE)
    keys = list(net.state_dict())
    bns = [n for n, m in net.named_modules() if type(m) is norm.BatchNorm2d]
    assert len(bns) == 1 + 16 + 3 + 6      # bn1, two per BasicBlock, the three down-samples, the deconv stack
    converted, skipped = sync_norm.use_hip_sync_norms(net, object())
    assert converted == bns and skipped == {}
    assert type(net.layer2[0].downsample[1]) is sync_norm.SyncBatchNorm and not net.layer2[0].downsample[1].relu
    assert net.bn1.relu and net.deconv_layers[16].relu and list(net.state_dict()) == keys
