"""CPU tests (no GPU) of ``centerpose_amd.pose_net_gru.PoseNetGRU``: its state dict against the reference's, its round trip
through HipPoseNet, and the reference the GPU test rests on (tests/pose_net_gru_ref.py): pinned to the oracle in evaluation
mode -- which ties the GRU steps, the routing and the GroupNorm grouping to the reference module -- and well conditioned in
float32 for the very cases the GPU test runs."""
import pytest
import torch

import __graft_entry__ as ge
from centerpose_amd import conv, conv_gru, group_norm, hip, synth
from centerpose_amd.lib.models.model import create_model
from centerpose_amd.pose_net import PoseNet
from centerpose_amd.pose_net_gru import PoseNetGRU
from tests import pose_net_gru_ref as R
from tests import pose_net_ref as P


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


class _Opt:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _opt(tracking):
    return _Opt(tracking_task=tracking, pre_img=tracking, pre_hm=tracking, pre_hm_hp=tracking)


@pytest.mark.parametrize("tracking", [False, True], ids=["plain", "tracking"])
@pytest.mark.parametrize("head_conv", [64, 256])
def test_state_dict_is_the_reference(built, tracking, head_conv):
    heads = R.heads_of(tracking)
    net = PoseNetGRU(heads, head_conv=head_conv, opt=_opt(tracking))
    sd = net.state_dict()
    spec = synth.param_spec("dlav1_34", heads, tracking, head_conv)
    assert list(sd) == list(spec)
    assert all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
    assert net.convGRU.step == (4 if tracking else 3)
    for h in heads:
        seq = getattr(net, h)
        assert type(seq[0]) is conv.Conv2d and type(seq[3]) is conv.Conv2d and seq[0].relu is False
        assert type(seq[1]) is group_norm.GroupNorm and seq[1].relu is True and seq[1].num_groups == 32
        if "hm" in h:   # pose_dla_dcn.py:509-510
            assert bool((seq[3].bias == -2.19).all()), h
    assert type(net.convGRU) is conv_gru.ConvGRU
    kinds = {type(m).__module__.split(".")[-1] for m in net.modules() if not list(m.children())}
    assert kinds == {"conv", "stem", "norm", "pool", "deconv", "group_norm", "linear"}   # (linear: nn.Identity, the absorbed ReLU)
    net.load_state_dict(synth.make_state_dict("dlav1_34", heads, tracking=tracking, head_conv=head_conv), strict=True)


def test_group_rule_and_refusals():
    from centerpose_amd import pose_net_gru

    assert [pose_net_gru.gn_groups(c) for c in (32, 64, 256, 48, 16)] == [32, 32, 32, 16, 16]
    # a head outside the routing table is refused at construction, as cp_model_create refuses it
    with pytest.raises(NotImplementedError, match="fed by no ConvGRU step"):
        PoseNetGRU({"hm": 1, "depth": 1}, 64)
    with pytest.raises(NotImplementedError, match="fed by no ConvGRU step"):
        PoseNetGRU({"hm": 1, "tracking": 2}, 64)            # routed only with tracking_task
    with pytest.raises(NotImplementedError, match="fed by no ConvGRU step"):
        PoseNetGRU({"hm": 1, "hps_uncertainty": 16}, 64)
    PoseNetGRU({"hm": 1, "tracking": 2, "hps_uncertainty": 16}, 64, _Opt(tracking_task=True))
    # PoseNet and train_module keep refusing dlav1 and say where to go
    with pytest.raises(NotImplementedError, match="PoseNetGRU"):
        PoseNet(synth.HEADS_POSE, arch="dlav1_34")
    with pytest.raises(NotImplementedError, match="PoseNetGRU.from_model"):
        create_model("dlav1_34", synth.HEADS_POSE, 256).train_module()
    with pytest.raises(NotImplementedError, match="not dlav1_34"):
        PoseNetGRU.from_model(create_model("dla_34", synth.HEADS_POSE, 256))
    with pytest.raises(RuntimeError, match="HIP device"):
        PoseNetGRU(synth.HEADS_POSE, 64)(torch.zeros(1, 3, 32, 32))


@pytest.mark.parametrize("tracking", [False, True], ids=["plain", "tracking"])
def test_round_trip_through_hip_pose_net(built, tracking):
    heads = R.heads_of(tracking)
    ref = synth.make_state_dict("dlav1_34", heads, tracking=tracking, head_conv=64)
    ref["base.level0.1.num_batches_tracked"] = torch.tensor(5)
    model = create_model("dlav1_34", heads, 64, _opt(tracking))
    model.load_state_dict(ref)
    net = PoseNetGRU.from_model(model)
    assert isinstance(net, PoseNetGRU) and net.training and net.tracking_task == tracking
    other = create_model("dlav1_34", heads, 64, _opt(tracking))
    other.load_module(net)
    back = other.state_dict()
    assert list(back) == list(ref)
    for k in ref:
        assert back[k].dtype == ref[k].dtype and torch.equal(back[k], ref[k]), k
    with torch.no_grad():
        net.convGRU.cell0.Wir.weight.add_(1.0)   # copies, not views
    assert torch.equal(model.state_dict()["convGRU.cell0.Wir.weight"], ref["convGRU.cell0.Wir.weight"])
    with pytest.raises(RuntimeError, match="does not match"):
        create_model("dlav1_34", heads, 256, _opt(tracking)).load_module(net)


@pytest.mark.parametrize("tracking", [False, True], ids=["plain", "tracking"])
def test_reference_eval_mode_equals_the_oracle(tracking):
    """tests/pose_net_gru_ref.py in evaluation mode against oracle.backbone.dlaseg_forward(arch='dlav1') (float32, pinned
    bit-exact to the reference module) at 64 x 64: 1e-5 x max |oracle| per head."""
    from oracle import backbone as ob

    heads = R.heads_of(tracking)
    sd = synth.make_state_dict("dlav1_34", heads, tracking=tracking, head_conv=256)
    x = synth.frames(1, seed=3, h=64, w=64)
    pre = {}
    if tracking:
        g = torch.Generator().manual_seed(5)
        pre = dict(pre_img=synth.frames(1, seed=4, h=64, w=64), pre_hm=torch.rand(1, 1, 64, 64, generator=g),
                   pre_hm_hp=torch.rand(1, 8, 64, 64, generator=g))
    zo = ob.dlaseg_forward(sd, x, heads, arch="dlav1", tracking_task=tracking, **pre)
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        z = R.forward(sd64, x.double(), heads, False, tracking, **{k: v.double() for k, v in pre.items()})
    assert list(z) == list(zo) == list(heads)
    for h in heads:
        err = float((z[h] - zo[h].double()).abs().max())
        print("%s: err %.3g of max %.3g" % (h, err, float(zo[h].abs().max())))
        assert err <= 1e-5 * float(zo[h].abs().max()), (h, err)
    assert all(int(v) == 0 for k, v in sd64.items() if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("tracking", [False, True], ids=["plain", "tracking"])
def test_reference_case_is_well_conditioned(tracking):
    """The GPU test's cases evaluated in float32 on the CPU: outputs, parameter gradients and running statistics within 1e-4 x
    max |float64| (a tenth of the GPU test's limits).  A case that fails this is replaced HERE, never by looking at the
    device's result."""
    sd, inp, r64 = R.reference_case(tracking)
    r32 = R.run(sd, tracking, *inp, torch.float32)
    assert list(r64.grads) == [k for k, v in sd.items() if v.is_floating_point() and "running_" not in k]
    for h in r64.z:
        assert float((r32.z[h].double() - r64.z[h]).abs().max()) <= 1e-4 * float(r64.z[h].abs().max()), h
    for k, g in r64.grads.items():
        if g is None:
            assert P.unused(k) and r32.grads[k] is None, k
            continue
        assert not P.unused(k), k
        scale = float(r64.grads[P.companion_weight(k)].abs().max()) if P.is_pre_bn_bias(k) else float(g.abs().max())
        assert scale > 0, k
        err = float((r32.grads[k].double() - g).abs().max())
        assert err <= 1e-4 * scale, (k, err, scale)
    for k, v in r64.buffers.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == (0 if P.unused(k) else 1), k
        elif not P.unused(k):
            assert float((r32.buffers[k].double() - v).abs().max()) <= 1e-4 * float(v.abs().max()), k
    # every gate of the heads' fused ReLU is exercised: some pre-activations are negative
    assert {R.family(k, g.dim()) for k, g in r64.grads.items() if g is not None} >= {"gru", "gn", "heads", "dcn", "conv", "bn", "stem"}
