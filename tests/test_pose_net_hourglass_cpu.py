"""CPU tests (no GPU) of ``centerpose_amd.pose_net_hourglass.PoseNetHourglass``: its state dict against the reference's, its
round trip through HipPoseNet, and the reference the GPU test rests on (tests/hourglass_net_ref.py): pinned in float64 to one
training step of the reference's own module (tests/golden/hourglass_train_ref.npz), pinned in evaluation mode at full depth to
the reference's output (tests/golden/backbone_hourglass.npz), and well conditioned in float32 for the very case the GPU test
runs."""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import __graft_entry__ as ge
from centerpose_amd import conv, hip, norm, pose_heads, stem, synth, upsample
from centerpose_amd.lib.models.model import create_model
from centerpose_amd.pose_net import PoseNet
from centerpose_amd.pose_net_hourglass import PoseNetHourglass
from tests import hourglass_net_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
HEADS = synth.HEADS_POSE


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "hourglass_train_ref.npz"))


def test_state_dict_is_the_reference():
    net = PoseNetHourglass(HEADS)
    sd = net.state_dict()
    spec = synth.param_spec("hourglass", HEADS)
    assert list(sd) == list(spec)
    assert all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
    keys = json.load(open(os.path.join(GOLD, "state_dict_keys.json")))["hourglass"]
    assert {k: list(v.shape) for k, v in sd.items()} == {k: list(v) for k, v in keys.items()}
    # strict load of a reference-format checkpoint
    net.load_state_dict(synth.make_state_dict("hourglass", HEADS), strict=True)
    # the reference's deterministic initial values (large_hourglass.py:255-256), on every stack
    fresh = PoseNetHourglass(HEADS)
    for h in HEADS:
        for k in range(2):
            b = getattr(getattr(fresh, h)[k], "1").bias
            assert bool((b == -2.19).all()) == ("hm" in h), (h, k)
            assert bool((getattr(getattr(fresh, h)[k], "0").conv.bias.abs() < 1).all())
    # the layers are the library's (the empty Sequentials -- max1, an identity skip -- hold nothing)
    leaves = [m for m in net.modules() if not list(m.children()) and not isinstance(m, nn.Sequential)]
    assert {type(m).__module__.split(".")[-1] for m in leaves} == {"conv", "stem", "norm", "upsample", "pose_heads"}
    assert {type(m) for m in leaves} == {conv.Conv2d, stem.StemConv2d, norm.BatchNorm2d, upsample.UpsampleAdd, pose_heads._Slot}
    assert type(net.pre[0].conv) is stem.StemConv2d and net.pre[0].conv.out_channels == 128 and net.pre[0].conv.stride == (2, 2)
    assert sum(type(m) is upsample.UpsampleAdd for m in net.modules()) == 10 and len(net.kps[0].max1) == 0
    # the fusions: a ReLU after every BatchNorm but the skips' and inters_'
    for name, m in net.named_modules():
        if type(m) is norm.BatchNorm2d:
            assert m.relu == (not (name.endswith(".skip.1") or name.startswith("inters_."))), name
            assert m.momentum == 0.1 and m.eps == 1e-5
        if type(m) is conv.Conv2d:
            assert m.relu is False and m.bias is None, name


def test_shallow_instance_is_the_reference(golden):
    net = PoseNetHourglass(HEADS, **R.CASE)
    sd = net.state_dict()
    assert list(sd) == list(golden["keys"]) == list(R.case_spec())
    assert [";".join(str(d) for d in v.shape) for v in sd.values()] == list(golden["shapes"])
    net.load_state_dict(R.case_state_dict(), strict=True)
    assert [k for k, _ in net.named_parameters()] == list(golden["g.names"])
    with pytest.raises(ValueError, match="n \\+ 1"):
        PoseNetHourglass(HEADS, n=3, dims=[256, 256], modules=[1, 1])
    with pytest.raises(NotImplementedError, match="dims\\[0\\]"):
        PoseNetHourglass(HEADS, n=1, dims=[128, 256], modules=[1, 1])


def test_sizes_are_checked_before_any_launch():
    net = PoseNetHourglass(HEADS, **R.CASE)
    for shape in ((1, 3, 64, 72), (1, 3, 40, 64), (1, 3, 8, 8)):
        with pytest.raises(RuntimeError, match="multiples of 16"):
            net(torch.zeros(shape))
    with pytest.raises(RuntimeError, match=r"\[B,3,H,W\]"):
        net(torch.zeros(1, 4, 64, 64))
    with pytest.raises(RuntimeError, match="HIP device"):   # a good size reaches the first layer, which has no CPU path
        net(torch.zeros(1, 3, 64, 64))


def test_round_trip_through_hip_pose_net(built):
    ref = synth.make_state_dict("hourglass", HEADS)
    ref["kps.1.low2.up1.0.bn1.num_batches_tracked"] = torch.tensor(5)
    model = create_model("hourglass", HEADS, 256)
    model.load_state_dict(ref)
    net = PoseNetHourglass.from_model(model)
    assert isinstance(net, PoseNetHourglass) and net.training and net.nstack == 2 and net.n == 5
    other = create_model("hourglass", HEADS, 256)
    other.load_module(net)
    back = other.state_dict()
    assert list(back) == list(ref)
    for k in ref:
        assert back[k].dtype == ref[k].dtype and torch.equal(back[k], ref[k]), k
    # copies, not views: training the module does not reach into the model until load_module
    with torch.no_grad():
        net.cnvs[1].conv.weight.add_(1.0)
    assert torch.equal(model.state_dict()["cnvs.1.conv.weight"], ref["cnvs.1.conv.weight"])
    with pytest.raises(RuntimeError, match="does not match"):
        create_model("dla_34", HEADS, 256).load_module(net)
    with pytest.raises(NotImplementedError, match="not hourglass"):
        PoseNetHourglass.from_model(create_model("dla_34", HEADS, 256))


def test_the_two_refusals_still_raise_and_say_where_to_go():
    with pytest.raises(NotImplementedError, match="hourglass"):
        PoseNet(HEADS, arch="hourglass")
    with pytest.raises(NotImplementedError, match="PoseNetHourglass.from_model"):
        PoseNet(HEADS, arch="hourglass")
    with pytest.raises(NotImplementedError, match="PoseNetHourglass.from_model"):
        create_model("hourglass", HEADS, 256).train_module()


def test_reference_equals_the_reference_module_in_float64(golden):
    """tests/hourglass_net_ref.py in float64 against one training step of the reference's own ``exkp`` in float64
    (tools/make_hourglass_train_golden.py): 1e-9 relative, two float64 evaluations of one graph."""
    _, _, r = R.reference_case()
    rel = lambda a, b: float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-300)
    for k, z in enumerate(r.z):
        assert list(z) == list(HEADS)
        for h in z:
            assert rel(z[h].numpy(), golden["z.%d.%s" % (k, h)]) <= 1e-9, (k, h)
    assert list(r.grads) == list(golden["g.names"])
    for i, (k, g) in enumerate(r.grads.items()):
        scale = float(golden["g.abs"][i])
        assert scale > 0, k
        assert abs(float(g.sum()) - float(golden["g.sum"][i])) <= 1e-9 * scale, k
        assert abs(float(g.abs().sum()) - scale) <= 1e-9 * scale, k
        assert rel(R.grad_sample(g).numpy(), golden["g.sample.%d" % i]) <= 1e-9, k
    for bn in R.GOLDEN_BNS:
        for leaf in ("running_mean", "running_var"):
            assert rel(r.buffers["%s.%s" % (bn, leaf)].numpy(), golden["b.%s.%s" % (bn, leaf)]) <= 1e-9, (bn, leaf)
        assert int(r.buffers[bn + ".num_batches_tracked"]) == int(golden["b.%s.num_batches_tracked" % bn]) == 1
    assert all(int(v) == 1 for k, v in r.buffers.items() if k.endswith("num_batches_tracked"))


def test_reference_eval_mode_equals_the_reference_output():
    """tests/hourglass_net_ref.py at full depth in evaluation mode on tests/golden/backbone_hourglass.npz (the reference
    module's own float32 output on synth's weights at 128 x 128): the last stack within that file's tolerance in
    tests/test_oracle_pins.py, 1e-5 absolute.  The restatement runs in float32, as the fixture's producer and that test's
    oracle do: the tolerance is one between two float32 evaluations (the fixture itself is 1.4e-5 from the float64 values)."""
    from oracle.tools import make_goldens as mg

    gold = np.load(os.path.join(GOLD, "backbone_hourglass.npz"))
    sd = synth.make_state_dict("hourglass", HEADS)
    x, _ = mg.backbone_inputs(False)
    sd = {k: v.clone() for k, v in sd.items()}
    with torch.no_grad():
        zs = R.forward(sd, x, HEADS, False)
    assert len(zs) == 2 and list(zs[1]) == list(HEADS)
    for h in HEADS:
        np.testing.assert_allclose(zs[1][h].numpy(), gold[h], rtol=0, atol=1e-5, err_msg=h)
    assert all(int(v) == 0 for k, v in sd.items() if k.endswith("num_batches_tracked"))  # evaluation touches no buffer


def test_reference_case_is_well_conditioned():
    """The GPU test's case evaluated in float32 on the CPU: every head map of both stacks, every parameter gradient and every
    running statistic within 1e-4 x max |float64| (a tenth of the GPU test's limit).  A case that fails this is replaced HERE
    (seed, size), never by looking at the device's result."""
    sd, inp, r64 = R.reference_case()
    r32 = R.run(sd, *inp, torch.float32)
    assert list(r64.grads) == [k for k, v in sd.items() if v.is_floating_point() and "running_" not in k]
    for k, z in enumerate(r64.z):
        for h in z:
            assert float((r32.z[k][h].double() - z[h]).abs().max()) <= 1e-4 * float(z[h].abs().max()), (k, h)
    for k, g in r64.grads.items():
        scale = float(g.abs().max())
        assert scale > 0, k   # this graph has no parameter whose gradient is mathematically zero
        assert float((r32.grads[k].double() - g).abs().max()) <= 1e-4 * scale, k
    for k, v in r64.buffers.items():
        if v.is_floating_point():
            assert float((r32.buffers[k].double() - v).abs().max()) <= 1e-4 * float(v.abs().max()), k
