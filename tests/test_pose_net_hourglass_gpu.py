"""GPU test of ``centerpose_amd.pose_net_hourglass.PoseNetHourglass``: one training step of the stacked hourglass on the library
against the float64 restatement of tests/hourglass_net_ref.py, the full-depth network against the reference's own output, the
hand-off of the trained parameters to the inference engine, and the loss on both stacks.

Set-up (tests/hourglass_net_ref.py): precision f32, the shallow instance ``exkp(2, 2, [256, 256, 384], [1, 1, 1])``, B = 2,
3 x 64 x 96 input, default heads, a seeded random state dict with the shifts ahead of the ReLUs raised, loss = a fixed random
linear functional of the 14 head maps.  Bounds, as tests/test_pose_net_gpu.py: every head map of both stacks, every parameter
gradient and every running statistic within 1e-3 x max |float64 reference|; ``num_batches_tracked`` exactly.  (That test
measures biases whose gradient is mathematically zero against their companion weight; this graph has none: every BatchNorm's
output reaches a padded 3x3 convolution, and tests/test_pose_net_hourglass_cpu.py asserts that every reference gradient is
non-zero.)  The same CPU test checks that the case in float32 on the CPU stays within a tenth of these limits.

Measured on an MI355X (max over the family of error / max |reference|; device, then the float32 CPU reference):
see DESIGN.md section 3.14.
"""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from centerpose_amd import synth
from tests import hourglass_net_ref as R

pytestmark = pytest.mark.gpu

LIMIT = 1e-3
HEADS = synth.HEADS_POSE
GOLD = os.path.join(os.path.dirname(__file__), "golden")


class _Opt:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _step(device):
    """One forward + backward of the shallow PoseNetHourglass on the reference case; returns (net, outputs on the CPU, x)."""
    from centerpose_amd import hip
    from centerpose_amd.pose_net_hourglass import PoseNetHourglass

    hip.set_default_precision("f32")
    sd, (x, lin), _ = R.reference_case()
    net = PoseNetHourglass(HEADS, **R.CASE)
    net.load_state_dict(sd, strict=True)
    net = net.to(device).train()
    x = x.to(device)
    out = net(x)
    assert isinstance(out, list) and len(out) == 2 and all(list(z) == list(HEADS) for z in out)
    loss = sum((z[h] * lin[k][h].to(device)).sum() for k, z in enumerate(out) for h in z)
    loss.backward()
    return net, [OrderedDict((h, v.detach().cpu()) for h, v in z.items()) for z in out], x


def test_training_step_matches_float64(device):
    sd, inp, r64 = R.reference_case()
    r32 = R.run(sd, *inp, torch.float32)   # the float32 CPU reference's own error, printed next to the device's
    net, zs, _ = _step(device)
    fam = {}

    def note(name, err_dev, err_cpu):
        a = fam.setdefault(name, [0.0, 0.0])
        a[0], a[1] = max(a[0], err_dev), max(a[1], err_cpu)

    failures = []
    for k, z64 in enumerate(r64.z):
        for h, ref in z64.items():
            s = float(ref.abs().max())
            e = float((zs[k][h].double() - ref).abs().max()) / s
            note("outputs, stack %d" % k, e, float((r32.z[k][h].double() - ref).abs().max()) / s)
            if e > LIMIT:
                failures.append(("z.%d.%s" % (k, h), e))
    params = dict(net.named_parameters())
    assert list(params) == list(r64.grads)
    for k, g in r64.grads.items():
        p = params[k]
        assert p.grad is not None, k
        s = float(g.abs().max())
        e = float((p.grad.cpu().double() - g).abs().max()) / s
        note(R.family(k, g.dim()), e, float((r32.grads[k].double() - g).abs().max()) / s)
        if e > LIMIT:
            failures.append((k, e))
    bufs = dict(net.named_buffers())
    assert list(bufs) == list(r64.buffers)
    for k, ref in r64.buffers.items():
        got = bufs[k].cpu()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref) == 1, k
            continue
        s = float(ref.abs().max())
        e = float((got.double() - ref).abs().max()) / s
        note("running statistics", e, float((r32.buffers[k].double() - ref).abs().max()) / s)
        if e > LIMIT:
            failures.append((k, e))
    for name, (e_dev, e_cpu) in fam.items():
        print("pose_net_hourglass %-20s device %.2e   float32 CPU %.2e   (of max |float64|)" % (name, e_dev, e_cpu))
    assert not failures, failures[:10]


def test_two_steps_are_bit_identical_and_eval_moves_no_buffer(device):
    """This graph has no atomics: two training steps from the same state give bit-identical outputs and bit-identical gradients
    for EVERY parameter.  eval() runs the same layers on the running statistics (no buffer moves)."""
    a, za, x = _step(device)
    b, zb, _ = _step(device)
    for k in range(2):
        for h in za[k]:
            assert torch.equal(za[k][h], zb[k][h]), (k, h)
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    for (k, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(p, q), k
    before = {k: v.clone() for k, v in a.state_dict().items()}
    a.eval()
    with torch.no_grad():
        out = a(x)
    assert len(out) == 2 and all(torch.equal(v, before[k]) for k, v in a.state_dict().items())


def test_default_network_eval_matches_the_reference_golden(device):
    """The default (full-depth) network in evaluation mode on the golden's 128 x 128 input (1 x 1 at the deepest level): the last
    stack against tests/golden/backbone_hourglass.npz, the reference module's own output, within the tolerance
    test_hourglass_vs_reference_golden (tests/test_gpu_parity.py) uses for f32."""
    from centerpose_amd import hip
    from centerpose_amd.pose_net_hourglass import PoseNetHourglass
    from oracle.tools import make_goldens as mg

    hip.set_default_precision("f32")
    gold = np.load(os.path.join(GOLD, "backbone_hourglass.npz"))
    net = PoseNetHourglass(HEADS)
    net.load_state_dict(synth.make_state_dict("hourglass", HEADS), strict=True)
    net = net.to(device).eval()
    x, _ = mg.backbone_inputs(False)
    with torch.no_grad():
        zs = net(x.to(device))
    assert len(zs) == 2
    z = zs[-1]
    for k in HEADS:
        ref = torch.from_numpy(gold[k])
        err = float((z[k].cpu() - ref).abs().max())
        assert err < 1e-3 * max(1.0, float(ref.abs().max())), (k, err)
    hm = torch.sigmoid(z["hm"].cpu())
    assert float((hm - torch.sigmoid(torch.from_numpy(gold["hm"]))).abs().max()) < 1e-3


def test_default_network_trains_and_hands_off_to_the_engine(device):
    """The default network takes one training step at B = 2, 128 x 256 (1 x 2 at the deepest level): every gradient is present
    and finite.  After one small SGD step and ``model.load_module(net)`` the engine's forward equals ``net.eval()``'s last stack:
    every head within 1e-3 x max |net.eval()|, the heat-maps within 1e-3 on sigmoid(hm)."""
    from centerpose_amd import hip
    from centerpose_amd.lib.models.model import create_model
    from centerpose_amd.pose_net_hourglass import PoseNetHourglass

    hip.set_default_precision("f32")
    model = create_model("hourglass", HEADS, 256, _Opt(precision="f32"))
    model.load_state_dict(synth.make_state_dict("hourglass", HEADS))
    net = PoseNetHourglass.from_model(model).to(device).train()
    x = synth.frames(2, seed=41, h=128, w=256).to(device)
    g = torch.Generator().manual_seed(5)
    out = net(x)
    assert len(out) == 2 and tuple(out[0]["hps"].shape) == (2, 16, 32, 64)
    loss = sum((z[h] * torch.randn(z[h].shape, generator=g).to(device)).sum() for z in out for h in z)
    loss.backward()
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        assert float(p.grad.abs().max()) > 0, k
    with torch.no_grad():
        for p in net.parameters():
            p.add_(p.grad, alpha=-1e-4 / max(1.0, float(p.grad.abs().max())))
    net.eval()
    with torch.no_grad():
        want = net(x)[-1]
    model.load_module(net)
    sd = model.state_dict()
    assert int(sd["pre.0.bn.num_batches_tracked"]) == 1 and int(sd["kps.1.low2.low2.low2.low2.low2.3.bn2.num_batches_tracked"]) == 1
    got = model.to(device)(x)[0]
    for h in HEADS:
        a, b = got[h].cpu().double(), want[h].cpu().double()
        assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max()), h
    for h in ("hm", "hm_hp"):
        assert float((torch.sigmoid(got[h]) - torch.sigmoid(want[h])).abs().max()) < 1e-3, h


def test_object_pose_loss_consumes_both_stacks(device):
    """``ObjectPoseLoss`` with ``num_stacks = 2`` on the shallow network's output list, with the ``stacks2`` batch of
    tests/pose_loss_cases.py (32 x 32 maps: a 128 x 128 input): the loss is finite and the heads of stack 0 receive non-zero
    gradients, as does the backbone below them."""
    from centerpose_amd import hip
    from centerpose_amd.pose_loss import ObjectPoseLoss
    from centerpose_amd.pose_net_hourglass import PoseNetHourglass
    from tests import pose_loss_cases as PC

    hip.set_default_precision("f32")
    opt, phase, _, batch = PC.case("stacks2")
    assert opt.num_stacks == 2 and set(PC.head_names(opt)) == set(HEADS)
    net = PoseNetHourglass(HEADS, opt, **R.CASE)
    net.load_state_dict(R.case_state_dict(), strict=True)
    net = net.to(device).train()
    x = synth.frames(2, seed=43, h=128, w=128).to(device)
    outs = net(x)
    assert len(outs) == opt.num_stacks and tuple(outs[0]["hm"].shape) == (2, 1, 32, 32)
    bt = {k: torch.from_numpy(v).to(device) for k, v in batch.items()}
    loss = ObjectPoseLoss(opt)(outs, bt, phase)[0]
    assert bool(torch.isfinite(loss))
    loss.backward()
    for h in HEADS:
        for k in range(2):
            seq = getattr(net, h)[k]
            for p in (getattr(seq, "0").conv.weight, getattr(seq, "0").conv.bias, getattr(seq, "1").weight, getattr(seq, "1").bias):
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (h, k)
    assert float(net.pre[0].conv.weight.grad.abs().max()) > 0 and float(net.kps[0].low2.low2[0].conv1.weight.grad.abs().max()) > 0
