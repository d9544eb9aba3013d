"""GPU test of ``centerpose_amd.pose_net.PoseNet``: one training step of the whole dla_34 graph on the library against the
float64 restatement of tests/pose_net_ref.py, then the hand-off of the trained parameters to the inference engine.

Set-up (tests/pose_net_ref.py): precision f32, B = 2, 3 x 64 x 96 input, head_conv 64, default heads, a random state dict with
small non-zero conv_offset_mask weights, loss = a fixed random linear functional of the head outputs.  Bounds: head outputs and
every parameter gradient within 1e-3 x max |float64 reference| (the bound tests/test_conv_backward_gpu.py uses for its
multi-layer block); biases whose gradient is mathematically zero (``pose_net_ref.is_pre_bn_bias``) within 1e-3 x max |the same
module's weight gradient|; running statistics within 1e-3 x max |reference| (they are 0.9 old + 0.1 x a statistic of the
activations, which carry that bound); ``num_batches_tracked`` exactly.  tests/test_pose_net_cpu.py checks that the same case in
float32 on the CPU stays within a tenth of these limits.

Measured on an MI355X (max over the family of error / max |reference|; device, then the float32 CPU reference):
see DESIGN.md section 3.11.
"""
from collections import OrderedDict

import pytest
import torch

from centerpose_amd import synth
from tests import pose_net_ref as R

pytestmark = pytest.mark.gpu

LIMIT = 1e-3


class _Opt:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _step(device, tracking):
    """One forward + backward of PoseNet on the reference case; returns (net, outputs on the CPU, inputs on the device)."""
    from centerpose_amd import hip
    from centerpose_amd.pose_net import PoseNet

    hip.set_default_precision("f32")
    sd, (x, pre_img, pre_hm, lin), _ = R.reference_case(tracking)
    net = PoseNet(synth.HEADS_POSE, head_conv=R.HEAD_CONV, opt=_Opt(pre_img=tracking, pre_hm=tracking, pre_hm_hp=False))
    net.load_state_dict(sd, strict=True)
    net = net.to(device).train()
    dev = lambda t: None if t is None else t.to(device)
    args = (dev(x), dev(pre_img), dev(pre_hm))
    out = net(*args)
    assert isinstance(out, list) and len(out) == 1 and list(out[0]) == list(synth.HEADS_POSE)
    z = out[0]
    loss = sum((z[h] * lin[h].to(device)).sum() for h in z)
    loss.backward()
    return net, OrderedDict((h, v.detach().cpu()) for h, v in z.items()), args


@pytest.mark.parametrize("tracking", [False, True], ids=["plain", "pre_img_pre_hm"])
def test_training_step_matches_float64(device, tracking):
    sd, inp, r64 = R.reference_case(tracking)
    r32 = R.run(sd, *inp, torch.float32)   # the float32 CPU reference's own error, printed next to the device's
    net, z, _ = _step(device, tracking)
    fam = {}

    def note(name, err_dev, err_cpu):
        a = fam.setdefault(name, [0.0, 0.0])
        a[0], a[1] = max(a[0], err_dev), max(a[1], err_cpu)

    failures = []
    for h, ref in r64.z.items():
        s = float(ref.abs().max())
        e = float((z[h].double() - ref).abs().max()) / s
        note("outputs", e, float((r32.z[h].double() - ref).abs().max()) / s)
        if e > LIMIT:
            failures.append((h, e))
    params = dict(net.named_parameters())
    assert list(params) == list(r64.grads)
    for k, g in r64.grads.items():
        p = params[k]
        if g is None:
            assert R.unused(k) and p.grad is None, k   # the outer project of levels 3 and 4
            continue
        assert p.grad is not None, k
        s = float(r64.grads[R.companion_weight(k)].abs().max()) if R.is_pre_bn_bias(k) else float(g.abs().max())
        e = float((p.grad.cpu().double() - g).abs().max()) / s
        name = "zero-gradient biases" if R.is_pre_bn_bias(k) else R.family(k, g.dim())
        note(name, e, float((r32.grads[k].double() - g).abs().max()) / s)
        if e > LIMIT:
            failures.append((k, e))
    bufs = dict(net.named_buffers())
    for k, ref in r64.buffers.items():
        got = bufs[k].cpu()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref) == (0 if R.unused(k) else 1), k
            continue
        if R.unused(k):
            assert torch.equal(got, sd[k]), k   # never run: as loaded
            continue
        s = float(ref.abs().max())
        e = float((got.double() - ref).abs().max()) / s
        note("running statistics", e, float((r32.buffers[k].double() - ref).abs().max()) / s)
        if e > LIMIT:
            failures.append((k, e))
    for name, (e_dev, e_cpu) in fam.items():
        print("pose_net %-14s %-22s device %.2e   float32 CPU %.2e   (of max |float64|)"
              % ("pre_img+pre_hm" if tracking else "plain", name, e_dev, e_cpu))
    assert not failures, failures[:10]


def test_hand_off_to_the_engine(device):
    """One SGD step, load_module into a HipPoseNet: the engine's forward equals net.eval()'s forward -- the heat-maps within the
    repository's 1e-3 tolerance on sigmoid(hm) (as smoke() checks), every head within 1e-3 x max |net.eval()|."""
    from centerpose_amd.lib.models.model import create_model

    net, _, args = _step(device, False)
    with torch.no_grad():
        for p in net.parameters():
            if p.grad is not None:
                p.add_(p.grad, alpha=-1e-4)
    net.eval()
    with torch.no_grad():
        want = net(args[0])[0]
    model = create_model("dla_34", synth.HEADS_POSE, R.HEAD_CONV, _Opt(precision="f32"))
    model.load_module(net)
    sd = model.state_dict()
    assert int(sd["base.level0.1.num_batches_tracked"]) == 1 and int(sd["base.level3.project.1.num_batches_tracked"]) == 0
    got = model.to(device)(args[0])[0]
    for h in synth.HEADS_POSE:
        a, b = got[h].cpu().double(), want[h].cpu().double()
        assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max()), h
    for h in ("hm", "hm_hp"):
        assert float((torch.sigmoid(got[h]) - torch.sigmoid(want[h])).abs().max()) < 1e-3, h


def test_eval_mode_and_repeatability(device):
    """eval() runs the same layers on the running statistics (no buffer moves).  Two training steps from the same state give
    bit-identical outputs and head gradients; behind the first DCN the parameter gradients inherit the float atomics of the
    DCNv2 input gradient (dcn_bwd.hip) and are compared with the reference only."""
    a, za, _ = _step(device, False)
    b, zb, args = _step(device, False)
    for h in za:
        assert torch.equal(za[h], zb[h]), h
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        if k.split(".")[0] in synth.HEADS_POSE:
            assert torch.equal(p.grad, q.grad), k
    before = {k: v.clone() for k, v in a.state_dict().items()}
    a.eval()
    with torch.no_grad():
        a(args[0])
    assert all(torch.equal(v, before[k]) for k, v in a.state_dict().items())
