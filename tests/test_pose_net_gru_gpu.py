"""GPU test of ``centerpose_amd.pose_net_gru.PoseNetGRU``: one training step of the whole dlav1_34 graph on the library against
the float64 restatement of tests/pose_net_gru_ref.py, then the hand-off of the trained parameters to the inference engine.

Set-up: precision f32, B = 2, 3 x 64 x 96 input, head_conv 64 (two channels per group), loss = a fixed random linear functional
of the head outputs; plain (default heads, 3 GRU steps) and tracking (``opt.tracking_task``, the tracking heads, 4 steps,
pre_img + pre_hm + pre_hm_hp).  Bounds, as tests/test_pose_net_gpu.py: head outputs, parameter gradients and running statistics
within 1e-3 x max |float64 reference|; biases whose gradient is mathematically zero within 1e-3 x max |the same module's weight
gradient|; ``num_batches_tracked`` exactly; the unused outer ``project`` of levels 3 and 4 untouched.
tests/test_pose_net_gru_cpu.py checks that the same cases in float32 on the CPU stay within a tenth of these limits.
The per-family figures are in DESIGN.md section 3.12.
"""
from collections import OrderedDict

import pytest
import torch

from centerpose_amd import synth
from tests import pose_net_gru_ref as R
from tests import pose_net_ref as P

pytestmark = pytest.mark.gpu

LIMIT = 1e-3


class _Opt:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _opt(tracking, **kw):
    return _Opt(tracking_task=tracking, pre_img=tracking, pre_hm=tracking, pre_hm_hp=tracking, **kw)


def _step(device, tracking, sd=None, head_conv=R.HEAD_CONV):
    """One forward + backward of PoseNetGRU on the reference case; returns (net, outputs on the CPU, inputs on the device)."""
    from centerpose_amd import hip
    from centerpose_amd.pose_net_gru import PoseNetGRU

    hip.set_default_precision("f32")
    case_sd, (x, pre_img, pre_hm, pre_hm_hp, lin), _ = R.reference_case(tracking)
    heads = R.heads_of(tracking)
    net = PoseNetGRU(heads, head_conv=head_conv, opt=_opt(tracking))
    net.load_state_dict(case_sd if sd is None else sd, strict=True)
    net = net.to(device).train()
    dev = lambda t: None if t is None else t.to(device)
    args = (dev(x), dev(pre_img), dev(pre_hm), dev(pre_hm_hp))
    out = net(*args)
    assert isinstance(out, list) and len(out) == 1 and list(out[0]) == list(heads)
    z = out[0]
    loss = sum((z[h] * lin[h].to(device)).sum() for h in z)
    loss.backward()
    return net, OrderedDict((h, v.detach().cpu()) for h, v in z.items()), args


@pytest.mark.parametrize("tracking", [False, True], ids=["plain", "tracking"])
def test_training_step_matches_float64(device, tracking):
    sd, inp, r64 = R.reference_case(tracking)
    r32 = R.run(sd, tracking, *inp, torch.float32)   # the float32 CPU reference's own error, printed next to the device's
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
            assert P.unused(k) and p.grad is None, k   # the outer project of levels 3 and 4
            continue
        assert p.grad is not None, k
        s = float(r64.grads[P.companion_weight(k)].abs().max()) if P.is_pre_bn_bias(k) else float(g.abs().max())
        e = float((p.grad.cpu().double() - g).abs().max()) / s
        name = "zero-gradient biases" if P.is_pre_bn_bias(k) else R.family(k, g.dim())
        note(name, e, float((r32.grads[k].double() - g).abs().max()) / s)
        if e > LIMIT:
            failures.append((k, e))
    bufs = dict(net.named_buffers())
    assert list(bufs) == list(r64.buffers)
    for k, ref in r64.buffers.items():
        got = bufs[k].cpu()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref) == (0 if P.unused(k) else 1), k
            continue
        if P.unused(k):
            assert torch.equal(got, sd[k]), k   # never run: as loaded
            continue
        s = float(ref.abs().max())
        e = float((got.double() - ref).abs().max()) / s
        note("running statistics", e, float((r32.buffers[k].double() - ref).abs().max()) / s)
        if e > LIMIT:
            failures.append((k, e))
    for name, (e_dev, e_cpu) in fam.items():
        print("pose_net_gru %-9s %-22s device %.2e   float32 CPU %.2e   (of max |float64|)"
              % ("tracking" if tracking else "plain", name, e_dev, e_cpu))
    assert {"gru", "gn", "heads"} <= set(fam)
    assert not failures, failures[:10]


def test_hand_off_to_the_engine(device):
    """head_conv 256, the width the engine's GroupNorm path is tested at.  One SGD step, load_module into a HipPoseNet: the
    engine's forward equals net.eval()'s forward -- the heat-maps within the repository's 1e-3 tolerance on sigmoid(hm), every
    head within 1e-3 x max |net.eval()| -- and from_model brings the state dict back exactly."""
    from centerpose_amd.lib.models.model import create_model
    from centerpose_amd.pose_net_gru import PoseNetGRU

    sd = R.case_state_dict(False, head_conv=256)
    net, _, args = _step(device, False, sd=sd, head_conv=256)
    with torch.no_grad():
        for p in net.parameters():
            if p.grad is not None:
                p.add_(p.grad, alpha=-1e-4)
    net.eval()
    with torch.no_grad():
        want = net(args[0])[0]
    model = create_model("dlav1_34", synth.HEADS_POSE, 256, _Opt(precision="f32"))
    model.load_module(net)
    msd = model.state_dict()
    assert int(msd["base.level0.1.num_batches_tracked"]) == 1 and int(msd["base.level3.project.1.num_batches_tracked"]) == 0
    assert not torch.equal(msd["convGRU.cell0.Whn.weight"], sd["convGRU.cell0.Whn.weight"])   # the step moved it
    got = model.to(device)(args[0])[0]
    for h in synth.HEADS_POSE:
        a, b = got[h].cpu().double(), want[h].cpu().double()
        err = float((a - b).abs().max())
        print("hand-off %s: err %.3g of max %.3g" % (h, err, float(b.abs().max())))
        assert err <= 1e-3 * float(b.abs().max()), h
    for h in ("hm", "hm_hp"):
        assert float((torch.sigmoid(got[h]) - torch.sigmoid(want[h])).abs().max()) < 1e-3, h
    back = PoseNetGRU.from_model(model).state_dict()
    mine = net.state_dict()
    assert list(back) == list(mine)
    for k in mine:
        assert back[k].dtype == mine[k].dtype and torch.equal(back[k], mine[k].cpu()), k


def test_eval_mode_and_repeatability(device):
    """Two training steps from the same state give bit-identical outputs and head gradients (behind the first DCN the parameter gradients inherit
    the float atomics of the DCNv2 input gradient and are compared with the reference only).  eval() moves no buffer."""
    a, za, _ = _step(device, False)
    b, zb, args = _step(device, False)
    for h in za:
        assert torch.equal(za[h], zb[h]), h
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        if k.split(".")[0] in synth.HEADS_POSE:   # conv, GroupNorm, conv: no atomics on the way
            assert torch.equal(p.grad, q.grad), k
    before = {k: v.clone() for k, v in a.state_dict().items()}
    a.eval()
    with torch.no_grad():
        a(args[0])
    assert all(torch.equal(v, before[k]) for k, v in a.state_dict().items())
