"""Non-finite values through the training operators on the device (pytest -m gpu): one call, one poisoned input element, against
the float64 torch autograd of the same operation -- the two rules of tests/nonfinite_cases.py (no laundering, no collateral),
whose premises tests/test_nonfinite_cpu.py checks without a GPU.  Every figure is printed before it is asserted; DESIGN.md,
"Non-finite values", holds the tables.

At the parent of the commit that added this file every ReLU of the library was ``fmaxf(v, 0)``, which turns a NaN into 0: the
BatchNorm and GroupNorm ``act=1`` forward cases and the input-poisoned PoseNet step failed rule 1 there (DESIGN.md has the
counts)."""
import collections

import pytest
import torch

from centerpose_amd import hip, synth
from tests import conv_backward_ref as CB
from tests import nonfinite_cases as N
from tests import pose_net_ref as R

pytestmark = pytest.mark.gpu
GROUPS = N.groups()


@pytest.fixture(autouse=True)
def f32_before_and_after():
    """Every test starts in "f32" and leaves the library there, whatever it switched to in between."""
    hip.set_default_precision("f32")
    yield
    hip.set_default_precision("f32")


@pytest.mark.parametrize("group", list(GROUPS))
def test_operator(device, group):
    failures, worst, counted = [], collections.OrderedDict(), 0
    for case in GROUPS[group]():
        for target in case.targets:
            for kind, where in N.POISONS:
                what = "%s | %s %s@%s" % (case.name, target, kind, where)
                inp = case.poisoned(target, kind, where)
                got, gate = case.device(device, inp)
                ref, exempt = case.reference(inp, target, None if gate is None else gate.double())
                collateral = not (case.f16x3 and kind != "nan")   # an Inf operand collapses its f16x3 scale: rule 1 only
                try:
                    stats = N.compare(got, ref, case.tol, what, collateral, exempt)
                except AssertionError as e:
                    failures.append(str(e))
                    continue
                for name, s in stats.items():
                    if collateral:
                        worst[name] = max(worst.get(name, 0.0), s.worst)
                    else:
                        counted += s.missed
    print("%s: worst rule 2 error as a fraction of its bound: %s; finite elements beyond the bound in the f16x3 Inf cases: %d"
          % (group, ", ".join("%s %.3g" % kv for kv in worst.items()), counted))
    assert not failures, "%d failures, the first ten:\n%s" % (len(failures), "\n".join(failures[:10]))


@pytest.mark.parametrize("geo", list(N.POOL_POSITIONS), ids=lambda g: "k%ds%dp%d" % g)
def test_max_pool(device, geo):
    """Exact: selection only.  A NaN wins its window (torch's rule, pool.hip's header) and takes the window's gradient."""
    x, g = N.pool_inputs()
    go = torch.randint(-4, 5, (N.POOL_SHAPE[0], N.POOL_SHAPE[1]) + N.pool_out_size(geo), generator=g).float()

    def run(xp, gp):
        xd, gd = N.nhwc(xp).to(device), N.nhwc(gp).to(device)
        return collections.OrderedDict(y=N.nchw(hip.max_pool2d_forward(xd, *geo)).cpu(), grad_x=N.nchw(hip.max_pool2d_backward(xd, gd, *geo)).cpu())

    failures = []
    for kind, value in N.VALUES.items():
        for (py, px) in N.POOL_POSITIONS[geo]:
            xp = x.clone()
            xp[0, 1, py, px] = value
            try:
                N.compare(run(xp, go), N.pool_reference(xp, go, geo), 0.0, "max_pool %s x[0,1,%d,%d]=%s" % (geo, py, px, kind))
            except AssertionError as e:
                failures.append(str(e))
        gp = go.clone()
        gp.view(-1)[3] = value
        try:
            N.compare(run(x, gp), N.pool_reference(x, gp, geo), 0.0, "max_pool %s grad_out %s" % (geo, kind))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures[:10])


def test_f16x3_backward_in_the_largest_binade(device):
    """grad_out in [2^127, 2^128), x and w of order 2^-100: the |max| exponent of grad_out is above cp_amax_to_scale's clamp, so
    its scaled values reach [2^15, 2^16) and the round-toward-zero split saturates the hi half at 65504 above that.  The f16x3
    gradients against the exact-f32 mode's (float64 has no such range problem and is no yardstick for it), at the f16x3
    Gaussian bound of tests/test_conv_backward_f16x3_gpu.py."""
    c = CB.CASES[1]
    assert CB.is_mfma(c)
    i = CB.gaussian_inputs(70, c)
    g = torch.Generator().manual_seed(71)
    mag = (1 + torch.rand(i.go.shape, generator=g)).clamp(max=2 - 2.0 ** -23) * 2.0 ** 127
    go = torch.where(i.go < 0, -mag, mag)
    assert bool(torch.isfinite(go).all()) and float(go.abs().min()) >= 2.0 ** 127
    x, w = (N.nhwc(i.x) * 2.0 ** -100).to(device), (i.w * 2.0 ** -100).to(device)
    assert hip.ops.conv2d_backward_precision_mask(c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.stride, c.pad) == 3
    res = {}
    for prec in ("f32", "f16x3"):
        gx, gw, _ = hip.ops.conv2d_backward_prec(x, w, N.nhwc(go).to(device), stride=c.stride, pad=c.pad, need_bias_grad=False, precision=prec)
        res[prec] = collections.OrderedDict(grad_x=gx.cpu(), grad_w=gw.cpu())
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in res["f32"].values())
    N.compare(res["f16x3"], collections.OrderedDict((k, v.double()) for k, v in res["f32"].items()), N.GRAD_TOL, "largest binade")


def _dcn_offset_case(C, value):
    """inputs of the DCN cases with C input channels and one offset (image 1, tap 4's row offset, pixel (4, 5)) poisoned -> (the
    poisoned inputs, the same inputs with that tap's sample switched off instead: offset 0, mask 0)"""
    from tests import dcn_backward_f16x3_cases as DF

    B, _, H, W, Co = N.DCN_SHAPES[1]
    x, w, b, off, mask, _ = DF.gaussian_case((B, C, H, W, Co), 0.5)
    bad, mute_off, mute_mask = off.clone(), off.clone(), mask.clone()
    bad[1, 8, 4, 5] = value
    mute_off[1, 8, 4, 5] = 0.0
    mute_mask[1, 4, 4, 5] = 0.0
    return (x, w, b, bad, mask), (x, w, b, mute_off, mute_mask)


@pytest.mark.parametrize("kernel", ["f32", "f16x3", "generic"])
def test_dcn_forward_offset_rule(device, kernel):
    """What each DCNv2 forward makes of a non-finite sampling coordinate.  +-Inf is outside the image in all of
    them: the sample is a zero, as in the reference CUDA code.  A NaN coordinate: the float32 fast path (igemm.hip) takes it for
    inside, as the backward's make_sample does, and the pixel's outputs are NaN like the float64 restatement's; the f16x3
    samplers (dcn_patch_common.h) and the generic kernel (dcn_generic.hip, here reached with C = 8) keep the reference CUDA
    code's comparisons, under which it is outside -- the sample is a zero and the output finite.  In every one of them no address
    is formed from such a coordinate."""
    from tests import dcn_backward_f16x3_cases as DF

    hip.set_default_precision("f16x3" if kernel == "f16x3" else "f32")
    C = 8 if kernel == "generic" else N.DCN_SHAPES[1][1]
    run = lambda a: collections.OrderedDict(out=hip.dcn_v2_forward(*(t.to(device) for t in a), *DF.CP).cpu())
    ref = lambda a: collections.OrderedDict(out=R.dcn_v2(*(t.double() for t in a)))
    for name, value in N.VALUES.items():
        bad, mute = _dcn_offset_case(C, value)
        propagates = name == "nan" and kernel == "f32"
        want = ref(bad if propagates else mute)
        assert int(N.nonfinite(want["out"]).sum()) == (N.DCN_SHAPES[1][4] if propagates else 0)
        N.compare(run(bad), want, N.DCN_FWD_TOL, "dcn_v2_forward %s, offset %s" % (kernel, name))


# ---- the whole network: PoseNet on the case of tests/pose_net_ref.py (B = 2, 3 x 64 x 96) ----
class _Opt:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _step(device, sd, x, lin):
    from centerpose_amd.pose_net import PoseNet

    net = PoseNet(synth.HEADS_POSE, head_conv=R.HEAD_CONV, opt=_Opt(pre_img=False, pre_hm=False, pre_hm_hp=False))
    net.load_state_dict(sd, strict=True)
    net = net.to(device).train()
    z = net(x.to(device))[0]
    sum((z[h] * lin[h].to(device)).sum() for h in z).backward()
    return net, collections.OrderedDict((h, v.detach().cpu()) for h, v in z.items())


def _laundered_grads(net, ref):
    """names of the parameter gradients that are finite somewhere the reference's is not"""
    params, bad = dict(net.named_parameters()), []
    for k, g in ref.grads.items():
        if g is None:
            assert params[k].grad is None, k
            continue
        n = int((N.nonfinite(g) & ~N.nonfinite(params[k].grad.cpu())).sum())
        if n:
            bad.append((k, n, int(N.nonfinite(g).sum())))
    return bad


def test_pose_net_poisoned_input_reaches_every_output_and_the_optimizer_skips(device):
    from centerpose_amd.optim import Adam

    sd, (x, _, _, lin), _ = R.reference_case(False)
    x = x.clone()
    x[1, 2, 30, 41] = float("nan")
    ref = R.run(sd, x, None, None, lin, torch.float64)
    assert all(bool(N.nonfinite(v).all()) for v in ref.z.values())   # one pixel poisons every channel of the first BatchNorm
    net, z = _step(device, sd, x, lin)
    failures = []
    for h, v in ref.z.items():
        n = int((N.nonfinite(v) & ~N.nonfinite(z[h])).sum())
        print("pose_net poisoned input: head %s non-finite ref %d, got %d, laundered %d" % (h, int(N.nonfinite(v).sum()), int(N.nonfinite(z[h]).sum()), n))
        if n:
            failures.append(("output " + h, n))
    bad = _laundered_grads(net, ref)
    print("pose_net poisoned input: %d of %d parameter gradients laundered" % (len(bad), sum(g is not None for g in ref.grads.values())))
    failures += bad[:10]
    k = "base.base_layer.1.running_mean"
    want, got = torch.isnan(ref.buffers[k]), torch.isnan(dict(net.named_buffers())[k].cpu())
    print("pose_net poisoned input: %s NaN in %d channels of the reference, %d of the device" % (k, int(want.sum()), int(got.sum())))
    assert bool(want.any())
    if bool((want & ~got).any()):
        failures.append((k, int((want & ~got).sum())))
    assert not failures, failures
    # the step torch would take on these gradients writes NaN into every parameter; with skip_nonfinite it is not taken
    before = collections.OrderedDict((n, p.detach().clone()) for n, p in net.named_parameters())
    opt = Adam(net.parameters(), lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    opt.step()
    assert bool(opt.last_step_skipped) and not bool(torch.isfinite(opt.last_grad_norm))
    for n, p in net.named_parameters():
        assert torch.equal(p.detach().view(torch.int32), before[n].view(torch.int32)), n


def test_pose_net_poisoned_head_bias_stays_in_its_head(device):
    """One bias of the ``hps`` head's hidden layer is NaN: that head's maps are non-finite, the other heads' maps are finite and
    within tests/test_pose_net_gpu.py's bound.  The hidden unit is NaN, so its ReLU gate passes the gradient (torch's
    threshold_backward): of the heads' parameter gradients only ``hps.2.weight``, which multiplies by the hidden layer, is
    non-finite, and the finite ones -- the poisoned head's own 3x3 weight and bias among them -- are within the same bound."""
    sd, (x, _, _, lin), _ = R.reference_case(False)
    sd = collections.OrderedDict((k, v.clone()) for k, v in sd.items())
    sd["hps.0.bias"][5] = float("nan")
    ref = R.run(sd, x, None, None, lin, torch.float64)
    for h, v in ref.z.items():
        assert bool(N.nonfinite(v).all() if h == "hps" else torch.isfinite(v).all()), h
    net, z = _step(device, sd, x, lin)
    N.compare(z, ref.z, 1e-3, "pose_net poisoned hps.0.bias, outputs")
    bad = _laundered_grads(net, ref)
    assert not bad, bad[:10]
    params = dict(net.named_parameters())
    heads = [k for k in ref.grads if k.split(".")[0] in synth.HEADS_POSE]
    assert len(heads) == 4 * len(synth.HEADS_POSE)
    assert [k for k in heads if not bool(torch.isfinite(ref.grads[k]).all())] == ["hps.2.weight"]
    N.compare({k: params[k].grad for k in heads}, {k: ref.grads[k] for k in heads}, 1e-3, "pose_net poisoned hps.0.bias, gradients")
