"""The ConvGRU on the device (pytest -m gpu): cp_gru_gate_forward / cp_gru_gate_backward and conv_gru.gru_gate against float64
CPU autograd at 1e-4 x max |reference| per output (float32 on the CPU is at about 1.5e-7), and conv_gru.ConvGRU against the
float64 restatement of convGRU.py with six separate convolutions (tests/conv_gru_ref.py)."""
from collections import OrderedDict

import pytest
import torch

from centerpose_amd import conv_gru, hip, synth
from tests import conv_gru_ref as R
from tests.batchnorm_ref import check

pytestmark = pytest.mark.gpu


def _device_gate(device, inp, step0):
    x3, go = inp.x3.to(device), inp.go.to(device)
    h3, hp = (None, None) if step0 else (inp.h3.to(device), inp.hprev.to(device))
    hout = hip.gru_gate_forward(x3, h3, hp)
    gx3, gh3, ghp = hip.gru_gate_backward(x3, h3, hp, go)
    cpu = lambda t: None if t is None else t.cpu()
    return dict(hout=cpu(hout), grad_x3=cpu(gx3), grad_h3=cpu(gh3), grad_hprev=cpu(ghp))


@pytest.mark.parametrize("step0", [False, True], ids=["with_h3", "step0"])
@pytest.mark.parametrize("M,Ch", R.GATE_CASES)
def test_gate_forward_and_gradients(device, M, Ch, step0):
    inp = R.gate_inputs(M + Ch, M, Ch)
    got = _device_gate(device, inp, step0)
    assert (got["grad_h3"] is None) == step0 == (got["grad_hprev"] is None)
    check(got, R.gate_reference(inp, step0), "gate M=%d Ch=%d step0=%d" % (M, Ch, step0), R.TOL)


def test_gate_two_calls_are_bit_identical_and_null_outputs(device):
    inp = R.gate_inputs(3, 4 * 37 * 45, 64)
    a, b = _device_gate(device, inp, False), _device_gate(device, inp, False)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    x3, h3, hp, go = (t.to(device) for t in inp)
    gx3, gh3, ghp = hip.gru_gate_backward(x3, h3, hp, go, need_h3_grad=False, need_hprev_grad=True)
    assert gh3 is None and torch.equal(gx3.cpu(), a["grad_x3"]) and torch.equal(ghp.cpu(), a["grad_hprev"])
    gx3, gh3, ghp = hip.gru_gate_backward(x3, h3, hp, go, need_h3_grad=True, need_hprev_grad=False)
    assert ghp is None and torch.equal(gh3.cpu(), a["grad_h3"])


def test_gate_function_takes_nchw_and_channels_last(device):
    B, Ch, H, W = 2, 8, 5, 7
    g = torch.Generator().manual_seed(9)
    x3, h3 = torch.randn(B, 3 * Ch, H, W, generator=g), torch.randn(B, 3 * Ch, H, W, generator=g)
    hp, go = torch.randn(B, Ch, H, W, generator=g), torch.randn(B, Ch, H, W, generator=g)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    back = lambda t, c: t.reshape(B, H, W, c).permute(0, 3, 1, 2)
    ref = R.gate_reference(R.GateInputs(rows(x3), rows(h3), rows(hp), rows(go)), False)
    for channels_last in (False, True):
        leaves = [t.to(device) for t in (x3, h3, hp)]
        if channels_last:
            leaves = [t.contiguous(memory_format=torch.channels_last) for t in leaves]
        for t in leaves:
            t.requires_grad_(True)
        out = conv_gru.gru_gate(*leaves)
        assert out.shape == (B, Ch, H, W) and out.is_contiguous(memory_format=torch.channels_last)
        out.backward(go.to(device))
        got = dict(hout=out.detach().cpu(), grad_x3=leaves[0].grad.cpu(), grad_h3=leaves[1].grad.cpu(), grad_hprev=leaves[2].grad.cpu())
        exp = dict(hout=back(ref["hout"], Ch), grad_x3=back(ref["grad_x3"], 3 * Ch), grad_h3=back(ref["grad_h3"], 3 * Ch),
                   grad_hprev=back(ref["grad_hprev"], Ch))
        check(got, exp, "gru_gate cl=%d" % channels_last, R.TOL)


@pytest.mark.parametrize("steps", [3, 4])
def test_conv_gru_against_six_convolutions(device, steps):
    hip.set_default_precision("f32")
    spec = synth.param_spec("dlav1_34")
    want = OrderedDict((k[len("convGRU."):], tuple(v)) for k, v in spec.items() if k.startswith("convGRU."))
    torch.manual_seed(steps)
    net = conv_gru.ConvGRU(64, [64], 3, step=steps, effective_step=list(range(steps)))
    assert OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items()) == want
    sd32 = OrderedDict((k, v.detach().clone()) for k, v in net.state_dict().items())
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 64, 16, 24, generator=g)
    lin = [torch.randn(2, 64, 16, 24, generator=g) for _ in range(steps)]
    net = net.to(device)
    xd = x.to(device).requires_grad_(True)
    outputs, last = net(xd)
    assert len(outputs) == steps and last is outputs[-1]
    sum((o * l.to(device)).sum() for o, l in zip(outputs, lin)).backward()
    sd = OrderedDict((k, v.double().requires_grad_(True)) for k, v in sd32.items())
    x64 = x.double().requires_grad_(True)
    ref = R.conv_gru(sd, x64, steps)
    grads = torch.autograd.grad(sum((o * l.double()).sum() for o, l in zip(ref, lin)), [x64] + list(sd.values()))
    check({"step%d" % i: o.detach().cpu() for i, o in enumerate(outputs)}, {"step%d" % i: o.detach() for i, o in enumerate(ref)},
          "ConvGRU steps=%d" % steps, R.TOL)
    got = dict(x=xd.grad.cpu(), **{k: p.grad.cpu() for k, p in net.named_parameters()})
    check(got, dict(zip(["x"] + list(sd), grads)), "ConvGRU steps=%d grad" % steps, R.TOL_LAYERS)
    # effective_step selects among the states; the last state is returned whatever it holds
    few = conv_gru.ConvGRU(64, [64], 3, step=steps, effective_step=[1]).to(device)
    few.load_state_dict(net.state_dict())
    with torch.no_grad():
        outs, last2 = few(xd)
    assert len(outs) == 1 and torch.equal(outs[0], outputs[1].detach()) and torch.equal(last2, last.detach())
