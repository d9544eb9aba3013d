"""CPU tests (no GPU) of the ConvGRU's training operators: declarations and refusals of cp_gru_gate_forward / _backward, the
module's parameters, and the float32 error of the gate arithmetic that the GPU test's limit is set against."""
import ctypes
import os
import re
from collections import OrderedDict

import pytest
import torch

import __graft_entry__ as ge
from centerpose_amd import conv_gru, hip, synth
from tests import conv_gru_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_gru_gate_forward", "cp_gru_gate_backward")


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def test_symbols_declared_exported_and_listed(built):
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and hasattr(built, name) and name in hip.exported_symbols(), name
    assert "convGRU.py:32-39" in header


def test_refusals_without_a_device(built):
    fwd, bwd = built.cp_gru_gate_forward, built.cp_gru_gate_backward
    p = ctypes.c_void_p(0x1000)

    def f(x3=p, h3=p, hprev=p, hout=p, M=35, Ch=64):
        return fwd(None, x3, h3, hprev, hout, M, Ch)

    def b(x3=p, h3=p, hprev=p, go=p, gx3=p, gh3=p, ghp=p, M=35, Ch=64):
        return bwd(None, x3, h3, hprev, go, gx3, gh3, ghp, M, Ch)

    for kw in (dict(x3=None), dict(hout=None)):
        assert f(**kw) == -1 and b"null argument" in built.cp_last_error(), kw
    for kw in (dict(x3=None), dict(go=None), dict(gx3=None)):
        assert b(**kw) == -1 and b"null argument" in built.cp_last_error(), kw
    for call in (f, b):
        assert call(M=0) == -1 and b"M must be at least 1" in built.cp_last_error()
        assert call(M=-3) == -1 and b"M must be at least 1" in built.cp_last_error()
        for ch in (0, 2, 6, 1028, 2048):
            assert call(Ch=ch) == -1 and b"multiple of 4 in 4..1024" in built.cp_last_error(), ch
        assert call(M=1 << 24, Ch=64) == -1 and b"2^31 elements" in built.cp_last_error()
        assert call(h3=None) == -1 and b"given together" in built.cp_last_error()
        assert call(hprev=None) == -1 and b"given together" in built.cp_last_error()
        assert call(x3=ctypes.c_void_p(0x1004)) == -1 and b"16-byte aligned" in built.cp_last_error()
        assert call(hprev=ctypes.c_void_p(0x1008)) == -1 and b"16-byte aligned" in built.cp_last_error()
    # step 0 has no hidden-side gradients
    assert b(h3=None, hprev=None) == -1 and b"no hidden-side gradients" in built.cp_last_error()
    assert b(h3=None, hprev=None, gh3=None) == -1 and b"no hidden-side gradients" in built.cp_last_error()
    assert b(h3=None, hprev=None, ghp=None) == -1 and b"no hidden-side gradients" in built.cp_last_error()
    assert b(gx3=ctypes.c_void_p(0x100c)) == -1 and b"16-byte aligned" in built.cp_last_error()


def test_no_cpu_path(built):
    inp = R.gate_inputs(0, 5, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.gru_gate_forward(inp.x3, inp.h3, inp.hprev)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.gru_gate_backward(inp.x3, None, None, inp.go)
    with pytest.raises(RuntimeError, match="HIP device"):
        conv_gru.gru_gate(torch.zeros(1, 24, 2, 2))
    with pytest.raises(RuntimeError, match="HIP device"):
        conv_gru.ConvGRU(64, [64], 3, step=3)(torch.zeros(1, 64, 4, 4))


def test_module_carries_the_reference_parameters():
    spec = synth.param_spec("dlav1_34")
    want = OrderedDict((k[len("convGRU."):], tuple(v)) for k, v in spec.items() if k.startswith("convGRU."))
    net = conv_gru.ConvGRU(64, [64], 3, step=4, effective_step=[0, 1, 2, 3])
    assert OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items()) == want
    assert list(dict(net.named_buffers())) == []   # the reference's zero br / bz / bin / bhn are not kept
    assert net.step == 4 and net.effective_step == [0, 1, 2, 3] and net.num_layers == 1
    with pytest.raises(NotImplementedError, match="one layer"):
        conv_gru.ConvGRU(64, [64, 64], 3)


@pytest.mark.parametrize("step0", [False, True])
def test_float32_gate_error_is_far_below_the_gpu_limit(step0):
    inp = R.gate_inputs(1, 63, 64)
    r64, r32 = R.gate_reference(inp, step0), R.gate_reference(inp, step0, torch.float32)
    for k, e in r64.items():
        if e is not None:
            assert float((r32[k].double() - e).abs().max()) <= 0.1 * R.TOL * float(e.abs().max()), k
