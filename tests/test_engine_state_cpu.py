"""The binding's work-space rule (centerpose_amd/hip/model.py: HipModel._fits), checked without a GPU against a stub library
whose size queries change between calls -- as the real ones do when the precision or the kernel-selection switches change
at an unchanged shape.  The rule: every call asks the library, and a kept buffer serves again only while its size is exactly
the answer; the size handed to the library is always the size of the buffer handed with it.  forward / features
(``_ws``), the dense detect (``_det_state``) and the lean detect (``_lean_state``) all follow it.

(The GPU side -- the library refusing a short work space before its first launch, and the walks that change precision and
switches on a living model -- is tests/test_engine_state_gpu.py.)"""
from collections import OrderedDict
from ctypes import c_void_p

import pytest
import torch

from centerpose_amd import synth
from centerpose_amd.hip import _abi
from centerpose_amd.hip.model import HipModel


class StubLib(object):
    """The entry points HipModel's forward / features / detect reach; every launch records the (pointer, bytes) pair it got."""

    def __init__(self):
        self.size = {"ws": 4096, "det": 8192, "lean": 16384}
        self.lean_ok = 0
        self.queries = {"ws": 0, "det": 0, "lean": 0}
        self.launches = []

    def _query(self, which):
        self.queries[which] += 1
        return self.size[which]

    def cp_model_workspace_bytes(self, h, B, H, W):
        return self._query("ws")

    def cp_model_detect_workspace_bytes(self, h, B, H, W, K):
        return self._query("det")

    def cp_model_detect_lean_workspace_bytes(self, h, B, H, W, K):
        return self._query("lean")

    def cp_model_lean_supported(self, h, B, H, W):
        return self.lean_ok

    def cp_last_error(self):
        return b"stub"

    def _launch(self, name, ws, nbytes):
        self.launches.append((name, ws.value, int(nbytes)))
        return 0

    def cp_model_forward(self, *a):
        return self._launch("forward", a[-2], a[-1])

    def cp_model_features(self, *a):
        return self._launch("features", a[-2], a[-1])

    def cp_model_detect(self, *a):
        return self._launch("detect", a[-3], a[-2])

    def cp_model_detect_lean(self, *a):
        return self._launch("detect_lean", a[-3], a[-2])


class _OnDevice(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True: what detect()'s argument check asks of its inputs."""
    is_cuda = property(lambda self: True)


@pytest.fixture
def stub(monkeypatch):
    L = StubLib()
    monkeypatch.setattr(_abi, "lib", lambda: L)
    monkeypatch.setattr(_abi, "_stream", lambda: c_void_p(0))
    monkeypatch.setattr(_abi, "_dev", lambda t: t)
    m = HipModel.__new__(HipModel)   # (no library handle: cp_model_create is not what is under test)
    m._h, m._ws = None, None
    m.arch, m.heads, m.tracking_task = "dla_34", OrderedDict(synth.HEADS_POSE), False
    x = torch.Tensor._make_subclass(_OnDevice, torch.zeros(1, 3, 64, 64))
    return L, m, x


def _walk(L, which, name, run, buffer_of):
    """Sizes 1, 1, 2, 2, 1 times the first: the buffer is replaced exactly at the two changes, and every launch gets the size
    of the buffer it gets"""
    base = L.size[which]
    seen = []
    for i, factor in enumerate((1, 1, 2, 2, 1)):
        L.size[which] = base * factor
        before = L.queries[which]
        run()
        assert L.queries[which] > before, "call %d did not ask the library for the size" % i
        buf = buffer_of()
        kind, ptr, nbytes = L.launches[-1]
        assert kind == name and nbytes == base * factor == buf.numel() and ptr == buf.data_ptr(), (i, L.launches[-1], buf.numel())
        seen.append(buf)
    assert seen[0] is seen[1] and seen[2] is seen[3], "a buffer of the right size was replaced"
    assert seen[1] is not seen[2] and seen[3] is not seen[4], "a buffer of another size was kept"


def test_forward_and_features_buffer_follows_the_query(stub):
    L, m, x = stub
    _walk(L, "ws", "forward", lambda: m.forward(x), lambda: m._ws)
    L.size["ws"] = 4096
    _walk(L, "ws", "features", lambda: m.features(x), lambda: m._ws)
    # the two share the buffer: the same size from either call keeps it
    m.forward(x)
    kept = m._ws
    m.features(x)
    assert m._ws is kept


def test_dense_detect_state_follows_the_query(stub):
    L, m, x = stub
    _walk(L, "det", "detect", lambda: m.detect(x, graph=False, heads="dense"), lambda: m._det_state[3])
    # the outputs belong to the state: a new work space comes with new outputs (and so a new graph key), an unchanged one keeps them
    outs0 = m.detect(x, graph=False, heads="dense")[0]
    assert m.detect(x, graph=False, heads="dense")[0]["hm"] is outs0["hm"]
    L.size["det"] += 256
    assert m.detect(x, graph=False, heads="dense")[0]["hm"] is not outs0["hm"]


def test_lean_detect_state_follows_the_query(stub):
    L, m, x = stub
    L.lean_ok = 1
    _walk(L, "lean", "detect_lean", lambda: m.detect(x, graph=False), lambda: m._lean_state[6])


def test_a_refused_size_query_raises_before_any_launch(stub):
    L, m, x = stub
    for which, run in (("ws", lambda: m.forward(x)), ("det", lambda: m.detect(x, graph=False, heads="dense"))):
        L.size[which] = 0
        with pytest.raises(RuntimeError, match="failed: stub"):
            run()
    assert L.launches == []


def test_fits_is_exact_size_and_same_device():
    buf = torch.empty(512, dtype=torch.uint8)
    assert HipModel._fits(buf, 512, "cpu") and HipModel._fits(buf, 512, torch.device("cpu"))
    assert not HipModel._fits(buf, 511, "cpu") and not HipModel._fits(buf, 768, "cpu")
    assert not HipModel._fits(None, 512, "cpu") and not HipModel._fits(buf, 512, "meta")
