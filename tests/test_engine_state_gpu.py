"""History independence of the engine, and its work-space bound (tests/engine_state_cases.py has the models, the call kinds
and the reference).

A ``cp_model`` and its Python wrapper carry state from call to call: the cached work-space query and lean-support answer, the
launch-form and tap fields, the arena with its peak and the max-pool launch count, the feature map a lean detect keeps, the
captured-graph cache with its 16-entry clear, the profiler's records and event pool, and the binding's three work-space
buffers.  Every test here walks one model through a sequence of calls and holds EACH step, bit for bit, to the same call made as
the first call of a freshly built model; DESIGN.md ("Cross-call state of the engine") lists which test holds which field.

The work-space tests at the end call the C ABI with a ``workspace_bytes`` 256 below the query while the buffer really passed
holds the full size plus a guard band, so that a library that launched anyway would still stay inside the allocation."""
from collections import OrderedDict
from ctypes import c_int, c_void_p

import pytest
import torch

from centerpose_amd import hip
from centerpose_amd.hip import _abi
from tests import engine_state_cases as C

pytestmark = pytest.mark.gpu

S = hip.KernelSel
FORM_TAPS = ["base.base_layer", "base.level2.project", "ida_up.node_1"]  # each selects another form of the launch sequence
# ... and one that leaves it alone: the output of the sub-tree base.level3.tree1 (in dla_34 level3 is two levels deep, so that
# sub-tree is itself a Tree and what it returns is tapped under the name of its root)
SAME_TAP = "base.level3.tree1.root"


def _same(got, want, what):
    bad = C.differing(got, want)
    assert not bad, "%s differs from the fresh model's in: %s" % (what, ", ".join(bad))


def _step(m, key, prec, kind, shape, device, what, seed=29, K=100, sel=0, graph=False):
    """One step of a walk: the call on the walked model ``m`` against the fresh model's -> what detect returned for the heads"""
    x, kw = C.inputs(key, shape, device, seed)
    with hip.select_kernels(sel):
        got, heads = C.call(m, kind, x, kw, K=K, graph=graph)
    _same(got, C.fresh(key, prec, kind, shape, device, seed=seed, K=K, sel=sel), what)
    return heads


# ------------------------------------------------- the control -------------------------------------------------
CONTROL = [("dla_34", p, k, C.A) for p in ("f16x3", "f32") for k in ("forward", "features", "dense", "tap:ida_up.node_1")] + \
          [("dla_34", "f16x3", "forward", C.B), ("dla_34", "f16x3", "forward_sig", C.A),
           ("dlav1_34_track", "f16x3", "forward", C.A), ("dlav1_34_track", "f32", "forward", C.A),
           ("hourglass", "f16x3", "forward", C.A), ("resdcn_18", "f16x3", "forward", C.A),
           ("resdcn_18", "f16x3", "features", C.A), ("dla_34", "f16x3", "lazy", None)]


@pytest.mark.parametrize("key,prec,kind,shape", CONTROL, ids=["%s-%s-%s-%s" % (c[0], c[1], c[2], "x".join(map(str, c[3] or ("lean",))))
                                                               for c in CONTROL])
def test_control_two_fresh_models_agree(device, key, prec, kind, shape):
    """The reference is reproducible: two models built one after the other return the same bits for their first call, for every
    call kind the walks use.  (A failure here is a finding about the kernels' determinism, not a reason for a tolerance.)"""
    if shape is None:
        shape = (C.lean_batch(C.build(key, prec)),) + C.LEAN_HW
    _same(C.fresh(key, prec, kind, shape, device, cached=False), C.fresh(key, prec, kind, shape, device), "a second fresh model")


# ------------------------------------------------- the walks -------------------------------------------------
SHAPE_WALKS = [("dla_34", "f16x3", C.B), ("dla_34", "f32", C.B), ("dlav1_34_track", "f16x3", C.B), ("resdcn_18", "f16x3", C.B),
               ("hourglass", "f16x3", C.A_WIDE)]


@pytest.mark.parametrize("key,prec,other", SHAPE_WALKS, ids=["%s-%s" % w[:2] for w in SHAPE_WALKS])
def test_shape_walk(device, key, prec, other):
    """A, another shape, A: the cached query (ws_cached / ws_key), the binding's buffer and the arena follow the shape."""
    m = C.build(key, prec)
    for i, shape in enumerate((C.A, other, C.A)):
        _step(m, key, prec, "forward", shape, device, "step %d, forward at %s" % (i, shape))


PRECISION_WALKS = [("dla_34", "forward"), ("dla_34", "features"), ("dla_34", "dense"), ("dlav1_34_track", "forward"),
                   ("hourglass", "forward"), ("resdcn_18", "forward"), ("resdcn_18", "features")]


@pytest.mark.parametrize("key,kind", PRECISION_WALKS, ids=["%s-%s" % w for w in PRECISION_WALKS])
def test_precision_walk(device, key, kind):
    """f16x3, f32, f16x3 at one shape.  At A the float32 sequence of dla_34 needs 20,709,376 bytes and the f16x3 one 8,781,824:
    a work-space buffer that survived set_precision would be 11.9 MB short (forward, features), or make the dense detect refuse
    its own buffer.  The library now refuses such a call before its first launch and the binding sizes its buffers by the
    query on every call, so every step runs, and equals the fresh model's."""
    m = C.build(key, "f16x3")
    sizes = []
    for i, prec in enumerate(("f16x3", "f32", "f16x3")):
        m.set_precision(prec)
        sizes.append(m.workspace_bytes(*C.A))
        _step(m, key, prec, kind, C.A, device, "step %d, %s in %s" % (i, kind, prec))
    assert sizes[0] == sizes[2]
    if key == "dla_34":
        assert sizes[1] > sizes[0], "the walk no longer crosses a growing work space: %s" % sizes


@pytest.mark.parametrize("kind", ["forward", "dense"])
def test_switch_walk(device, kind):
    """default, NO_LOWC, default at A through the public select_kernels alone (the two settings need different work spaces:
    the plan pins of dla_34 at 1x128x128)."""
    m = C.build("dla_34", "f16x3")
    for i, sel in enumerate((0, S.NO_LOWC, 0)):
        _step(m, "dla_34", "f16x3", kind, C.A, device, "step %d, %s under switches %#x" % (i, kind, int(sel)), sel=sel)


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
@pytest.mark.parametrize("tap", FORM_TAPS + [SAME_TAP])
def test_tap_then_untapped(device, tap, prec):
    """A tap selects another launch sequence (the fused heads off; for these three also the stem, the entries' projections,
    the IDAUp sums).  None of it may stay: the untapped forward after it, features() and forward() again return the fresh model's
    tensors, stand-alone max-pool launch count and arena peak."""
    m = C.build("dla_34", prec)
    for kind in ("tap:" + tap, "forward", "features", "forward"):
        _step(m, "dla_34", prec, kind, C.A, device, "%s after a tap on %s" % (kind, tap))


@pytest.mark.parametrize("key", ["dla_34", "dlav1_34_track", "hourglass", "resdcn_18"])
def test_profile_on_and_off(device, key):
    """A profiled pass and the pass after profiling was switched off both return the unprofiled bits; the first read drains the
    records, the second finds none."""
    m = C.build(key, "f16x3")
    m.profile(True)
    _step(m, key, "f16x3", "forward", C.A, device, "the profiled forward")
    assert sum(v["launches"] for v in m.profile_read().values()) > 0
    m.profile(False)
    _step(m, key, "f16x3", "forward", C.A, device, "the forward after profile(False)")
    assert m.profile_read() == OrderedDict()
    if key == "dla_34":  # detect under the profiler runs eagerly whatever `graph` says, and leaves no graph behind
        m.profile(True)
        _step(m, key, "f16x3", "dense", C.A, device, "the profiled dense detect", graph=True)
        assert sum(v["launches"] for v in m.profile_read().values()) > 0
        m.profile(False)
        _step(m, key, "f16x3", "dense", C.A, device, "the dense graph detect after profile(False)", graph=True)
        assert m.profile_read() == OrderedDict()


@pytest.fixture(scope="module")
def lean_shape(device):
    m = C.build("dla_34", "f16x3")
    n = C.lean_batch(m)
    assert m.lean_supported(n, *C.LEAN_HW) and (n == 1 or not m.lean_supported(n - 1, *C.LEAN_HW))
    assert not C.build("dla_34", "f32").lean_supported(n, *C.LEAN_HW)
    return (n,) + C.LEAN_HW


def _replay_lean(m, xg, frames_seed, shape, device, K, what):
    """Copy the frames of ``frames_seed`` into the captured input ``xg`` and call the lean graph detect -> its LazyHeads"""
    x2, _ = C.inputs("dla_34", shape, device, frames_seed)
    xg.copy_(x2)
    torch.cuda.synchronize()
    got, heads = C.call(m, "lazy", xg, {}, K=K, graph=True)
    _same(got, C.fresh("dla_34", "f16x3", "lazy", shape, device, seed=frames_seed, K=K), what)
    assert isinstance(heads, hip.LazyHeads) and not heads.materialised()
    return heads


def _lazy_maps_are_forwards(heads, seed, shape, device, what):
    want = C.fresh("dla_34", "f16x3", "forward_sig", shape, device, seed=seed)
    with torch.cuda.stream(C.side(device)):
        got = OrderedDict((k, heads[k]) for k in heads)
        C.side(device).synchronize()
    bad = [k for k in got if not torch.equal(got[k], want[k])]
    assert heads.materialised() and not bad, "%s: the lazy maps differ from forward's in %s" % (what, bad)


def test_detect_kinds_interleaved(device, lean_shape):
    """dense eager, lazy eager, lazy graph (capture, then a replay on new frames copied into the captured input), a forward in
    between, the replay again: one model, three work-space buffers, the kept feature map (kept / graph_kept) and the graph
    cache.  The replayed call's regression maps, materialised afterwards, are forward's."""
    key, prec = "dla_34", "f16x3"
    m = C.build(key, prec)
    _step(m, key, prec, "dense", lean_shape, device, "dense eager")
    heads = _step(m, key, prec, "lazy", lean_shape, device, "lazy eager")
    assert isinstance(heads, hip.LazyHeads)
    xg = C.inputs(key, lean_shape, device, 29)[0].clone()
    got, _ = C.call(m, "lazy", xg, {}, graph=True)
    _same(got, C.fresh(key, prec, "lazy", lean_shape, device), "lazy graph, the capturing call")
    _replay_lean(m, xg, 31, lean_shape, device, 100, "lazy graph, replay on new frames")
    _step(m, key, prec, "forward_sig", lean_shape, device, "forward between two replays", seed=31)
    heads = _replay_lean(m, xg, 31, lean_shape, device, 100, "lazy graph, second replay")
    _lazy_maps_are_forwards(heads, 31, lean_shape, device, "after the second replay")


def test_graph_cache_turnover_dense(device):
    """Dense detect(graph=True) with K = 1..17 on one model: 17 keys, so the 17th capture clears the 16-entry cache; then
    K = 1 again, captured anew and replayed.  Every result equals the eager call's (of a second model that never captures; its
    first call, and K = 1 and 17, are also held to fresh models).
    Not probed: the clear destroying an executable graph that is still in flight -- every comparison here synchronises after
    the call."""
    key, prec = "dla_34", "f16x3"
    m, eager = C.build(key, prec), C.build(key, prec)
    x, kw = C.inputs(key, C.A, device)
    for K in list(range(1, 18)) + [1, 1]:
        got, _ = C.call(m, "dense", x, kw, K=K, graph=True)
        want, _ = C.call(eager, "dense", x, kw, K=K)
        _same(got, want, "dense graph detect, K = %d" % K)
        if K in (1, 17):
            _same(got, C.fresh(key, prec, "dense", C.A, device, K=K), "dense graph detect, K = %d" % K)


def test_graph_cache_turnover_lean(device, lean_shape):
    """The same on the lean path: 17 distinct K cross the clear, which drops graph_kept with the graphs.  A lean graph captured
    after the clear, replayed on new frames, still leaves a LazyHeads that materialises forward's maps.  (In-flight destruction
    is not probed: see test_graph_cache_turnover_dense.)"""
    key, prec = "dla_34", "f16x3"
    m, eager = C.build(key, prec), C.build(key, prec)
    xg = C.inputs(key, lean_shape, device)[0].clone()
    for K in range(1, 18):
        got, heads = C.call(m, "lazy", xg, {}, K=K, graph=True)
        want, _ = C.call(eager, "lazy", xg, {}, K=K)
        assert isinstance(heads, hip.LazyHeads)
        _same(got, want, "lean graph detect, K = %d" % K)
    got, _ = C.call(m, "lazy", xg, {}, K=1, graph=True)          # captured anew
    _same(got, C.fresh(key, prec, "lazy", lean_shape, device, K=1), "lean graph detect after the clear, K = 1")
    heads = _replay_lean(m, xg, 31, lean_shape, device, 1, "lean graph replay after the clear")
    _lazy_maps_are_forwards(heads, 31, lean_shape, device, "after the clear")


def _refuse_bad_h(m, device):
    x = torch.zeros(1, 3, 100, 128, device=device)
    with pytest.raises(RuntimeError, match="multiples of 32"):
        m.forward(x)


def _refuse_default_stream_graph(m, device):
    x, kw = C.inputs("dla_34", C.A, device, 37)
    assert torch.cuda.current_stream().cuda_stream == 0
    with pytest.raises(RuntimeError, match="non-default stream"):
        m.detect(x, graph=True, heads="dense", **kw)


def _refuse_k129(m, device):
    x, kw = C.inputs("dla_34", C.A, device)
    with torch.cuda.stream(C.side(device)):
        with pytest.raises(RuntimeError):
            m.detect(x, K=129, graph=False, heads="dense", **kw)


@pytest.mark.parametrize("refusal", [_refuse_bad_h, _refuse_default_stream_graph, _refuse_k129],
                         ids=["h_not_multiple_of_32", "graph_on_default_stream", "K_129"])
def test_refused_call_leaves_no_trace(device, refusal):
    """A call the library or the binding refuses changes nothing: the valid calls after it return the fresh model's results."""
    key, prec = "dla_34", "f16x3"
    m = C.build(key, prec)
    _step(m, key, prec, "forward", C.A, device, "forward before the refusal")
    refusal(m, device)
    torch.cuda.synchronize()
    _step(m, key, prec, "dense", C.A, device, "dense detect after the refusal")
    _step(m, key, prec, "forward", C.A, device, "forward after the refusal")
    refusal(m, device)
    torch.cuda.synchronize()
    _step(m, key, prec, "features", C.A, device, "features after the second refusal")
    _step(m, key, prec, "dense", C.A, device, "dense graph detect after the second refusal", graph=True)


def test_two_models_alive_at_once(device):
    """dla_34 and the hourglass interleaved: nothing of one model's state is the library's."""
    d, h = C.build("dla_34", "f16x3"), C.build("hourglass", "f16x3")
    for i, (m, key, kind) in enumerate([(d, "dla_34", "forward"), (h, "hourglass", "forward"), (d, "dla_34", "dense"),
                                        (h, "hourglass", "forward"), (d, "dla_34", "tap:ida_up.node_1"),
                                        (h, "hourglass", "dense"), (d, "dla_34", "forward"), (h, "hourglass", "forward")]):
        _step(m, key, "f16x3", kind, C.A, device, "step %d, %s of %s" % (i, kind, key))


# ------------------------------------------------- the work-space bound -------------------------------------------------
GUARD = 1 << 20
CANARY = 0xA5
SENTINEL = -12345.0


def _raw_call(m, entry, x, ws, ws_bytes, tap=None):
    """cp_model_forward / _forward_tap / _features through ctypes with a caller-chosen ``workspace_bytes`` -> (code, outputs
    pre-filled with SENTINEL)"""
    L = _abi.lib()
    n, _, h, w = x.shape
    out = OrderedDict()
    if entry == "cp_model_features":
        out["features"] = torch.full((n, h // 4, w // 4, 64), SENTINEL, device=x.device)
        rc = L.cp_model_features(m._h, _abi._stream(), n, h, w, *_abi._ptrs(x, None, None, None), _abi._ptr(out["features"]),
                                 _abi._ptr(ws), ws_bytes)
        return rc, out
    for k, c in m.heads.items():
        out[k] = torch.full((n, c, h // 4, w // 4), SENTINEL, device=x.device)
    ptrs = (c_void_p * len(m.heads))(*[out[k].data_ptr() for k in m.heads])
    if entry == "cp_model_forward":
        rc = L.cp_model_forward(m._h, _abi._stream(), n, h, w, *_abi._ptrs(x, None, None, None), ptrs, 0, _abi._ptr(ws), ws_bytes)
        return rc, out
    out["tap:" + tap] = torch.full((n * 16 * h * w,), SENTINEL, device=x.device)
    dims = (c_int * 3)(0, 0, 0)
    rc = L.cp_model_forward_tap(m._h, _abi._stream(), n, h, w, *_abi._ptrs(x, None, None, None), ptrs, 0, _abi._ptr(ws), ws_bytes,
                                tap.encode(), _abi._ptr(out["tap:" + tap]), dims)
    if rc == 0:
        out["tap:" + tap] = out["tap:" + tap][: n * dims[0] * dims[1] * dims[2]].view(n, dims[0], dims[1], dims[2])
    return rc, out


BOUND_CASES = [("cp_model_forward", "forward", None), ("cp_model_forward_tap", "tap:ida_up.node_1", "ida_up.node_1"),
               ("cp_model_forward_tap", "tap:" + SAME_TAP, SAME_TAP), ("cp_model_features", "features", None)]


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
@pytest.mark.parametrize("entry,kind,tap", BOUND_CASES, ids=[c[1] for c in BOUND_CASES])
def test_workspace_one_block_short_is_refused_before_any_launch(device, entry, kind, tap, prec):
    """``workspace_bytes`` = the query - 256 (one arena block): CP_ERR_INVALID with both sizes in the message, every output still
    the sentinel, the work space itself and the guard band behind it untouched.  Then the queried size: the call succeeds and
    returns the fresh model's tensors.  The buffer holds the full size plus 1 MiB of guard in both calls, so even a library
    without the check stays inside the allocation."""
    key = "dla_34"
    m = C.build(key, prec)
    x, _ = C.inputs(key, C.A, device)
    need = m.workspace_bytes(*C.A)
    assert need % 256 == 0 and need > 256
    buf = torch.full((need + GUARD,), CANARY, dtype=torch.uint8, device=device)
    with torch.cuda.stream(C.side(device)):
        rc, out = _raw_call(m, entry, x, buf, need - 256, tap)
        msg = _abi.lib().cp_last_error().decode()
        C.side(device).synchronize()
        assert rc == _abi.CP_ERR_INVALID, (rc, msg)
        assert str(need - 256) in msg and str(need) in msg and "too small" in msg, msg
        for k, v in out.items():
            assert bool((v == SENTINEL).all()), "%s was written by a refused call" % k
        assert bool((buf == CANARY).all()), "a refused call wrote its work space"

        rc, out = _raw_call(m, entry, x, buf, need, tap)
        C.side(device).synchronize()
        assert rc == 0, _abi.lib().cp_last_error().decode()
        assert bool((buf[need:] == CANARY).all()), "the pass wrote behind the size it was given"
        assert not bool((buf[:need] == CANARY).all())
    want = C.fresh(key, prec, kind, C.A, device)
    for k, v in out.items():
        assert torch.equal(v.view(want[k].shape) if k != "features" else v.permute(0, 3, 1, 2), want[k]), k
    assert m.workspace_used() <= need
