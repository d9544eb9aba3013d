"""CPU test (no GPU) of the three precision-aware training backwards' entry points: the plain calls and queries --
cp_conv2d_backward_nhwc, cp_pose_heads_backward, cp_dcnv2_backward, cp_dcnv2_backward_det and their *_workspace_bytes -- answer
exactly as the *_prec entries do at CP_PREC_F32 (and the matching `deterministic`): the same return value and the same
cp_last_error() bytes, over every refused geometry of the operators' CPU tests and, on one accepted geometry each, the
null-argument and short-workspace refusals.  Nothing launches: every refusal comes before the first use of a pointer."""
import ctypes

import pytest

import __graft_entry__ as ge
from centerpose_amd import hip
from tests import dcn_det_cases as D
from tests.test_conv_backward_f16x3_cpu import REFUSED as CONV_REFUSED
from tests.test_pose_heads_f16x3_cpu import REFUSED as HEADS_REFUSED

F32 = hip.PRECISIONS["f32"]
P = ctypes.c_void_p(0x1000)     # never dereferenced


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def _same(L, old, new):
    """Both thunks start from the same recorded error, one no backward entry emits, so that an entry which returns without
    recording anything is told from one that records; returns the common (value, cp_last_error())."""
    seen = []
    for f in (old, new):
        assert L.cp_set_default_precision(-1) == hip.CP_ERR_INVALID and L.cp_last_error() == b"precision must be 0 or 1"
        seen.append((f(), L.cp_last_error()))
    assert seen[0] == seen[1], seen
    return seen[0]


# ---- Conv2d ----
CONV_OK = (2, 16, 16, 64, 64, 3, 3, 1, 1)


def _conv(fn, geo, tail, x=P, w=P, y=None, go=P, gx=P, gw=P, gb=P, ws=P, nbytes=1 << 40):
    return fn(None, x, w, y, go, gx, gw, gb, *geo, *tail, ws, nbytes)


def test_conv2d(built):
    L = built
    old_q, new_q, old, new = (L.cp_conv2d_backward_workspace_bytes, L.cp_conv2d_backward_prec_workspace_bytes,
                              L.cp_conv2d_backward_nhwc, L.cp_conv2d_backward_prec_nhwc)
    for geo, text in CONV_REFUSED:
        for need_x in (0, 1):
            v, e = _same(L, lambda: old_q(*geo, need_x), lambda: new_q(*geo, need_x, F32))
            assert v == 0 and text in e, (geo, e)
        v, e = _same(L, lambda: _conv(old, geo, ()), lambda: _conv(new, geo, (F32,)))
        assert v == hip.CP_ERR_INVALID and text in e, (geo, e)
    need = [_same(L, lambda: old_q(*CONV_OK, nx), lambda: new_q(*CONV_OK, nx, F32)) for nx in (0, 1)]
    assert 0 < need[0][0] < need[1][0] and {e for _, e in need} == {b"precision must be 0 or 1"}   # a success records nothing
    n = need[1][0]
    for kw in (dict(x=None), dict(w=None), dict(go=None), dict(gw=None), dict(ws=None)):
        v, e = _same(L, lambda: _conv(old, CONV_OK, (), nbytes=n, **kw), lambda: _conv(new, CONV_OK, (F32,), nbytes=n, **kw))
        assert v == hip.CP_ERR_INVALID and e == b"conv2d_backward: null argument", kw
    for nbytes in (n - 1, need[0][0], 0):
        v, e = _same(L, lambda: _conv(old, CONV_OK, (), nbytes=nbytes), lambda: _conv(new, CONV_OK, (F32,), nbytes=nbytes))
        assert v == hip.CP_ERR_INVALID and e == b"conv2d_backward: workspace too small", nbytes
    # without grad_x the smaller workspace is enough: past every refusal the next thing is a launch, which this test does not do
    for kw in (dict(x=None, gx=None), dict(ws=None, gx=None)):
        v, e = _same(L, lambda: _conv(old, CONV_OK, (), nbytes=need[0][0], **kw), lambda: _conv(new, CONV_OK, (F32,), nbytes=need[0][0], **kw))
        assert v == hip.CP_ERR_INVALID and e == b"conv2d_backward: null argument", kw


# ---- PoseHeads ----
HEADS_OK = (2, 16, 16, 64, 64)


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _tab(*v):
    return (ctypes.c_void_p * len(v))(*v)


NONE = ctypes.cast(None, ctypes.POINTER(ctypes.c_void_p))


def _heads(fn, geo, tail, n, cls, feat=P, w0=None, b0=None, w1=None, b1=None, go=None, gw0=None, gb0=None, gw1=None, gb1=None, gf=P,
           ws=P, nbytes=1 << 40):
    tab = _tab(*[0x1000] * max(n, 1))
    pick = lambda t: tab if t is None else t
    return fn(None, feat, n, pick(w0), pick(b0), pick(w1), pick(b1), cls, pick(go), pick(gw0), pick(gb0), pick(gw1), pick(gb1), gf,
              *geo, *tail, ws, nbytes)


def test_pose_heads(built):
    L = built
    old_q, new_q, old, new = (L.cp_pose_heads_backward_workspace_bytes, L.cp_pose_heads_backward_prec_workspace_bytes,
                              L.cp_pose_heads_backward, L.cp_pose_heads_backward_prec)
    cls = _ints(2, 16)
    # the geometries of tests/test_pose_heads_f16x3_cpu.py, then those of tests/test_pose_heads_cpu.py with their class lists
    refused = [(geo, 2, cls, text) for geo, text in HEADS_REFUSED] + [
        (HEADS_OK, 2, _ints(2, 65), b"classes must be"), (HEADS_OK, 0, cls, b"at least one head"),
        ((1, 8, 8, 48, 64), 1, _ints(2), b"Cin must be"), ((1, 8, 8, 0, 64), 1, _ints(2), b"Cin must be"),
        ((1, 8, 8, 64, 100), 1, _ints(2), b"hidden width must be"), ((1, 8, 8, 64, 64), 1, _ints(0), b"classes must be in 1..64"),
        ((1, 8, 8, 64, 64), 2, _ints(3, 65), b"classes must be in 1..64"), ((1, 8, 8, 64, 64), 0, _ints(1), b"at least one head"),
        ((0, 8, 8, 64, 64), 1, _ints(1), b"at least 1"), ((1, 0, 8, 64, 64), 1, _ints(1), b"at least 1"),
        ((64, 1024, 1024, 64, 64), 1, _ints(1), b"2^31 elements"), ((1, 4096, 4096, 64, 256), 1, _ints(1), b"2^31 elements"),
        (HEADS_OK, 2, None, b"at least one head")]
    for geo, n, c, text in refused:
        v, e = _same(L, lambda: old_q(*geo, n, c), lambda: new_q(*geo, n, c, F32))
        assert v == 0 and text in e, (geo, e)
        v, e = _same(L, lambda: _heads(old, geo, (), n, c), lambda: _heads(new, geo, (F32,), n, c))
        assert v == hip.CP_ERR_INVALID and text in e, (geo, e)
    need, e = _same(L, lambda: old_q(*HEADS_OK, 2, cls), lambda: new_q(*HEADS_OK, 2, cls, F32))
    assert need > 0 and e == b"precision must be 0 or 1"
    hole = _tab(0x1000, None)
    for kw in (dict(feat=None), dict(w0=NONE), dict(b0=NONE), dict(w1=NONE), dict(b1=NONE), dict(go=NONE), dict(gw0=NONE), dict(gb0=NONE),
               dict(gw1=NONE), dict(gb1=NONE), dict(ws=None), dict(w0=hole), dict(b0=hole), dict(w1=hole), dict(b1=hole), dict(gw0=hole),
               dict(gb0=hole), dict(gw1=hole), dict(gb1=hole)):
        v, e = _same(L, lambda: _heads(old, HEADS_OK, (), 2, cls, nbytes=need, **kw),
                     lambda: _heads(new, HEADS_OK, (F32,), 2, cls, nbytes=need, **kw))
        assert v == hip.CP_ERR_INVALID and e == b"pose_heads_backward: null argument", kw
    for nbytes in (need - 1, need - 256, 0):
        v, e = _same(L, lambda: _heads(old, HEADS_OK, (), 2, cls, nbytes=nbytes), lambda: _heads(new, HEADS_OK, (F32,), 2, cls, nbytes=nbytes))
        assert v == hip.CP_ERR_INVALID and e == b"pose_heads_backward: workspace too small", nbytes


# ---- DCNv2: the plain pair is deterministic = 0, the _det pair deterministic = 1 ----
DCN_OK = (1, 16, 8, 8, 16) + D.CP
_DCN_BASE = dict(B=1, C=4, H=8, W=8, Co=4, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, dg=1)
# tests/test_dcn_backward_cpu.py's refused shapes, tests/test_dcn_backward_det_cpu.py's, then the non-fast geometries, which only
# the deterministic form refuses
DCN_REFUSED = [tuple(dict(_DCN_BASE, **kw).values()) for kw in (
    dict(C=6, dg=4), dict(kh=0), dict(H=2, W=2, ph=0, pw=0, kh=5, kw=5), dict(H=3, W=3, dh=3, ph=0, pw=0), dict(B=0), dict(sh=0),
    dict(B=4096, C=512, H=1024, W=1024), dict(C=16, Co=16, B=0), dict(C=16, Co=16, kh=0), dict(C=0, Co=16), dict(C=16, Co=16, H=0))]
DCN_NON_FAST = [(2, C, H, W, Co) + tuple(geo) for C, H, W, Co, geo in D.NON_FAST.values()] + [tuple(_DCN_BASE.values())]


def _dcn(fn, shape, tail, null=None, nbytes=1 << 40):
    ptr = [P] * 11
    if null is not None:
        ptr[null] = None
    return fn(None, *ptr[:10], *shape, *tail, ptr[10], nbytes)


@pytest.mark.parametrize("det", [0, 1])
def test_dcn_v2(built, det):
    L = built
    old_q, old = ((L.cp_dcnv2_backward_det_workspace_bytes, L.cp_dcnv2_backward_det) if det else
                  (L.cp_dcnv2_backward_workspace_bytes, L.cp_dcnv2_backward))
    new_q, new = L.cp_dcnv2_backward_prec_workspace_bytes, L.cp_dcnv2_backward_prec
    name = b"dcn_v2_backward_det" if det else b"dcn_v2_backward"
    for shape in DCN_REFUSED:
        v, e = _same(L, lambda: old_q(*shape), lambda: new_q(*shape, det, F32))
        assert v == 0 and e == b"precision must be 0 or 1", (shape, e)    # the DCN queries refuse a shape without a word
        v, e = _same(L, lambda: _dcn(old, shape, ()), lambda: _dcn(new, shape, (det, F32)))
        assert v == hip.CP_ERR_INVALID and e.startswith(b"dcn_v2_backward: "), (shape, e)
    for shape in DCN_NON_FAST:
        v, e = _same(L, lambda: old_q(*shape), lambda: new_q(*shape, det, F32))
        assert (v == 0) == bool(det) and e == b"precision must be 0 or 1", (shape, e)
        if det:
            v, e = _same(L, lambda: _dcn(old, shape, ()), lambda: _dcn(new, shape, (det, F32)))
            assert v == hip.CP_ERR_INVALID and e.startswith(b"dcn_v2_backward_det: geometry ") and b"outside the deterministic path" in e
        else:   # accepted: the refusals past the geometry
            n = v
            v, e = _same(L, lambda: _dcn(old, shape, (), nbytes=n - 1), lambda: _dcn(new, shape, (det, F32), nbytes=n - 1))
            assert v == hip.CP_ERR_INVALID and e == b"dcn_v2_backward: workspace too small"
    need, e = _same(L, lambda: old_q(*DCN_OK), lambda: new_q(*DCN_OK, det, F32))
    assert need > 0 and e == b"precision must be 0 or 1"
    for null in range(11):
        v, e = _same(L, lambda: _dcn(old, DCN_OK, (), null, need), lambda: _dcn(new, DCN_OK, (det, F32), null, need))
        assert v == hip.CP_ERR_INVALID and e == name + b": null argument", null
    for nbytes in (need - 1, 64, 0):
        v, e = _same(L, lambda: _dcn(old, DCN_OK, (), nbytes=nbytes), lambda: _dcn(new, DCN_OK, (det, F32), nbytes=nbytes))
        assert v == hip.CP_ERR_INVALID and e == name + b": workspace too small", nbytes
