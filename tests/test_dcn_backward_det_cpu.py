"""The deterministic DCNv2 backward, CPU side (no device): the ABI surface and refusals of cp_dcnv2_backward_det, the plan
mirror of tests/dcn_det_cases.py against the library, the resolution of the `deterministic` switch, and the shared device /
host header centerpose_amd/csrc/dcn_bwd_det_common.h built for the host (tests/native/dcn_det_host.cpp): id round trip, keys
of non-finite and edge positions, and the index build + stable sort on the "one cell" case."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from centerpose_amd import hip
from tests import dcn_det_cases as D

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CP = D.CP
u32p = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


@pytest.fixture(scope="module")
def host():
    out = os.path.join(REPO, "tests", "_build", "libcp_dcn_det_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(REPO, "tests", "native", "dcn_det_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
    lib = ctypes.CDLL(out)
    lib.dcn_det_host_roundtrip.restype = ctypes.c_uint32
    lib.dcn_det_host_roundtrip.argtypes = [ctypes.c_uint32]
    lib.dcn_det_host_keys.restype = None
    lib.dcn_det_host_keys.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.dcn_det_host_passes.restype = ctypes.c_int
    lib.dcn_det_host_passes.argtypes = [ctypes.c_uint32]
    lib.dcn_det_host_index.restype = ctypes.c_int
    lib.dcn_det_host_index.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


# ---- ABI and refusals ----
def test_header_declares_and_library_exports_the_deterministic_call(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "centerpose_hip.h")).read(), flags=re.S)
    for name in ("cp_dcnv2_backward_det_workspace_bytes", "cp_dcnv2_backward_det"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(built, name) and name in hip.exported_symbols()
    q, c = built.cp_dcnv2_backward_det_workspace_bytes, built.cp_dcnv2_backward_det
    assert q.restype is ctypes.c_size_t and q.argtypes == [ctypes.c_int] * 14
    assert c.restype is ctypes.c_int
    assert c.argtypes == [ctypes.c_void_p] * 11 + [ctypes.c_int] * 14 + [ctypes.c_void_p, ctypes.c_size_t]
    # the same argument lists as the default call's declarations, and no ABI bump for an addition
    decl = {n: re.search(r"\b%s\s*\((.*?)\);" % n, text, flags=re.S).group(1).split() for n in
            ("cp_dcnv2_backward", "cp_dcnv2_backward_det", "cp_dcnv2_backward_workspace_bytes",
             "cp_dcnv2_backward_det_workspace_bytes")}
    assert decl["cp_dcnv2_backward"] == decl["cp_dcnv2_backward_det"]
    assert decl["cp_dcnv2_backward_workspace_bytes"] == decl["cp_dcnv2_backward_det_workspace_bytes"]
    assert built.cp_abi_version() == 7


def _query(L, B, C, H, W, Co, geo):
    return L.cp_dcnv2_backward_det_workspace_bytes(B, C, H, W, Co, *geo)


@pytest.mark.parametrize("kind", sorted(D.NON_FAST))
def test_query_is_zero_for_a_non_fast_geometry(built, kind):
    C, H, W, Co, geo = D.NON_FAST[kind]
    assert _query(built, 2, C, H, W, Co, geo) == 0
    assert built.cp_dcnv2_backward_workspace_bytes(2, C, H, W, Co, *geo) > 0   # a geometry the default call accepts


@pytest.mark.parametrize("bad", [dict(B=0), dict(kh=0), dict(C=0), dict(H=0)])
def test_query_is_zero_for_a_bad_shape(built, bad):
    a = dict(B=1, C=16, H=8, W=8, Co=16, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, dg=1)
    a.update(bad)
    assert built.cp_dcnv2_backward_det_workspace_bytes(*a.values()) == 0


ALL_SHAPES = D.PARITY_SHAPES + [D.SMALL, D.REPRO, D.ONE_CELL, D.CHUNKED, (16, 64, 128, 128, 64), (16, 512, 16, 16, 256),
                                (5, 16, 384, 384, 16), (64, 256, 32, 32, 128)]


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_query_equals_the_plan_mirror_and_exceeds_the_default(built, shape):
    n = _query(built, *shape, CP)
    d = built.cp_dcnv2_backward_workspace_bytes(*shape, *CP)
    assert d == D.default_workspace_bytes(*shape)
    assert n == D.det_workspace_bytes(*shape)
    assert n > d
    B, C, H, W, _ = shape
    assert n - d >= 16 * D.plan(*shape).nb * H * W * 36   # keys and ids, double-buffered


def test_the_chunked_case_is_one_image_per_chunk():
    assert D.plan(*D.CHUNKED).nb == 1
    B, C, H, W, Co = D.CHUNKED
    assert D.plan(1, C, H, W, Co).nb == 1 and 2 * 9 * C * H * W * 4 > (256 << 20) >= 9 * C * H * W * 4
    assert D.plan(16, 64, 128, 128, 64).nb == 7    # DLA's widest DCN at the benchmark's batch: three chunks


def _call(L, B=1, C=16, H=8, W=8, Co=16, geo=CP, ws_bytes=1 << 30, null=None):
    fake = [ctypes.c_void_p(256)] * 11  # never dereferenced: every refusal comes before any launch
    if null is not None:
        fake[null] = ctypes.c_void_p(0)
    return L.cp_dcnv2_backward_det(ctypes.c_void_p(0), *fake[:10], B, C, H, W, Co, *geo, fake[10], ws_bytes)


@pytest.mark.parametrize("null", [0, 5, 7, 10])
def test_null_pointer_is_refused(built, null):
    assert _call(built, null=null) == hip.CP_ERR_INVALID
    assert "dcn_v2_backward_det: null argument" in built.cp_last_error().decode()


def test_short_workspace_is_refused(built):
    need = _query(built, 1, 16, 8, 8, 16, CP)
    assert _call(built, ws_bytes=need - 1) == hip.CP_ERR_INVALID
    assert "dcn_v2_backward_det: workspace too small" in built.cp_last_error().decode()
    # the default call's size is too small as well
    assert _call(built, ws_bytes=built.cp_dcnv2_backward_workspace_bytes(1, 16, 8, 8, 16, *CP)) == hip.CP_ERR_INVALID


def test_bad_shape_is_refused_as_the_default_call_refuses_it(built):
    assert _call(built, B=0) == hip.CP_ERR_INVALID
    assert "bad shape" in built.cp_last_error().decode()


@pytest.mark.parametrize("kind", sorted(D.NON_FAST))
def test_non_fast_geometry_is_refused_and_named(built, kind):
    C, H, W, Co, geo = D.NON_FAST[kind]
    assert _call(built, 2, C, H, W, Co, geo) == hip.CP_ERR_INVALID
    msg = built.cp_last_error().decode()
    kh, kw, sh, sw, ph, pw, dh, dw, dg = geo
    for part in ("%dx%d" % (kh, kw), "stride %d,%d" % (sh, sw), "pad %d,%d" % (ph, pw), "dilation %d,%d" % (dh, dw),
                 "deformable_group %d" % dg, "C = %d" % C,
                 "3x3 / stride 1 / pad 1 / dilation 1 / one group / C % 16 == 0"):
        assert part in msg, (part, msg)


# ---- the switch ----
@pytest.fixture
def flags():
    own = hip.deterministic()
    t, w = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    yield
    hip.set_deterministic(own)
    torch.use_deterministic_algorithms(t, warn_only=w)


def _resolve(requested, fast):
    return hip.resolve_deterministic(requested, fast, hip.deterministic(), torch.are_deterministic_algorithms_enabled(),
                                     torch.is_deterministic_algorithms_warn_only_enabled(), "the test's geometry")


def test_switch_defaults_off_and_explicit_values_override(flags):
    assert hip.deterministic() is False
    assert _resolve(None, True) == (False, False) and _resolve(None, False) == (False, False)
    assert _resolve(True, True) == (True, False)
    assert _resolve(False, True) == (False, False)
    assert hip.set_deterministic(True) is False and hip.deterministic() is True
    assert _resolve(None, True) == (True, False)
    assert _resolve(False, True) == (False, False) and _resolve(False, False) == (False, False)
    assert hip.set_deterministic(False) is True and hip.deterministic() is False


def test_torch_flag_is_read_at_call_time(flags):
    torch.use_deterministic_algorithms(True)
    assert _resolve(None, True) == (True, False)
    assert _resolve(False, True) == (False, False)
    torch.use_deterministic_algorithms(False)
    assert _resolve(None, True) == (False, False)


def test_non_fast_geometry_raises_under_every_request_but_warn_only(flags):
    with pytest.raises(RuntimeError, match="deterministic implementation for the test's geometry"):
        _resolve(True, False)
    hip.set_deterministic(True)
    with pytest.raises(RuntimeError, match="3x3 / stride 1 / pad 1"):
        _resolve(None, False)
    hip.set_deterministic(False)
    torch.use_deterministic_algorithms(True)
    with pytest.raises(RuntimeError):
        _resolve(None, False)
    torch.use_deterministic_algorithms(True, warn_only=True)
    assert _resolve(None, False) == (False, True)       # torch's flag alone, warn_only: warn, run the atomic path
    assert _resolve(None, True) == (True, False)
    with pytest.raises(RuntimeError):                   # an explicit request is not softened by warn_only
        _resolve(True, False)
    hip.set_deterministic(True)
    with pytest.raises(RuntimeError):                   # nor is the library's own switch
        _resolve(None, False)


def test_geometry_predicate_matches_the_library(built):
    for C, H, W, Co, geo in D.NON_FAST.values():
        assert not hip.dcn_backward_is_fast(C, *geo)
    for B, C, H, W, Co in D.PARITY_SHAPES:
        assert hip.dcn_backward_is_fast(C, *CP)


def test_ext_signature_is_unchanged_and_backward_passes_nothing_new():
    import inspect

    from centerpose_amd.lib.models.networks.DCNv2 import _ext

    assert len(inspect.signature(_ext.dcn_v2_backward).parameters) == 15
    sig = inspect.signature(hip.dcn_v2_backward)
    assert sig.parameters["deterministic"].default is None and sig.parameters["workspace"].default is None


# ---- the shared header on the host ----
def test_id_round_trip_over_the_largest_case(host):
    B, C, H, W, Co = D.CHUNKED
    n = D.plan(*D.CHUNKED).nb * H * W * 36
    assert n == 512 * 512 * 36
    assert host.dcn_det_host_roundtrip(n) == 0


def _make_sample_ref(sy, sx, H, W):
    """dcn_bwd.hip: make_sample on float32 scalars -> (in, the four corner flags, the four cells).  A NaN position passes the
    `<=` / `>=` tests and converts to corner (0, 0), as the device's conversion does."""
    inn = not (sy <= np.float32(-1) or sx <= np.float32(-1) or sy >= np.float32(H) or sx >= np.float32(W))
    if not inn:
        return False, [False] * 4, [None] * 4
    y0 = 0 if np.isnan(sy) else int(np.floor(sy))
    x0 = 0 if np.isnan(sx) else int(np.floor(sx))
    flags = [y0 >= 0 and x0 >= 0, y0 >= 0 and x0 + 1 <= W - 1, y0 + 1 <= H - 1 and x0 >= 0,
             y0 + 1 <= H - 1 and x0 + 1 <= W - 1]
    return True, flags, [(y0 + (q >> 1), x0 + (q & 1)) for q in range(4)]


def _edge_values(n):
    f = np.float32
    up, down = f(np.inf), f(-np.inf)
    return [f(np.nan), up, down, f(1e30), f(-1e30), f(3e9), f(-3e9), f(-1), np.nextafter(f(-1), up), np.nextafter(f(-1), down),
            f(n - 1), f(n), np.nextafter(f(n), up), np.nextafter(f(n), down), f(0), f(0.5), f(n - 1.5)]


def test_keys_of_edge_and_non_finite_positions_stay_in_range(host):
    H, W, bi, nb = 5, 7, 1, 2
    cells = nb * H * W
    ys, xs = _edge_values(H), _edge_values(W)
    sy = np.array([y for y in ys for _ in xs], np.float32)
    sx = np.array([x for _ in ys for x in xs], np.float32)
    n = len(sy)
    keys, valid, inn = np.zeros((n, 4), np.uint32), np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
    host.dcn_det_host_keys(sy.ctypes.data, sx.ctypes.data, n, bi, H, W, cells, keys.ctypes.data, valid.ctypes.data,
                           inn.ctypes.data)
    assert int(keys.max()) <= cells
    seen_valid = 0
    for i in range(n):
        r_in, r_flags, r_cells = _make_sample_ref(sy[i], sx[i], H, W)
        assert bool(inn[i]) == r_in, (sy[i], sx[i])
        for q in range(4):
            assert bool(valid[i, q]) == r_flags[q], (sy[i], sx[i], q)
            if r_flags[q]:
                y, x = r_cells[q]
                assert 0 <= y < H and 0 <= x < W
                assert keys[i, q] == (bi * H + y) * W + x
                seen_valid += 1
            else:
                assert keys[i, q] == cells   # the sentinel
    assert seen_valid > 0


def test_keys_of_edge_and_non_finite_offsets_stay_in_range(host):
    """The same values as offsets, on both axes, of every pixel and tap of a small chunk of two images."""
    H, W, nb = 5, 7, 2
    cells, n = nb * H * W, nb * H * W * 36
    vy, vx = _edge_values(H), _edge_values(W)
    off = np.zeros((nb, 18, H, W), np.float32)
    k = 0
    for b in range(nb):
        for tap in range(9):
            for ho in range(H):
                for wo in range(W):
                    off[b, 2 * tap, ho, wo] = vy[k % len(vy)]
                    off[b, 2 * tap + 1, ho, wo] = vx[(k // len(vy)) % len(vx)]
                    k += 1
    keys, ids = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    host.dcn_det_host_index(off.ctypes.data, nb, H, W, keys.ctypes.data, ids.ctypes.data)
    assert int(keys.max()) <= cells and np.all(np.diff(keys.astype(np.int64)) >= 0)
    assert sorted(ids.tolist()) == list(range(n))


def _lists(keys, ids, cells):
    """{cell: ids in list order} of a sorted index, the sentinel's list left out."""
    out = {}
    for k, i in zip(keys.tolist(), ids.tolist()):
        if k < cells:
            out.setdefault(k, []).append(i)
    return out


def test_one_cell_case_builds_four_ascending_lists(host):
    x, w, b, off, mask, go = D.one_cell_case()
    _, _, H, W, _ = D.ONE_CELL
    cells, n = H * W, H * W * 36
    off = np.ascontiguousarray(off.numpy())
    keys, ids = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    passes = host.dcn_det_host_index(off.ctypes.data, 1, H, W, keys.ctypes.data, ids.ctypes.data)
    assert passes == host.dcn_det_host_passes(cells) == 2   # keys 0 .. 256 need nine bits
    assert np.all(np.diff(keys.astype(np.int64)) >= 0)
    lists = _lists(keys, ids, cells)
    y, x_ = int(D.ONE_CELL_POS[0]), int(D.ONE_CELL_POS[1])
    assert sorted(lists) == sorted((y + dy) * W + x_ + dx for dy in (0, 1) for dx in (0, 1))
    valid = 0
    for pix in range(H * W):
        for tap in range(9):
            sy = np.float32(pix // W - 1 + tap // 3) + off[0, 2 * tap].reshape(-1)[pix]
            sx = np.float32(pix % W - 1 + tap % 3) + off[0, 2 * tap + 1].reshape(-1)[pix]
            assert (float(sy), float(sx)) == D.ONE_CELL_POS
            valid += sum(_make_sample_ref(sy, sx, H, W)[1])
    assert sum(len(v) for v in lists.values()) == valid == n
    for cell, lst in lists.items():
        assert len(lst) == 16 * 16 * 9 > D.CHUNK and all(a < b_ for a, b_ in zip(lst, lst[1:])), cell
        assert {i & 3 for i in lst} == {[(y + dy) * W + x_ + dx for dy in (0, 1) for dx in (0, 1)].index(cell)}


def test_radix_index_equals_a_stable_sort_by_key(host):
    """A random far-offset case: the host restatement of the device's passes against numpy's stable sort of the keys."""
    H, W, nb = 9, 13, 3
    cells, n = nb * H * W, nb * H * W * 36
    off = (6.0 * torch.randn(nb, 18, H, W, generator=torch.Generator().manual_seed(2))).numpy()
    keys, ids = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    host.dcn_det_host_index(np.ascontiguousarray(off).ctypes.data, nb, H, W, keys.ctypes.data, ids.ctypes.data)
    unsorted = np.zeros(n, np.uint32)
    unsorted[ids] = keys
    order = np.argsort(unsorted, kind="stable")
    assert np.array_equal(ids, order.astype(np.uint32)) and np.array_equal(keys, unsorted[order])
    assert 0 < int((keys == cells).sum()) < n
