"""The decode edge-case helper (tests/decode_edge_cases.py) checked on the CPU: its reference against a second route, its
restatement of decode.hip's control flow against a per-pixel brute force and against the library's own workspace
arithmetic, and every named case against the branch its name promises.  test_decode_edges_gpu.py runs the same maps
through the kernels."""
import struct

import numpy as np
import pytest

from centerpose_amd import hip
from oracle import decode as odec
from tests import decode_edge_cases as E

K = E.K_CASE
SMALL = E.ONE_WG_SHAPES + E.SEAM_SHAPES + ((264, 128),)


def _cases():
    """(shape, recipe): every recipe at the small shapes, the named ones at the large."""
    out = [(s, n) for s in SMALL for n in E.recipes(*s, K)]
    out += [(s, n) for _, n, s, _, _ in E.COVERAGE if (s, n) not in out]
    return out


@pytest.fixture(scope="module")
def maps():
    return {(s, n): E.recipes(*s, K)[n] for s, n in _cases()}


def test_constructors_give_float32_dyadics(maps):
    for (s, n), m in maps.items():
        assert m.dtype == np.float32 and m.shape == s and np.isfinite(m).all(), (s, n)
        if "ladder" not in n:
            assert np.array_equal(m * 256, np.round(m * 256)), (s, n)   # multiples of 1/256
    lad = E.ladder(64, 128, 129)
    top = np.sort(lad[lad > 0]).view(np.uint32)
    assert np.array_equal(np.diff(top), np.ones(128, np.uint32))   # one ulp apart: only the low byte differs
    ex = E.exponent_ladder(64, 128)
    bits = np.sort(ex[ex > 0]).view(np.uint32)
    assert bits[0] == 1 and np.all(bits[1:] & 0x7fffff == 0) and len(set(bits[1:] >> 24)) > 16   # a denormal, powers of two


def test_lexsort_reference_equals_the_oracles_topk(maps):
    """Two independent routes to (value desc, pixel index asc): np.lexsort and the oracle's stable argsort."""
    for (s, n), m in maps.items():
        v, i = E.reference_peaks(m, K)
        ov, oi, _, _ = odec.topk_channel(odec.nms(m[None, None]), K)
        np.testing.assert_array_equal(i, oi[0, 0], err_msg=str((s, n)))
        np.testing.assert_array_equal(v, ov[0, 0], err_msg=str((s, n)))


def test_restatement_selects_what_the_reference_selects(maps):
    for (s, n), m in maps.items():
        for k in (1, 100, K):
            v, i = E.reference_peaks(m, k)
            if m.size <= E.ONE_WG_MAX:
                np.testing.assert_array_equal(E.one_workgroup(m, k)["ind"], i, err_msg=str((s, n, k)))
            if s not in E.ONE_WG_SHAPES:
                np.testing.assert_array_equal(E.tiled(m, k)["ind"], i, err_msg=str((s, n, k)))


def _bits(f):
    return struct.unpack("<I", struct.pack("<f", f))[0]


def test_nms_keys_equal_a_per_pixel_brute_force():
    H, W = 12, 8
    rng = np.random.RandomState(5)
    for m in (rng.randint(-4, 5, (H, W)).astype(np.float32) / 4, E.near_flat(H, W, 20, 2, 1, strict=False),
              E.staircase(H, W), -E.staircase(H, W)):
        want = np.zeros((H, W), np.uint32)
        for y in range(H):
            for x in range(W):
                v = float(m[y, x])
                mx = max(float(m[yy, xx]) for yy in range(max(y - 1, 0), min(y + 2, H))
                         for xx in range(max(x - 1, 0), min(x + 2, W)))
                b = _bits((v if mx == v else 0.0) + 0.0)   # a zero of either sign, kept or suppressed, is +0
                want[y, x] = (~b & 0xffffffff) if b & 0x80000000 else b | 0x80000000
        assert np.array_equal(E.nms_keys(m), want)


@pytest.mark.parametrize("feature,recipe,shape,route,pred", E.COVERAGE, ids=[c[0] for c in E.COVERAGE])
def test_named_case_reaches_its_branch(feature, recipe, shape, route, pred):
    assert pred(E.reach(recipe, shape, route)), (feature, recipe, shape)


def test_coverage_list_is_complete():
    """Every item the suite promises to reach is named, and every shape of the GPU tests takes the route it is listed for."""
    assert [c[0] for c in E.COVERAGE] == [
        "positive class, all_eq", "positive class, partial tie", "zero class, need 1; tot_pos K-1",
        "zero class, need K-1; H*W == K", "zero class, need K; tot_pos + tot_zero K",
        "general class, mixed values, partial tie", "general class, H*W == K", "tot_pos K", "tot_pos K+1",
        "tot_pos + tot_zero K-1", "tie from element 1 of a float4; crosses pixel 4096 in peaks_kernel<4>",
        "tie from element 2; crosses pixel 16384 in peaks_kernel<8>", "tie from element 3",
        "tie crosses pixel 4096 of a band", "tie starts at the first pixel of band 1",
        "tie starts in the last row of band 0 and crosses the seam", "halo row alone suppresses a band's first row",
        "tie in merge group >= 1 while group 0's positives win", "taken ties cross merge groups 0 -> 1",
        "last band with rows*W < K", "merge <1>", "merge <2>", "merge <4>", "merge <8>", "merge <16>"]
    for H, W in E.ONE_WG_SHAPES:
        assert K <= H * W <= E.ONE_WG_MAX
    want = {(264, 128): (64, 5, 1), (34, 4096): (2, 17, 2), (66, 4096): (2, 33, 4), (130, 4096): (2, 65, 8),
            (256, 4096): (2, 128, 8), (260, 2732): (2, 130, 16), (1024, 1024): (8, 128, 8), (66, 128): (64, 2, 1),
            (2049, 4): (2048, 2, 1)}
    for (H, W), (R, T, G) in want.items():
        r, t, ns = E.tiled_geom(H, W, K)
        assert (r, t, E.merge_instantiation(ns)) == (R, T, G), (H, W)
    assert E.tiled_geom(66, 4096, K)[2] == 4224 and E.tiled_geom(256, 4096, K)[2] == 16384
    assert E.tiled_geom(260, 2732, K)[2] == 16640 and 256 * 4096 == 1024 * 1024 == 1 << 20
    assert set(E.TILED_PEAK_SHAPES) | set(E.SEAM_SHAPES) == set(want)


def test_tiled_geom_agrees_with_the_workspace_query():
    L = hip.lib()
    for H, W in E.all_shapes():
        for B, k in ((1, 1), (1, 100), (1, K), (2, K)):
            _, _, NS = E.tiled_geom(H, W, k)
            peaks = (B * 9 * k * 8 + 255) & ~255
            assert L.cp_decode_tiled_workspace_bytes(B, H, W, k) == peaks + B * 9 * NS * 8 + 256, (H, W, B, k)


def _oracle(d):
    return odec.object_pose_decode(d["hm"], d["hps"], wh=d["wh"], obj_scale=d["scale"], reg=d["reg"], hm_hp=d["hm_hp"],
                                   hp_offset=d["hp_offset"], K=E.ASSOC_K, rep_mode=1)


def test_association_case_lands_on_its_boundaries():
    """The hand-built 16 x 16 frame: the oracle's records are what each scenario says, so every comparison of assoc_kernel
    named there sits exactly on its boundary."""
    d = E.assoc_case()
    assert all(v.dtype == np.float32 for v in d.values())
    E.assoc_check(d, _oracle(d))
    # every joint peak survives the NMS: no two are neighbours
    for j, peaks in E._PEAKS.items():
        kept = odec.nms(d["hm_hp"][:, j:j + 1])[0, 0]
        assert all(kept[y, x] == np.float32(s) for x, y, s in peaks), j


def test_association_case_right_of_the_map_raises_in_the_oracle_only_there():
    d, without, (k, j) = E.assoc_beyond_right_edge()
    with pytest.raises(IndexError):
        _oracle(d)
    inside = {n: v.copy() for n, v in d.items()}
    inside["hp_offset"][0, 0, E.BEYOND[2][1], E.BEYOND[2][0]] = 0.5   # the same peak half a pixel inside the map
    a, b = _oracle(inside), _oracle(without)
    for n in a:   # the extra joint peak moves that joint of that record and nothing else
        diff = np.argwhere(a[n] != b[n])
        assert all(tuple(i[:2]) == (0, k) and i[2] // (1 if a[n].shape[2] == 8 else 2) == j for i in diff), (n, diff)
