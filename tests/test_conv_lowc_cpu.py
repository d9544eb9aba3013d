"""CPU tests (no GPU) of the low-channel 3x3 conv backward path (conv_bwd_lowc.hip): which geometries cp_conv2d_backward_path
sends where, the path's workspace plan restated in tests/conv_lowc_cases.py against the library's query byte for byte, the
unchanged queries of every older case, and the premises of the GPU cases (tests/test_conv_lowc_gpu.py)."""
import pytest

import __graft_entry__ as ge
from centerpose_amd import hip
from tests import conv_backward_ref as CR
from tests import conv_lowc_cases as LC
from tests import plan_cases as P


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


@pytest.mark.parametrize("c", LC.ALL_LOWC, ids=CR.case_id)
def test_new_cases_take_the_lowc_path(built, c):
    assert LC.expected_path(c) == LC.LOWC
    assert built.cp_conv2d_backward_path(*LC.geo(c)) == LC.LOWC == hip.CONV_BWD_LOWC
    assert hip.conv2d_backward_path(*LC.geo(c)) == LC.LOWC


def test_older_cases_keep_their_paths(built):
    for c in CR.GENERIC_CASES + [LC.BELOW_CASE]:
        assert built.cp_conv2d_backward_path(*LC.geo(c)) == LC.GENERIC == hip.CONV_BWD_GENERIC, c
    for c in CR.MFMA_CASES + CR.PADDED_CASES:
        assert built.cp_conv2d_backward_path(*LC.geo(c)) == LC.MFMA == hip.CONV_BWD_MFMA, c
    for c in CR.CASES + CR.dla34_shapes(16) + [LC.BELOW_CASE]:
        assert built.cp_conv2d_backward_path(*LC.geo(c)) == LC.expected_path(c) != LC.LOWC, c


def test_each_condition_of_the_predicate(built):
    """One step away from a low-channel geometry in every direction is another path."""
    base = dict(B=1, H=64, W=64, Cin=16, Cout=16, KH=3, KW=3, stride=1, pad=1)
    q = lambda **kw: built.cp_conv2d_backward_path(*{**base, **kw}.values())
    assert q() == LC.LOWC and q(Cout=32) == LC.LOWC and q(stride=2, B=4) == LC.LOWC
    assert q(stride=2, B=3) == LC.GENERIC          # 3 x 32 x 32 = 3072 output pixels
    assert q(H=63) == LC.GENERIC and q(stride=3, B=16) == LC.GENERIC
    assert q(Cout=24) == LC.GENERIC and q(Cout=48) == LC.GENERIC and q(Cin=8) == LC.GENERIC
    assert q(pad=0) == LC.GENERIC and q(pad=2) == LC.GENERIC and q(KH=5, KW=5, pad=1) == LC.GENERIC
    assert q(KH=1, KW=1, pad=0) == LC.GENERIC and q(Cin=32) == LC.MFMA
    # the tracking task's 8-plane 7x7 stem stays where it is
    assert q(Cin=8, KH=7, KW=7, pad=3, H=512, W=512) == LC.GENERIC


def test_refused_geometries_are_errors(built):
    for bad in ((0, 64, 64, 16, 16, 3, 3, 1, 1), (1, 64, 64, 6, 16, 3, 3, 1, 1), (1, 64, 64, 16, 16, 3, 3, 5, 1),
                (1, 1, 1, 16, 16, 3, 3, 1, 0)):
        assert built.cp_conv2d_backward_path(*bad) == -1   # CP_ERR_INVALID
        assert built.cp_conv2d_backward_workspace_bytes(*bad, 1) == 0
        with pytest.raises(RuntimeError, match="refused"):
            hip.conv2d_backward_path(*bad)


@pytest.mark.parametrize("c", LC.ALL_LOWC, ids=CR.case_id)
def test_lowc_plan_is_the_librarys(built, c):
    for need_x in (0, 1):
        assert built.cp_conv2d_backward_workspace_bytes(*LC.geo(c), need_x) == LC.workspace_bytes(c, need_x) > 0


def test_lowc_plan_by_hand():
    """2 x 37 x 131 at stride 1: 5 x 3 weight-gradient tiles per image, 30 slabs of 16 x 144 floats; the generic plan's 64
    slabs are the larger buffer.  dla_34's level0 at B = 16: 8192 tiles, eight per workgroup, 1024 slabs."""
    c = LC.LOWC_CASES[0]
    assert LC.wgrad_plan(c) == LC.RunPlan(30, 15, 1, 30, 1)
    assert LC.workspace_bytes(c, 1) == P.align256(2 * 37 * 131 * 16 * 4) + P.align256(152 * 16 * 4) + 64 * 16 * 144 * 4
    big = CR._c(16, 16, 16, 512, 512, 3, 1)
    assert LC.wgrad_plan(big) == LC.RunPlan(8192, 512, 8, 1024, 8) and LC.dgrad_plan(big) == LC.RunPlan(16384, 1024, 16, 1024, 16)
    assert LC.workspace_bytes(big, 0) == 16 * 512 * 512 * 16 * 4 + 512 * 16 * 4 + 1024 * 16 * 144 * 4


@pytest.mark.parametrize("c", CR.CASES + [LC.BELOW_CASE], ids=CR.case_id)
def test_unchanged_queries(built, c):
    assert built.cp_conv2d_backward_workspace_bytes(*LC.geo(c), 0) == P.conv_workspace_bytes(c) > 0


@pytest.mark.parametrize("cout,stride,H,W", [(16, 1, 40, 40), (32, 1, 40, 40), (32, 2, 75, 75), (16, 2, 64, 70)])
def test_query_is_monotone_in_batch_across_the_floor(built, cout, stride, H, W):
    geo = lambda B: (B, H, W, 16, cout, 3, 3, stride, 1)
    paths = [built.cp_conv2d_backward_path(*geo(B)) for B in range(1, 9)]
    assert paths[0] == LC.GENERIC and paths[-1] == LC.LOWC and paths == sorted(paths)   # crosses 4096 pixels inside 1..8
    for need_x in (0, 1):
        q = [built.cp_conv2d_backward_workspace_bytes(*geo(B), need_x) for B in range(1, 9)]
        assert all(a <= b for a, b in zip(q, q[1:])) and q[0] > 0, q


@pytest.mark.parametrize("c", list(LC.LOWC_CAP_CASES), ids=CR.case_id)
def test_cap_cases_are_beyond_the_cap(c):
    for p, want in zip((LC.wgrad_plan(c), LC.dgrad_plan(c)), LC.LOWC_CAP_CASES[c]):
        assert p == want
        assert p.tiles > LC.LOWC_MAX_WG and p.tiles_per_wg >= 2 and 1 <= p.last_wg_tiles < p.tiles_per_wg
        assert (p.wgs - 1) * p.tiles_per_wg + p.last_wg_tiles == p.tiles
        assert p.tiles_per_image % p.tiles_per_wg   # runs cross image boundaries
    Ho, Wo = CR.out_size(c)
    assert Ho % LC.WG_TILE_ROWS and Wo % LC.WG_TILE_COLS[c.stride]   # ragged tiles in both directions
    assert c.B * c.H * c.W * c.Cin * 4 <= 40 << 20 and c.B * Ho * Wo * c.Cout * 4 <= 40 << 20
    # every other case stays below the cap: one tile per workgroup
    assert all(LC.wgrad_plan(o).tiles_per_wg == 1 and LC.dgrad_plan(o).tiles_per_wg == 1 for o in LC.LOWC_CASES)


@pytest.mark.parametrize("c", LC.ALL_LOWC + [LC.BELOW_CASE], ids=CR.case_id)
def test_exactness_premise(c):
    CR.dyadic_inputs(0, c)   # asserts the premise of exactness
