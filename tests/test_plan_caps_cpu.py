"""CPU tests (no GPU) of tests/plan_cases.py: every restated launch plan is pinned to the built library through the operator's
workspace query, byte for byte, on the cap-crossing cases and on some of each operator's older cases; and every cap-crossing
case is asserted to be beyond its cap, with the plan it was chosen for.  A change to a plan constant in stem_bwd.hip,
batchnorm.hip, deconv_bwd.hip or conv_bwd.hip fails here instead of silently pulling a GPU case of
tests/test_plan_caps_gpu.py back under the cap."""
import pytest

import __graft_entry__ as ge
from centerpose_amd import hip
from tests import batchnorm_ref as BR
from tests import conv_backward_ref as CR
from tests import deconv_backward_ref as DR
from tests import plan_cases as P


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def _stem_geo(t):
    cin, cout, stride, H, W, B = t
    return (B, H, W, cin, cout, stride)


@pytest.mark.parametrize("t", list(P.STEM_CAP_CASES) + P.STEM_OLD_CASES, ids=P.stem_id)
def test_stem_plan_is_the_librarys(built, t):
    assert built.cp_conv2d_stem_backward_workspace_bytes(*_stem_geo(t)) == P.stem_workspace_bytes(*_stem_geo(t)) > 0


def test_stem_plan_on_both_sides_of_the_cap(built):
    """512 tiles are 512 slabs of one tile; 513 are 257 slabs of two (the last of one)."""
    for B, want in ((512, P.StemPlan(512, 1, 1, 512, 1)), (513, P.StemPlan(513, 1, 2, 257, 1)), (1025, P.StemPlan(1025, 1, 3, 342, 2))):
        assert P.stem_plan(B, 8, 64, 1) == want
        assert built.cp_conv2d_stem_backward_workspace_bytes(B, 8, 64, 3, 16, 1) == P.align256(want.slabs * 16 * 148 * 4)


@pytest.mark.parametrize("t", list(P.STEM_CAP_CASES), ids=P.stem_id)
def test_stem_cases_are_beyond_the_cap(t):
    cin, cout, stride, H, W, B = t
    p = P.stem_plan(B, H, W, stride)
    assert p == P.STEM_CAP_CASES[t]
    assert p.tiles > P.STEM_MAX_WG and p.tiles_per_wg >= 2 and 1 <= p.last_wg_tiles <= p.tiles_per_wg
    assert (p.slabs - 1) * p.tiles_per_wg + p.last_wg_tiles == p.tiles
    Ho, Wo = CR.out_size(P.stem_case(t))
    assert Wo % P.STEM_TILE_COLS   # a ragged column band
    if t == list(P.STEM_CAP_CASES)[0]:
        assert Ho % P.STEM_TILE_ROWS   # and a ragged row band
    if p.tiles_per_image % p.tiles_per_wg:
        assert p.tiles_per_image > p.tiles_per_wg   # a run crosses an image boundary after starting inside the image
    CR.dyadic_inputs(0, P.stem_case(t))   # asserts the premise of exactness


def test_pool_cases_are_beyond_one_grid_pass():
    assert P.POOL_GRID_ITEMS == 1048576
    assert P.POOL_H % 2 and P.POOL_W % 2 and P.POOL_C % 4 == 0
    for geo, want in P.POOL_CAP_CASES.items():
        fwd, bwd = P.pool_items(P.POOL_B, P.POOL_C, P.POOL_H, P.POOL_W, geo)
        assert (fwd, bwd) == want
        assert P.POOL_GRID_ITEMS < fwd < 2 * P.POOL_GRID_ITEMS and bwd > 4 * P.POOL_GRID_ITEMS
    # the largest case of tests/test_pool_gpu.py stays inside one pass
    assert max(P.pool_items(2, 36, 8, 8, (2, 2, 0))) < P.POOL_GRID_ITEMS


def _conv_geo(c):
    return (c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.stride, c.pad)


@pytest.mark.parametrize("c", list(P.CONV_CAP_CASES) + P.CONV_OLD_CASES + CR.dla34_shapes(32)[:6], ids=CR.case_id)
def test_conv_plan_is_the_librarys(built, c):
    assert built.cp_conv2d_backward_workspace_bytes(*_conv_geo(c), 0) == P.conv_workspace_bytes(c) > 0


@pytest.mark.parametrize("c", list(P.CONV_CAP_CASES), ids=CR.case_id)
def test_conv_cases_are_beyond_the_cap(c):
    s = P.conv_stage_plan(c)
    assert s == P.CONV_CAP_CASES[c]
    assert CR.is_mfma(c) and s.Q > 512 * 64 and s.st_px > 64 and s.st_slabs <= s.st_bound == 512
    # the largest stage of tests/conv_backward_ref.py is at the cap, not beyond it
    assert max(P.conv_stage_plan(o).st_px for o in CR.CASES) == 64
    CR.dyadic_inputs(0, c)   # asserts the premise of exactness


def test_conv_slab_plan_restated():
    """The weight-gradient slabs of one case by hand: 64 -> 64 3x3 on 2 x 128 x 128: CoP 64 (two co tiles per wave), 18 k tiles
    in 9 pairs, so 9 jobs, ceil(2048 / 9) = 228 slabs wanted of the 256 rows: 2 rows per slab, 128 slabs."""
    p = P.conv_slab_plan(CR.MFMA_CASES[0])
    assert p == P.ConvSlabPlan(228, 2, 128, 228 * 64 * 9 * 64 * 4)


@pytest.mark.parametrize("c", list(P.BN_CAP_CASES) + P.BN_OLD_CASES, ids=lambda c: "B%d_%dx%d_C%d" % c)
def test_bn_plan_is_the_librarys(built, c):
    assert built.cp_batchnorm_workspace_bytes(*c) == P.bn_workspace_bytes(*c) > 0


@pytest.mark.parametrize("c", list(P.BN_CAP_CASES), ids=lambda c: "B%d_%dx%d_C%d" % c)
def test_bn_cases_are_beyond_the_cap(c):
    p = P.bn_plan(*c)
    assert p == P.BN_CAP_CASES[c]
    assert p.steps > 8 * p.red_bound and p.red_bound == 2048 // p.npass
    assert p.red_px // p.S > 8 and p.red_slabs < p.red_bound
    assert P.BN_LARGE_MEAN_CASE in P.BN_CAP_CASES
    # every older case has exactly eight steps per slab (or a single short slab)
    assert all(P.bn_plan(*o).red_px // P.bn_plan(*o).S <= 8 for o in BR.CASES + BR.LARGE_MEAN_CASES)


def _dw_geo(c):
    return (c.B, c.H, c.W, c.Cin, c.stride)


@pytest.mark.parametrize("c", list(P.DW_CAP_CASES) + P.DW_OLD_CASES, ids=DR.case_id)
def test_dw_plan_is_the_librarys(built, c):
    for need_x in (0, 1):
        assert built.cp_conv_transpose2d_backward_workspace_bytes(*DR.geo(c), need_x) == P.dw_workspace_bytes(*_dw_geo(c)) > 0


@pytest.mark.parametrize("c", list(P.DW_CAP_CASES), ids=DR.case_id)
def test_dw_cases_are_beyond_the_cap(c):
    p = P.dw_plan(*_dw_geo(c))
    assert p == P.DW_CAP_CASES[c]
    assert p.rounds > 8 * 1024 and p.want == 1024 and p.rounds_per_slab > 8 and p.slabs <= p.want
    assert c.B * c.H * c.W * c.stride ** 2 * c.Cin < 2 ** 30   # the kernel's 32-bit byte offsets
    assert all(P.dw_plan(*_dw_geo(o)).rounds_per_slab <= 8 for o in DR.DW_CASES)
