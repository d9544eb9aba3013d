"""Cases of the low-channel 3x3 conv backward path and its launch plans restated in Python (test helper, not a test module;
tests/test_conv_lowc_{cpu,gpu}.py), in the manner of tests/plan_cases.py.

conv_bwd_lowc.hip takes 3x3 / pad 1, stride 1 | 2, 16 -> 16 | 32 channels from 4096 output pixels on.  Both its kernels give a
workgroup a contiguous run of tiles, at most LOWC_MAX_WG workgroups; the weight gradient's workgroups are its slabs
[Cout][9 x 16], and the workspace reserves min(tiles, LOWC_MAX_WG) of them, or the generic plan's buffer where that is larger
(so that the query stays monotone in B across the pixel floor).  The data gradient needs no workspace; its plan is restated
for the cap-crossing cases only.
"""
import collections

from tests import conv_backward_ref as CR
from tests import plan_cases as P

GENERIC, MFMA, LOWC = 0, 1, 2   # include/centerpose_hip.h: CP_CONV_BWD_*
LOWC_MIN_PIXELS = 4096
LOWC_MAX_WG = 1024
WG_TILE_ROWS = 8
WG_TILE_COLS = {1: 64, 2: 16}    # output columns of a weight-gradient tile, per stride
DG_TILE_ROWS, DG_TILE_COLS = 8, 32   # data gradient: input pixels (stride 1), parity-class coordinates (stride 2)

_c = CR._c
LOWC_CASES = [
    _c(2, 16, 16, 37, 131, 3, 1),   # ragged tiles in both directions, several tiles per row and per column
    _c(1, 16, 32, 70, 66, 3, 1),
    _c(2, 16, 32, 75, 133, 3, 2),   # odd H and W: unequal parity classes, the last output row and column read the pad
    _c(3, 16, 16, 81, 67, 3, 2),
    _c(1, 16, 16, 64, 64, 3, 1),    # exactly 4096 output pixels
]
BELOW_CASE = _c(1, 16, 16, 63, 65, 3, 1)   # 4095 output pixels: the generic path

RunPlan = collections.namedtuple("RunPlan", "tiles tiles_per_image tiles_per_wg wgs last_wg_tiles")
# beyond the cap: a workgroup walks several tiles, runs cross image boundaries, the last workgroup walks fewer
# case -> (weight-gradient plan, data-gradient plan)
LOWC_CAP_CASES = {
    _c(515, 16, 16, 9, 131, 3, 1): (RunPlan(3090, 6, 4, 773, 2), RunPlan(5150, 10, 6, 859, 2)),
    _c(515, 16, 32, 17, 67, 3, 2): (RunPlan(3090, 6, 4, 773, 2), RunPlan(2060, 4, 3, 687, 2)),
}
ALL_LOWC = LOWC_CASES + list(LOWC_CAP_CASES)


def is_lowc(c):
    Ho, Wo = CR.out_size(c)
    return (c.k == 3 and c.pad == 1 and c.stride in (1, 2) and c.Cin == 16 and c.Cout in (16, 32)
            and c.B * Ho * Wo >= LOWC_MIN_PIXELS)


def expected_path(c):
    return MFMA if CR.is_mfma(c) else LOWC if is_lowc(c) else GENERIC


def _run_plan(B, ty, tx):
    tiles = B * ty * tx
    per_wg = P._cdiv(tiles, LOWC_MAX_WG)
    wgs = P._cdiv(tiles, per_wg)
    return RunPlan(tiles, ty * tx, per_wg, wgs, tiles - (wgs - 1) * per_wg)


def wgrad_plan(c):
    Ho, Wo = CR.out_size(c)
    return _run_plan(c.B, P._cdiv(Ho, WG_TILE_ROWS), P._cdiv(Wo, WG_TILE_COLS[c.stride]))


def dgrad_plan(c):
    hj, wj = (c.H, c.W) if c.stride == 1 else ((c.H + 1) // 2, (c.W + 1) // 2)
    return _run_plan(c.B, P._cdiv(hj, DG_TILE_ROWS), P._cdiv(wj, DG_TILE_COLS))


def workspace_bytes(c, need_grad_x):
    """cp_conv2d_backward_workspace_bytes on the low-channel path: the staged grad_out and the stage slabs' column sums as on
    the other paths (CoP == Cout), the weight-gradient slabs, and no data-gradient operand whatever need_grad_x says."""
    assert is_lowc(c) and need_grad_x in (0, 1)
    s = P.conv_stage_plan(c)
    assert s.CoP == c.Cout
    slab = min(wgrad_plan(c).tiles, LOWC_MAX_WG) * c.Cout * 144 * 4
    return P.align256(s.Q * s.CoP * 4) + P.align256(s.st_bound * s.CoP * 4) + P.align256(max(slab, P.conv_slab_plan(c).slab_bytes))


def geo(c):
    return (c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.stride, c.pad)
