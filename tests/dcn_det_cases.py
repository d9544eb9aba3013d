"""Cases of the deterministic DCNv2 backward (cp_dcnv2_backward_det) and its launch plan restated in Python (test helper, not
a test module; tests/test_dcn_backward_det_{cpu,gpu}.py).  The plan mirror -- dcn_bwd.hip: plan, dcn_bwd_carve, dcn_det_carve --
gives the images per grad_col chunk (`nb`) and the workspace bytes; the CPU test pins it to the built library byte for byte,
so the GPU test can assert from it which side of the 256 MiB chunk cap a case is on."""
import collections

import torch

from tests.plan_cases import _cdiv, align256

CP = (3, 3, 1, 1, 1, 1, 1, 1, 1)
NAMES = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")
RS_TILE, SCAN_SEG, CHUNK = 4096, 4096, 512   # dcn_bwd.hip: RS_TILE, SCAN_SEG; dcn_bwd_det_common.h: DCN_DET_CHUNK

# (B, C, H, W, Co), geometry CP
PARITY_SHAPES = [
    (2, 16, 13, 21, 16),    # odd sides, C % 32 != 0
    (2, 64, 32, 32, 64),
    (1, 128, 16, 16, 32),
    (1, 512, 8, 8, 32),     # lanes loop over the channels
    (3, 32, 9, 40, 16),
]
PARITY_STDS = [0.5, 2.0, 6.0]
SMALL = (2, 16, 10, 10, 16)            # std 0 and zero_mask
REPRO = (2, 64, 48, 48, 64)            # the existing reproducibility case, std 2.0, seed 9
BATCH = (3, 32, 9, 40, 16)             # independence of the batch, std 2.0
ONE_CELL = (1, 16, 16, 16, 16)
ONE_CELL_POS = (7.25, 7.5)
CHUNKED = (2, 16, 512, 512, 16)        # the smallest C = 16 shape whose two images fit no grad_col chunk
# non-fast geometries, one of each kind from tests/test_dcn_backward_gpu.py: GENERIC -> (C, H, W, Co, geometry)
NON_FAST = {
    "5x5": (8, 9, 11, 5, (5, 5, 1, 1, 2, 2, 1, 1, 1)),
    "stride2": (8, 12, 13, 7, (3, 3, 2, 2, 1, 1, 1, 1, 1)),
    "dilation2": (16, 11, 9, 20, (3, 3, 1, 1, 2, 2, 2, 2, 1)),
    "two_groups": (8, 10, 10, 6, (3, 3, 1, 1, 1, 1, 1, 1, 2)),
    "C24": (24, 8, 8, 33, CP),
}

Plan = collections.namedtuple("Plan", "nb nslab slab_px")


def plan(B, C, H, W, Co):
    """dcn_bwd.hip: plan, on the fast geometry (Ho = H, Wo = W, T = 9)."""
    HW, TC = H * W, 9 * C
    Q = B * HW
    nb = max(1, min(B, (256 << 20) // (TC * HW * 4)))
    tiles = _cdiv(TC, 32) * _cdiv(Co, 128)
    ns = _cdiv(8192, tiles)
    ns = min(ns, max(1, (64 << 20) // (Co * TC * 4)))
    ns = max(1, min(ns, _cdiv(Q, 64)))
    spx = (_cdiv(Q, ns) + 1) & ~1
    return Plan(nb, _cdiv(Q, spx), spx)


def default_workspace_bytes(B, C, H, W, Co):
    """dcn_bwd_carve: wt, go_t, xh, gin, gcol, slab."""
    P, HW, TC = plan(B, C, H, W, Co), H * W, 9 * C
    return (align256(Co * TC * 4) + align256(B * HW * Co * 4) + 2 * align256(B * HW * C * 4) + align256(P.nb * TC * HW * 4)
            + align256(P.nslab * Co * TC * 4))


def det_workspace_bytes(B, C, H, W, Co):
    """+ dcn_det_carve: keys and ids twice (16 bytes an entry), the digit table and its segment sums, the lists' bounds,
    the partial rows."""
    cells = plan(B, C, H, W, Co).nb * H * W
    n = cells * 36
    m = 256 * _cdiv(n, RS_TILE)
    return (default_workspace_bytes(B, C, H, W, Co) + 4 * align256(n * 4) + align256(m * 4) + align256(_cdiv(m, SCAN_SEG) * 4)
            + align256(cells * 8) + align256(_cdiv(n, CHUNK) * C * 4))


def one_cell_case(seed=11):
    """ONE_CELL with every offset set so that every tap of every pixel samples ONE_CELL_POS: the four cells around it
    receive 16 * 16 * 9 = 2304 entries each (past the 64 and the 512 boundaries), every other cell none.  The positions are
    exact in float32 (quarter-integers minus small integers)."""
    from tests.test_dcn_backward_gpu import _case

    B, C, H, W, Co = ONE_CELL
    x, w, b, off, mask, go = _case(B, C, H, W, Co, CP, 1.0, seed=seed)
    ho = torch.arange(H, dtype=torch.float32).view(H, 1).expand(H, W)
    wo = torch.arange(W, dtype=torch.float32).view(1, W).expand(H, W)
    for tap in range(9):
        i, j = divmod(tap, 3)
        off[0, 2 * tap] = ONE_CELL_POS[0] - (ho - 1 + i)
        off[0, 2 * tap + 1] = ONE_CELL_POS[1] - (wo - 1 + j)
    return x, w, b, off, mask, go
