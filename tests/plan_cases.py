"""Launch plans of the training operators restated in Python, and the cases that cross their caps (test helper, not a test
module; tests/test_plan_caps_{cpu,gpu}.py).

Every training operator sizes its launch from a small host-side plan with a cap: below the cap a workgroup gets a fixed small
amount of work (one tile, eight row steps, 64 pixels), above it the workgroup loops.  The functions below restate those plans
-- stem_bwd.hip: stem_plan, batchnorm.hip: plan, deconv_bwd.hip: dw_plan, conv_bwd.hip: plan / slab_plan -- so that a test can
assert which side of the cap its case is on; tests/test_plan_caps_cpu.py pins each of them to the built library through the
workspace queries, byte for byte.  The max-pool has no workspace to pin it with: POOL_GRID_ITEMS restates pool.hip: grid_for.
"""
import collections

from tests import batchnorm_ref, conv_backward_ref, deconv_backward_ref


def _cdiv(a, b):
    return (a + b - 1) // b


def align256(n):
    """op_common.h: Carve rounds every region up to 256 bytes."""
    return _cdiv(n, 256) * 256


# ---- image stems (stem_bwd.hip: TR, TCW, MAX_WG, stem_plan) ----
STEM_TILE_ROWS, STEM_TILE_COLS, STEM_MAX_WG = 8, 64, 512
StemPlan = collections.namedtuple("StemPlan", "tiles tiles_per_image tiles_per_wg slabs last_wg_tiles")


def stem_plan(B, H, W, stride):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    per_image = _cdiv(Ho, STEM_TILE_ROWS) * _cdiv(Wo, STEM_TILE_COLS)
    tiles = B * per_image
    tiles_per_wg = _cdiv(tiles, STEM_MAX_WG)
    slabs = _cdiv(tiles, tiles_per_wg)
    return StemPlan(tiles, per_image, tiles_per_wg, slabs, tiles - (slabs - 1) * tiles_per_wg)


def stem_workspace_bytes(B, H, W, Cin, Cout, stride):
    return align256(stem_plan(B, H, W, stride).slabs * Cout * (49 * Cin + 1) * 4)


def stem_case(t):
    cin, cout, stride, H, W, B = t
    return conv_backward_ref.Case(B, cin, cout, H, W, 7, stride, 3)


def stem_id(t):
    return "%dto%d_s%d_%dx%d_B%d" % t


# (Cin, Cout, stride, H, W, B) -> the plan the case was chosen for
STEM_CAP_CASES = {
    # 8 x 2 tiles per image, ragged in both directions; runs of 3 tiles cross tile rows and images, the last run has 2
    (3, 16, 1, 60, 70, 65): StemPlan(1040, 16, 3, 347, 2),
    # output 16 x 70, the widest accumulator instance (four co tiles)
    (1, 64, 2, 31, 140, 129): StemPlan(516, 4, 2, 258, 2),
}
# cases of tests/test_stem_gpu.py, all one tile per workgroup
STEM_OLD_CASES = [(3, 16, 1, 9, 11, 2), (3, 64, 2, 10, 13, 2), (3, 16, 1, 70, 66, 3)]

# ---- max-pool (pool.hip: grid_for: at most 256 * 16 workgroups of TPB = 256 threads, one float4 item per thread and pass) ----
POOL_GRID_ITEMS = 4096 * 256
POOL_B, POOL_C, POOL_H, POOL_W = 8, 64, 131, 257
# (kernel, stride, padding) -> (forward items, backward items): float4s of the output, resp. of grad_x
POOL_CAP_CASES = {(2, 2, 0): (1064960, 4309376), (3, 2, 1): (1089792, 4309376)}


def pool_items(B, C, H, W, geo):
    k, s, p = geo
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return B * Ho * Wo * (C // 4), B * H * W * (C // 4)


# ---- conv backward (conv_bwd.hip: plan, slab_plan, cp_conv_wgrad_plan) ----
ConvStagePlan = collections.namedtuple("ConvStagePlan", "Q CoP st_bound st_px st_slabs")
ConvSlabPlan = collections.namedtuple("ConvSlabPlan", "ns rows_per_slab slabs slab_bytes")


def conv_stage_plan(c):
    """stage_kernel / bias_reduce_kernel: at most 512 slabs of at least 64 pixels."""
    Ho, Wo = conv_backward_ref.out_size(c)
    Q = c.B * Ho * Wo
    CoP = _cdiv(c.Cout, 32) * 32 if conv_backward_ref.is_mfma(c) else c.Cout
    st_bound = max(1, min(512, _cdiv(Q, 64)))
    st_px = _cdiv(Q, st_bound)
    return ConvStagePlan(Q, CoP, st_bound, st_px, _cdiv(Q, st_px))


def conv_slab_plan(c):
    """The weight gradient's slabs of whole output rows: at most 64 MiB and one per row; the MFMA path wants about two waves
    per SIMD (2048 jobs) and at most 512 slabs, the generic path 64."""
    Ho, _ = conv_backward_ref.out_size(c)
    rows, taps = c.B * Ho, c.k * c.k
    CoP = conv_stage_plan(c).CoP
    wbytes = CoP * taps * c.Cin * 4
    if conv_backward_ref.is_mfma(c):
        nh = 4 if CoP % 128 == 0 else 2 if CoP % 64 == 0 else 1
        jobs = (CoP // (32 * nh)) * _cdiv(taps * c.Cin // 32, 2)
        ns = min(512, _cdiv(2048, jobs))
    else:
        ns = 64
    ns = min(ns, max(1, (64 << 20) // wbytes))
    ns = max(1, min(ns, rows))
    rows_per_slab = _cdiv(rows, ns)
    return ConvSlabPlan(ns, rows_per_slab, _cdiv(rows, rows_per_slab), ns * wbytes)


def conv_workspace_bytes(c):
    """cp_conv2d_backward_workspace_bytes with need_grad_x = 0 (the packed-weight region is then empty): the staged grad_out,
    the stage slabs' column sums, the weight-gradient slabs."""
    s = conv_stage_plan(c)
    return align256(s.Q * s.CoP * 4) + align256(s.st_bound * s.CoP * 4) + align256(conv_slab_plan(c).slab_bytes)


_c = conv_backward_ref._c
CONV_CAP_CASES = {
    _c(1, 32, 40, 182, 182, 1, 1): ConvStagePlan(33124, 64, 512, 65, 510),   # pad lanes (Cout 40)
    _c(2, 32, 64, 259, 260, 3, 2): ConvStagePlan(33800, 64, 512, 67, 505),   # output 130 x 130; the stride-2 data gradient
}
CONV_OLD_CASES = [conv_backward_ref.MFMA_CASES[0], conv_backward_ref.MFMA_CASES[1], conv_backward_ref.MFMA_CASES[12],
                  conv_backward_ref.PADDED_CASES[0], conv_backward_ref.GENERIC_CASES[0], conv_backward_ref.GENERIC_CASES[2]]

# ---- BatchNorm (batchnorm.hip: lane_of, plan) ----
BnPlan = collections.namedtuple("BnPlan", "S npass steps red_bound red_px red_slabs")


def bn_plan(B, H, W, C):
    L = C // 4
    CL = min(L, 64)
    npass = _cdiv(L, 64)
    S = 4 * (64 // CL)
    P = B * H * W
    steps = _cdiv(P, S)
    red_bound = max(1, min(_cdiv(steps, 8), max(1, 2048 // npass)))
    red_px = _cdiv(steps, red_bound) * S
    return BnPlan(S, npass, steps, red_bound, red_px, _cdiv(P, red_px))


def bn_workspace_bytes(B, H, W, C):
    return align256(bn_plan(B, H, W, C).red_bound * 2 * C * 4) + align256(2 * C * 4)


BN_CAP_CASES = {
    batchnorm_ref.Case(2, 129, 128, 512): BnPlan(4, 2, 8256, 1024, 36, 918),      # two channel passes, 9 steps per slab
    batchnorm_ref.Case(1, 1025, 1024, 16): BnPlan(64, 1, 16400, 2048, 576, 1823),   # DLA level 0's width, 9 steps per slab
}
BN_LARGE_MEAN_CASE = batchnorm_ref.Case(2, 129, 128, 512)   # the many-way Chan merge over 918 slabs
BN_OLD_CASES = [batchnorm_ref.CASES[3], batchnorm_ref.CASES[5], batchnorm_ref.CASES[7], batchnorm_ref.CASES[10]]

# ---- depth-wise deconv backward (deconv_bwd.hip: dw_plan) ----
DwPlan = collections.namedtuple("DwPlan", "G PL rounds want rounds_per_slab slabs")


def dw_plan(B, H, W, C, f):
    k = 2 * f
    G = k * k // 16
    PL = (256 // G) // (C // 4)
    Q = B * H * W
    rounds = _cdiv(Q, PL)
    want = max(1, min(1024, _cdiv(rounds, 8)))
    rps = _cdiv(rounds, want)
    return DwPlan(G, PL, rounds, want, rps, _cdiv(Q, rps * PL))


def dw_workspace_bytes(B, H, W, C, f):
    return align256(dw_plan(B, H, W, C, f).want * 4 * f * f * C * 4)


DW_CAP_CASES = {
    deconv_backward_ref.dw(2, 257, 256, 16, 4): DwPlan(4, 16, 8224, 1024, 9, 914),   # the four-tap-group instance
    deconv_backward_ref.dw(2, 513, 512, 16, 2): DwPlan(1, 64, 8208, 1024, 9, 912),   # the single-group instance
}
DW_OLD_CASES = [deconv_backward_ref.DW_CASES[1], deconv_backward_ref.DW_CASES[5], deconv_backward_ref.DW_CASES[7],
                deconv_backward_ref.DW_CASES[13]]
