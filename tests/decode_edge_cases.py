"""Helper (not a test module): heat-maps that steer decode.hip's data-dependent control flow, and a Python restatement of
that control flow which says where a map lands.

Three parts.

* Constructors.  Every value is a small dyadic (or 0.5 + i ulp, a power of two, one denormal), every map float32, so a
  case lands where its name says: ``tie_map`` (a plateau over a flat pixel range whose first pixel is chosen, plus a few
  higher isolated pixels), ``staircase`` (row ranges at three levels), ``halo_map`` (a row that only the row above it,
  across a band seam, suppresses), ``near_flat`` (a constant -0.25 with isolated lowered pixels -- each becomes a
  suppressed zero -- and isolated raised ones, each kept, each suppressing its neighbours), ``ladder`` (top values one
  ulp apart: the low radix byte decides), ``exponent_ladder`` (powers of two and one positive denormal: the high byte
  decides).  ``recipes(H, W, K)`` builds every one that fits a shape.
* The restatement: ``nms_keys`` forms the keys as peaks_kernel does (v * keep, + 0.0f, ordered bits), ``select`` names the
  class (positive / zero / general), prefix, need, total_eq and all_eq of one selection, ``one_workgroup`` adds
  peaks_kernel's instantiation and the 4096-pixel groups of the first and last taken tie, ``tiled`` runs the same
  selection per band (with min(K, rows*W)) and over the bands' candidates (groups of 2048) and names the merge
  instantiation.  It restates the control flow, not the parallel mechanics: no histogram, no scan.
* The reference of the peaks half, ``reference_peaks``: np.lexsort on (pixel index, -value) over oracle.decode.nms.  It
  shares no code with the restatement above.  A suppressed negative is -0.0 there and +0.0 from the kernels, which add
  +0.0f so that equal values tie; comparisons are by value (np.testing.assert_array_equal treats the two zeros as equal).

``python -m tests.decode_edge_cases`` prints the table of cases against the branches reached.
"""
from collections import OrderedDict

import numpy as np

from oracle import decode as odec

F32 = np.float32
ZKEY = 0x80000000          # f2ord(+0.0f)
PK_GROUP = 4096            # pixels of one register group of peaks_kernel / peaks_tile_kernel (1024 lanes x float4)
MERGE_GROUP = 2048         # candidates of one register group of peaks_merge_kernel (1024 lanes x 2)
TL_PIX = 8192              # pixels of a band
ONE_WG_MAX = 32768         # cp_decode / the one-workgroup route of cp_decode_peaks
N_SINGLES = 10

# ---------------------------------------------------------------------------------------------------------------------
# restatement of the control flow


def f2ord(a):
    b = np.ascontiguousarray(a, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def nms_keys(m):
    """Keys of one H x W map as peaks_kernel forms them: kept = (max3x3 == v) ? v : v * 0.0f; key = ordered bits of
    kept + 0.0f; key 0 (unreachable for finite input) would become 1."""
    m = np.ascontiguousarray(m, F32)
    H, W = m.shape
    pad = np.full((H + 2, W + 2), -np.inf, F32)
    pad[1:-1, 1:-1] = m
    hmax = m.copy()
    for dy in range(3):
        for dx in range(3):
            np.maximum(hmax, pad[dy:dy + H, dx:dx + W], out=hmax)
    kept = np.where(hmax == m, m, m * F32(0.0)) + F32(0.0)
    k = f2ord(kept)
    k[k == 0] = 1
    return k


def select(keys, K):
    """One selection (peaks_kernel's, or select_top's) over keys in linear position order; key 0 = empty slot."""
    keys = np.ascontiguousarray(keys, np.uint32).ravel()
    tot_pos = int((keys > ZKEY).sum())
    tot_zero = int((keys == ZKEY).sum())
    if tot_pos < K and tot_pos + tot_zero >= K:
        cls, prefix, need = "zero", ZKEY, K - tot_pos
    else:
        cls = "positive" if tot_pos >= K else "general"
        prefix = int(np.partition(keys, keys.size - K)[keys.size - K])   # the K-th largest
        assert prefix != 0, "fewer than K real keys"
        need = K - int((keys > prefix).sum())
    eq = np.flatnonzero(keys == prefix)
    taken = eq[:need]
    pos = np.concatenate([np.flatnonzero(keys > prefix), taken])
    winners = pos[np.lexsort((pos, -keys[pos].astype(np.int64)))]
    return dict(cls=cls, tot_pos=tot_pos, tot_zero=tot_zero, prefix=prefix, need=need, total_eq=int(eq.size),
                all_eq=bool(eq.size <= need), first_eq=int(eq[0]), first_taken=int(taken[0]), last_taken=int(taken[-1]),
                winners=winners, win_keys=keys[winners])


def one_workgroup(m, K):
    """peaks_kernel on one map: the selection, the instantiation and the groups of the first and last taken tie."""
    H, W = m.shape
    assert K <= H * W <= ONE_WG_MAX and W % 4 == 0
    s = select(nms_keys(m), K)
    s["PK_G"] = 4 if H * W <= 16384 else 8
    s["g_first"], s["g_last"] = s["first_taken"] // PK_GROUP, s["last_taken"] // PK_GROUP
    s["ind"] = s["winners"]
    return s


def tiled_geom(H, W, K):
    R = TL_PIX // W
    T = -(-H // R)
    return R, T, (T * K + 1) & ~1


def merge_instantiation(NS):
    for g in (1, 2, 4, 8):
        if NS <= MERGE_GROUP * g:
            return g
    return 16


def tiled(m, K):
    """peaks_tile_kernel per band and peaks_merge_kernel over the bands' candidates."""
    H, W = m.shape
    assert K <= H * W <= 1 << 20 and W % 4 == 0 and W <= 4096
    R, T, NS = tiled_geom(H, W, K)
    keys = nms_keys(m).ravel()   # a band's keys with its two halo rows are the whole map's keys of those rows
    ckey, cpix, bands = np.zeros(NS, np.uint32), np.full(NS, -1, np.int64), []
    for t in range(T):
        p0, p1 = t * R * W, min(H, (t + 1) * R) * W
        s = select(keys[p0:p1], min(K, p1 - p0))
        s["K_band"] = min(K, p1 - p0)
        n = s["winners"].size
        ckey[t * K:t * K + n] = s["win_keys"]
        cpix[t * K:t * K + n] = p0 + s["winners"]
        bands.append(s)
    mg = select(ckey, K)
    w = mg["winners"]
    return dict(R=R, T=T, NS=NS, G=merge_instantiation(NS), bands=bands, merge=mg, ind=cpix[w], cand_pix=cpix,
                first_eq_pix=int(cpix[mg["first_eq"]]), g_first=mg["first_taken"] // MERGE_GROUP,
                g_last=mg["last_taken"] // MERGE_GROUP, g_first_eq=mg["first_eq"] // MERGE_GROUP,
                group0_above=int(((w < MERGE_GROUP) & (mg["win_keys"] > mg["prefix"])).sum()))


def reference_peaks(m, K):
    """(scores, indices) of the K largest of nms(map), (value desc, pixel index asc)."""
    v = odec.nms(np.ascontiguousarray(m, F32)[None, None])[0, 0].ravel()
    order = np.lexsort((np.arange(v.size), -v))[:K]
    return v[order], order.astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# constructors


def _singles(flat, s0, n=N_SINGLES):
    """n isolated pixels above every plateau, pairwise different: 0.75 + i / 256 at s0 + 1 + 8 i."""
    for i in range(n):
        flat[s0 + 1 + 8 * i] = F32(0.75) + F32(i) / F32(256)


def tie_map(H, W, p0, length, before=True):
    """A plateau of 0.5 over the flat pixels [p0, p0 + length) of a zero map and N_SINGLES higher isolated pixels, in the
    first rows (``before``) or behind the plateau.  None where they do not fit three rows apart."""
    HW = H * W
    p1 = min(p0 + length, HW)
    span = 8 * N_SINGLES + 2
    if p0 < 0 or p1 - p0 < 8:
        return None
    s_before, s_after = 0, ((p1 - 1) // W + 3) * W
    ok_before = (span - 1) // W + 3 <= p0 // W
    ok_after = s_after + span <= HW
    if not (ok_before if before else ok_after):
        before = not before
        if not (ok_before if before else ok_after):
            return None
    m = np.zeros((H, W), F32)
    m.reshape(-1)[p0:p1] = 0.5
    _singles(m.reshape(-1), s_before if before else s_after)
    return m


def staircase(H, W):
    """Rows 1-2 at 0.25, 3-4 at 0.5, 5 at 0.75, 6-7 at 0.5: NMS keeps rows 1, 3, 5 and 7 whole and suppresses the row of
    every step that touches a higher one."""
    if H < 8:
        return None
    m = np.zeros((H, W), F32)
    m[1:3], m[3:5], m[5:6], m[6:8] = 0.25, 0.5, 0.75, 0.5
    return m


def halo_map(H, W, r0):
    """Row r0 - 1 at 0.75 and row r0 at 0.5: with r0 the first row of a band, only the band's halo row suppresses it.
    A plateau of 0.25 from pixel 2 W + 2 gives narrow maps a tie."""
    if r0 < 6 or r0 >= H:
        return None
    m = np.zeros((H, W), F32)
    end = min(2 * W + 2 + 256, (r0 - 3) * W)
    m.reshape(-1)[2 * W + 2:end] = 0.25
    m[r0 - 1], m[r0] = 0.75, 0.5
    return m


def near_flat(H, W, zeros, p, q, strict=True):
    """A constant -0.25 with p isolated raised negatives (-1/8, -1/16, ...; each kept, its neighbours suppressed to zero),
    q isolated positives (0.5, 0.25) and as many isolated lowered pixels (-0.5, each a suppressed zero) as bring the
    number of zero keys to ``zeros``.  None (strict) where the shape has no room for that."""
    m = np.full((H, W), -0.25, F32)
    sites = [(y, x) for y in range(H - 2, 0, -3) for x in range(1, W - 1, 3)][:p + q]
    if len(sites) < p + q:
        return None
    for i, (y, x) in enumerate(sites):
        m[y, x] = -F32(2.0) ** -(3 + i) if i < p else F32(2.0) ** -(1 + i - p)
    ymax = min(y for y, _ in sites) - 2
    z0 = int((nms_keys(m) == ZKEY).sum())
    n, half = zeros - z0, (W + 1) // 2
    room = max(0, (ymax + 1) // 2) * half
    if n < 0 or n > room:
        if strict:
            return None
        n = min(max(n, 0), room)
    for i in range(n):
        m[2 * (i // half), 2 * (i % half)] = -0.5
    assert not strict or int((nms_keys(m) == ZKEY).sum()) == zeros
    return m


def _lattice(H, W, n):
    """n isolated pixels (even rows, even columns), spread over the map, as flat indices; None if there are fewer."""
    half, rows = (W + 1) // 2, (H + 1) // 2
    if rows * half < n:
        return None
    s = np.arange(n, dtype=np.int64) * ((rows * half) // n)
    return 2 * (s // half) * W + 2 * (s % half)


def ladder(H, W, n):
    """n isolated pixels at 0.5 + i ulp, i = 0 .. n-1 in scrambled pixel order, on a zero map."""
    at = _lattice(H, W, n)
    if at is None:
        return None
    m = np.zeros(H * W, F32)
    i = (np.arange(n) * 37) % n
    m[at] = (np.full(n, 0.5, F32).view(np.uint32) + i.astype(np.uint32)).view(F32)
    return m.reshape(H, W)


def exponent_ladder(H, W):
    """64 isolated pixels at 2^-i and one at the smallest positive denormal, on a zero map."""
    at = _lattice(H, W, 65)
    if at is None:
        return None
    m = np.zeros(H * W, F32)
    i = (np.arange(65) * 37) % 65
    v = np.ldexp(F32(1.0), -i).astype(F32)
    v[i == 64] = np.uint32(1).view(F32)
    m[at] = v
    return m.reshape(H, W)


def single_peak(H, W):
    m = np.zeros(H * W, F32)
    m[H * W // 2 + 1] = 0.5
    return m.reshape(H, W)


def recipes(H, W, K=128):
    """Every constructor that fits an H x W map, built for top-K, by name."""
    HW, L = H * W, 2 * K + 40
    R, T, _ = tiled_geom(H, W, K)
    r = OrderedDict()
    r["tie_e1_x4096"] = tie_map(H, W, 4096 - 39, L, before=False) if HW >= 4096 + L else None
    r["tie_e2_x16384"] = tie_map(H, W, 16384 - 38, L, before=False) if HW >= 16384 + L else None
    if T >= 2:
        t = min(15, T - 2)
        r["tie_e3_band_last_row"] = tie_map(H, W, (t + 1) * R * W - 37, L)
        r["tie_band_start"] = tie_map(H, W, min(16, T - 1) * R * W, L)
        r["halo_row"] = halo_map(H, W, min(16, T - 1) * R)
    if T >= 22:
        r["tie_merge_group1"] = tie_map(H, W, 20 * R * W + 2, L)
    r["staircase"] = staircase(H, W)
    r["flat_neg_tie"] = near_flat(H, W, K // 2, 3, 2, strict=False)
    r["flat_neg_Km1"] = near_flat(H, W, K - 1, 3, 0)
    r["flat_neg_K"] = near_flat(H, W, K, 3, 0)
    r["ladder_Km1"] = ladder(H, W, K - 1)
    r["ladder_K"] = ladder(H, W, K)
    r["ladder_Kp1"] = ladder(H, W, K + 1)
    r["single_peak"] = single_peak(H, W)
    r["exponent_ladder"] = exponent_ladder(H, W)
    return OrderedDict((k, v) for k, v in r.items() if v is not None)


KINDS = {  # the three kinds of the whole-decode tests
    "plateau": ("tie_e1_x4096", "tie_e3_band_last_row", "tie_band_start", "halo_row", "staircase", "single_peak"),
    "flat_neg": ("flat_neg_tie", "flat_neg_Km1", "flat_neg_K"),
    "ladder": ("ladder_Km1", "ladder_K", "ladder_Kp1", "exponent_ladder"),
}


def nine_maps(H, W, names, K=128):
    """hm [1,1,H,W] and hm_hp [1,8,H,W] from the recipes ``names`` that fit the shape, repeated in turn."""
    r = recipes(H, W, K)
    have = [n for n in names if n in r]
    assert have, (H, W, names)
    maps = np.stack([r[have[i % len(have)]] for i in range(9)])
    return maps[None, 0:1].copy(), maps[None, 1:9].copy(), [have[i % len(have)] for i in range(9)]


# ---------------------------------------------------------------------------------------------------------------------
# the named cases: what each promises, asserted by test_decode_edges_cpu.py through the restatement above

ONE_WG_SHAPES = ((8, 16), (32, 4), (64, 128), (132, 128))
SEAM_SHAPES = ((66, 128), (2049, 4))                       # tiled, reached through decode_raw_tiled
MERGE_SHAPES = {1: (66, 128), 2: (34, 4096), 4: (66, 4096), 8: (130, 4096), 16: (260, 2732)}
TILED_PEAK_SHAPES = ((264, 128), (34, 4096), (66, 4096), (130, 4096), (256, 4096), (260, 2732), (1024, 1024))
K_CASE = 128


def _halo_alone(s):
    """The first row of band ``t`` is all zero keys on the map, and all kept when the band is cut out without its halo."""
    m, R = s["map"], s["R"]
    r0 = min(16, s["T"] - 1) * R
    return r0 > 0 and (nms_keys(m)[r0] == ZKEY).all() and (nms_keys(m[r0:r0 + R])[0] > ZKEY).all()


K_ = K_CASE
COVERAGE = [  # (feature, recipe, shape, route, predicate over the restatement of that route)
    ("positive class, all_eq", "ladder_Kp1", (64, 128), "wg", lambda s: s["cls"] == "positive" and s["all_eq"]),
    ("positive class, partial tie", "tie_e1_x4096", (64, 128), "wg",
     lambda s: s["cls"] == "positive" and s["need"] < s["total_eq"]),
    ("zero class, need 1; tot_pos K-1", "ladder_Km1", (64, 128), "wg",
     lambda s: s["cls"] == "zero" and s["need"] == 1 and s["tot_pos"] == K_ - 1),
    ("zero class, need K-1; H*W == K", "single_peak", (32, 4), "wg",
     lambda s: s["cls"] == "zero" and s["need"] == K_ - 1 and s["map"].size == K_),
    ("zero class, need K; tot_pos + tot_zero K", "flat_neg_K", (64, 128), "wg",
     lambda s: s["cls"] == "zero" and s["need"] == K_ and s["tot_pos"] + s["tot_zero"] == K_),
    ("general class, mixed values, partial tie", "flat_neg_tie", (64, 128), "wg",
     lambda s: s["cls"] == "general" and s["tot_pos"] > 0 and s["tot_zero"] > 0 and s["need"] < s["total_eq"]
     and (s["win_keys"] < ZKEY).sum() > s["need"]),
    ("general class, H*W == K", "flat_neg_tie", (8, 16), "wg",
     lambda s: s["cls"] == "general" and s["map"].size == K_ and s["tot_pos"] > 0 and s["tot_zero"] > 0),
    ("tot_pos K", "ladder_K", (64, 128), "wg", lambda s: s["cls"] == "positive" and s["tot_pos"] == K_),
    ("tot_pos K+1", "ladder_Kp1", (64, 128), "wg", lambda s: s["tot_pos"] == K_ + 1),
    ("tot_pos + tot_zero K-1", "flat_neg_Km1", (64, 128), "wg",
     lambda s: s["cls"] == "general" and s["tot_pos"] + s["tot_zero"] == K_ - 1),
    ("tie from element 1 of a float4; crosses pixel 4096 in peaks_kernel<4>", "tie_e1_x4096", (64, 128), "wg",
     lambda s: s["first_eq"] % 4 == 1 and not s["all_eq"] and s["PK_G"] == 4 and (s["g_first"], s["g_last"]) == (0, 1)),
    ("tie from element 2; crosses pixel 16384 in peaks_kernel<8>", "tie_e2_x16384", (132, 128), "wg",
     lambda s: s["first_eq"] % 4 == 2 and not s["all_eq"] and s["PK_G"] == 8 and (s["g_first"], s["g_last"]) == (3, 4)),
    ("tie from element 3", "tie_e3_band_last_row", (66, 128), "wg", lambda s: s["first_eq"] % 4 == 3 and not s["all_eq"]),
    ("tie crosses pixel 4096 of a band", "tie_e1_x4096", (66, 128), "tiled",
     lambda s: (lambda b: not b["all_eq"] and (b["first_taken"] // PK_GROUP, b["last_taken"] // PK_GROUP) == (0, 1))(
         s["bands"][0])),
    ("tie starts at the first pixel of band 1", "tie_band_start", (66, 128), "tiled",
     lambda s: s["first_eq_pix"] == s["R"] * 128 and not s["merge"]["all_eq"] and not s["bands"][1]["all_eq"]),
    ("tie starts in the last row of band 0 and crosses the seam", "tie_e3_band_last_row", (66, 128), "tiled",
     lambda s: s["first_eq_pix"] // 128 == s["R"] - 1 and not s["merge"]["all_eq"]
     and s["cand_pix"][s["merge"]["last_taken"]] >= s["R"] * 128),
    ("halo row alone suppresses a band's first row", "halo_row", (66, 128), "tiled", _halo_alone),
    ("tie in merge group >= 1 while group 0's positives win", "tie_merge_group1", (66, 4096), "tiled",
     lambda s: s["g_first_eq"] >= 1 and not s["merge"]["all_eq"] and s["group0_above"] == N_SINGLES),
    ("taken ties cross merge groups 0 -> 1", "tie_e3_band_last_row", (66, 4096), "tiled",
     lambda s: (s["g_first"], s["g_last"]) == (0, 1) and not s["merge"]["all_eq"]),
    ("last band with rows*W < K", "tie_e3_band_last_row", (2049, 4), "tiled",
     lambda s: s["T"] == 2 and s["bands"][-1]["K_band"] == 4 < K_),
] + [("merge <%d>" % g, "staircase", MERGE_SHAPES[g], "tiled", (lambda g: lambda s: s["G"] == g)(g))
     for g in (1, 2, 4, 8, 16)]


def reach(recipe, shape, route):
    """The restatement of one named case on one route, with the map itself under "map"."""
    m = recipes(*shape, K_CASE)[recipe]
    s = (one_workgroup if route == "wg" else tiled)(m, K_CASE)
    s["map"] = m
    return s


def all_shapes():
    return ONE_WG_SHAPES + SEAM_SHAPES + TILED_PEAK_SHAPES


def reach_table():
    """Markdown rows, one per named case: where the restatement says the deciding selection lands."""
    rows = ["| reached | case | shape | route | class | need / total_eq | taken ties in groups |",
            "|---|---|---|---|---|---|---|"]
    for feature, recipe, (H, W), route, _ in COVERAGE:
        s = reach(recipe, (H, W), route)
        if route == "wg":
            where, g = "peaks_kernel<%d>" % s["PK_G"], s
        else:
            part = sum(1 for b in s["bands"] if not b["all_eq"])
            where, g = "%d bands (%d with a partial tie), merge<%d>" % (s["T"], part, s["G"]), s["merge"]
        rows.append("| %s | `%s` | %d x %d | %s | %s | %d / %d | %d..%d |" % (
            feature, recipe, H, W, where, g["cls"], g["need"], g["total_eq"], s["g_first"], s["g_last"]))
    return "\n".join(rows)


# ---------------------------------------------------------------------------------------------------------------------
# assoc_kernel's float comparisons on their boundaries: one 16 x 16 frame built by hand, K = 16.
#
# The 16 centre peaks sit at (2 + 4a, 2 + 4b); record k is the k-th row of _DETS (scores fall with k).  reg = (0.5, 0.5)
# everywhere, so a box is (cx + 0.5 -+ w/2, cy + 0.5 -+ h/2).  A scenario is (record, joint): a joint peak at a pixel (plus
# hp_offset, which is one map for all joints) and the keypoint the record regresses for that joint.  Every product the
# kernel compares against is an exact float32: 0.8f * 5 = 4, 1.2f * 10 = 12, 0.3f * 5 = 1.5, 0.5f * 5 = 2.5.
# Of the seven conditions of the inference filter, six are put on their boundary alone.  The seventh, hs > 0.1, cannot be:
# a joint peak scoring exactly 0.1 is masked first (hs = -1, hx = hy = -10000), which fails the box conditions with it; the
# first scenario holds that boundary at the mask.

ASSOC_K = 16
T01 = F32(0.1)
T01_UP = np.nextafter(T01, F32(1))
_DETS = [  # (cx, cy), (w, h), score
    ((6, 2), (16, 4)), ((6, 6), (5, 5)), ((2, 10), (10, 5)), ((14, 10), (10, 5)), ((10, 6), (5, 5)), ((10, 14), (5, 5)),
    ((10, 10), (11, 11)), ((2, 2), (15, 15)), ((14, 2), (5, 5)), ((10, 2), (5, 5)), ((14, 6), (5, 5)), ((2, 6), (5, 5)),
    ((6, 10), (5, 5)), ((6, 14), (5, 5)), ((14, 14), (5, 5)), ((2, 14), (5, 5))]
_PEAKS = {  # joint -> [(x, y, score)]
    0: [(5, 2, T01_UP), (9, 2, T01), (8, 6, 0.5), (13, 13, 0.25)],
    1: [(8, 10, 0.75), (12, 10, 0.5), (0, 10, 0.625), (15, 10, 0.03125)],
    2: [(3, 3, 0.0625), (11, 11, T01)],
    3: [(4, 6, 0.5), (4, 10, 0.75)],
    4: [(9, 6, 0.5), (10, 4, 0.75)],
    5: [(6, 4, 0.5), (12, 2, 0.75)],
    6: [(6, 9, 0.5), (2, 12, 0.75)],
    7: [(7, 6, 0.5), (3, 14, 0.75), (13, 14, 0.625)],
}
_OFFSETS = {(7, 6): (0.5, 0), (8, 6): (0.5, 0), (0, 10): (-1.5, 0), (15, 10): (1.5, 0)}
NEG = -10000.0
# (what, record, joint, regressed keypoint, kps the record must carry, its heat-map keypoint or None for -10000, height)
_SCENARIOS = [
    ("joint score 0.1 is masked, one ulp above is not", 0, 0, (9, 2), (5, 2), (5, 2), T01_UP),
    ("equal distance: the lower candidate index wins", 6, 1, (10, 10), (8, 10), (8, 10), 0.75),
    ("hx == l: kept", 1, 3, (5, 6), (4, 6), (4, 6), 0.5),
    ("hx == r: kept", 1, 4, (8, 6), (9, 6), (9, 6), 0.5),
    ("hy == t: kept", 1, 5, (6, 5), (6, 4), (6, 4), 0.5),
    ("hy == bt: kept", 1, 6, (6, 8), (6, 9), (6, 9), 0.5),
    ("best == 0.3 size: kept", 1, 7, (6, 6), (7.5, 6), (7.5, 6), 0.5),
    ("hx == 0.8 l: filtered", 6, 3, (6, 10), (6, 10), None, NEG),
    ("hy == 0.8 t: filtered", 6, 4, (10, 3), (10, 3), None, NEG),
    ("hx == 1.2 r: filtered", 7, 5, (10, 2), (10, 2), None, NEG),
    ("hy == 1.2 bt: filtered", 7, 6, (2, 10), (2, 10), None, NEG),
    ("best == 0.5 size: filtered", 1, 0, (6, 6), (6, 6), None, NEG),
    ("centre score 0.1: filtered", 15, 7, (3, 14), (3, 14), None, NEG),
    ("centre score one ulp above 0.1: passes", 14, 7, (13, 14), (13, 14), (13, 14), 0.625),
    ("hx < 0: the height is read from the last column", 2, 1, (0, 10), (-1.5, 10), (-1.5, 10), 0.03125),
]
BEYOND = (3, 3, (15, 10), (16.5, 10))   # record, joint, pixel of the extra joint peak, its keypoint right of the map
BEYOND_XY = BEYOND[3]


def assoc_case():
    H = W = 16
    d = {"hm": np.zeros((1, 1, H, W), F32), "hm_hp": np.zeros((1, 8, H, W), F32), "hps": np.zeros((1, 16, H, W), F32),
         "wh": np.full((1, 2, H, W), 5, F32), "reg": np.full((1, 2, H, W), 0.5, F32),
         "hp_offset": np.zeros((1, 2, H, W), F32), "scale": np.full((1, 3, H, W), 0.75, F32)}
    for k, ((cx, cy), (w, h)) in enumerate(_DETS):
        d["hm"][0, 0, cy, cx] = T01_UP if k == 14 else T01 if k == 15 else F32(0.9375) - F32(k) / 32
        d["wh"][0, :, cy, cx] = (w, h)
        d["scale"][0, :, cy, cx] = (0.5 + k / 16, 1, 2)
    for j, peaks in _PEAKS.items():
        for x, y, s in peaks:
            d["hm_hp"][0, j, y, x] = s
    for (x, y), off in _OFFSETS.items():
        d["hp_offset"][0, :, y, x] = off
    for _, k, j, (kx, ky), _, _, _ in _SCENARIOS:
        (cx, cy), _ = _DETS[k]
        d["hps"][0, 2 * j:2 * j + 2, cy, cx] = (kx - cx, ky - cy)
    return d


def assoc_check(d, o):
    """The oracle's records (rep_mode 1, uint8 masks) land where the scenarios say, and the boundaries are exact."""
    f = F32
    assert f(0.8) * f(5) == 4 and f(1.2) * f(10) == 12 and f(5) * f(0.3) == 1.5 and f(5) * f(0.5) == 2.5
    assert T01_UP > T01 and T01_UP.view(np.uint32) - T01.view(np.uint32) == 1
    box = o["bboxes"][0]
    np.testing.assert_array_equal(box[1], [4, 4, 9, 9])
    np.testing.assert_array_equal(box[6], [5, 5, 16, 16])
    np.testing.assert_array_equal(box[7], [-5, -5, 10, 10])
    np.testing.assert_array_equal(o["scores"][0, 14:, 0], [T01_UP, T01])
    for what, k, j, kp, kps, hm_kp, height in _SCENARIOS:
        np.testing.assert_array_equal(o["kps_displacement_mean"][0, k, 2 * j:2 * j + 2], kp, err_msg=what)
        np.testing.assert_array_equal(o["kps"][0, k, 2 * j:2 * j + 2], kps, err_msg=what)
        np.testing.assert_array_equal(o["kps_heatmap_mean"][0, k, 2 * j:2 * j + 2], hm_kp or (NEG, NEG), err_msg=what)
        assert o["kps_heatmap_height"][0, k, j] == f(height), what
    # joint 2: no candidate passes 0.1 -- all sit at (-10000, -10000), candidate 0 is taken and rejected
    np.testing.assert_array_equal(o["kps"][0, :, 4:6], o["kps_displacement_mean"][0, :, 4:6])
    assert np.all(o["kps_heatmap_height"][0, :, 2] == NEG)


def assoc_beyond_right_edge():
    """(heads with a joint peak whose keypoint lies right of the map, the same heads without it, (record, joint))."""
    k, j, (x, y), _ = BEYOND
    d = assoc_case()
    (cx, cy), _ = _DETS[k]
    d["hps"][0, 2 * j:2 * j + 2, cy, cx] = (x - cx, y - cy)
    without = {n: v.copy() for n, v in d.items()}
    d["hm_hp"][0, j, y, x] = 0.5
    return d, without, (k, j)


if __name__ == "__main__":
    print(reach_table())
