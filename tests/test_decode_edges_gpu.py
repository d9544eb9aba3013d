"""GPU tests of the heat-map decode where its control flow turns on the data and on the grid: ties at the K-th rank (from
every element of a lane's float4, across peaks_kernel's 4096-pixel groups, across band seams and merge groups), the three
key classes and their boundaries, every instantiation of peaks_merge_kernel, both corners of the tiled envelope
(256 x 4096 and 1024 x 1024), rep_mode 2 / 3 / 4, and the float comparisons of assoc_kernel on their boundaries.

The maps come from tests/decode_edge_cases.py; test_decode_edges_cpu.py asserts that each lands on the branch it is named
for.  The references are np.lexsort over the oracle's NMS (peaks half) and oracle.decode.object_pose_decode (records);
neither shares code with the kernels.  Comparisons are exact, by value: a suppressed negative is -0.0 in the references
and +0.0 from the kernels, which np.testing.assert_array_equal takes as equal."""
import functools

import numpy as np
import pytest
import torch

from centerpose_amd import hip
from oracle import decode as odec
from tests import decode_edge_cases as E

pytestmark = pytest.mark.gpu

K = E.K_CASE
_OPT = ("hps_uncertainty", "scale", "scale_uncertainty", "reg", "hp_offset", "tracking", "tracking_hp")
# at 2^19 pixels and above one image of nine maps (36 MB at 2^20, nine host sorts): the cases that need a band or a merge
_BIG = ("tie_e1_x4096", "tie_e3_band_last_row", "tie_band_start", "halo_row", "tie_merge_group1", "flat_neg_tie",
        "flat_neg_Km1", "ladder_Kp1", "exponent_ladder")


@functools.lru_cache(maxsize=None)
def _stack(H, W):
    """Every recipe of the shape as [B, 9, H, W] (B = 2 holds different maps per image), and the reference top K."""
    r = E.recipes(H, W, K)
    names = [n for n in r if H * W < 1 << 19 or n in _BIG]
    B = -(-len(names) // 9)
    names = [names[i % len(names)] for i in range(9 * B)]
    maps = np.stack([r[n] for n in names]).reshape(B, 9, H, W)
    ref = [E.reference_peaks(m, min(K, H * W)) for m in maps.reshape(-1, H, W)]
    return names, maps, np.stack([v for v, _ in ref]).reshape(B, 9, -1), np.stack([i for _, i in ref]).reshape(B, 9, -1)


def _peaks(maps, device, k, apply_sigmoid=False):
    t = torch.from_numpy(maps).to(device)
    hm, hm_hp = t[:, 0:1].contiguous(), t[:, 1:9].contiguous()
    s, i = hip.decode_peaks(hm, hm_hp, K=k, apply_sigmoid=apply_sigmoid)
    return s.cpu().numpy(), i.cpu().numpy(), torch.cat([hm, hm_hp], 1).cpu().numpy()


@pytest.mark.parametrize("H,W", E.ONE_WG_SHAPES + E.TILED_PEAK_SHAPES, ids=lambda v: str(v))
def test_peaks_against_the_lexsort_reference(device, H, W):
    """The top K of a prefix of the total order (value desc, index asc) is that prefix: one reference serves every K."""
    names, maps, ref_v, ref_i = _stack(H, W)
    for k in (1, 100, K):
        if k > H * W:
            continue
        s, i, _ = _peaks(maps, device, k)
        for b in range(maps.shape[0]):
            for c in range(9):
                tag = "%s %dx%d K=%d" % (names[9 * b + c], H, W, k)
                np.testing.assert_array_equal(i[b, c], ref_i[b, c, :k], err_msg=tag)
                np.testing.assert_array_equal(s[b, c], ref_v[b, c, :k], err_msg=tag)


def test_peaks_fused_sigmoid_with_ties_at_66x4096(device):
    """Dyadic logits repeated on plateaus: equal inputs give equal sigmoids, so the ties survive expf.  The reference is
    the lexsort of the maps the kernels wrote back."""
    H, W = 66, 4096
    names, maps, _, _ = _stack(H, W)
    logits = (maps[:1] * 4 - 2).astype(np.float32)
    s, i, wrote = _peaks(logits, device, K, apply_sigmoid=True)
    assert np.abs(wrote - 1 / (1 + np.exp(-logits.astype(np.float64)))).max() < 1e-6
    for c in range(9):
        v, ind = E.reference_peaks(wrote[0, c], K)
        if names[c].startswith("tie_"):   # still a partial tie at the K-th rank
            assert np.sum(wrote[0, c] == v[-1]) > np.sum(v == v[-1]) > 1, names[c]
        np.testing.assert_array_equal(i[0, c], ind, err_msg=names[c])
        np.testing.assert_array_equal(s[0, c], v, err_msg=names[c])


# ---------------------------------------------------------------------------------------------------------------------
# whole decode against the oracle


def _decode(fn, d, device, k, rep_mode, sem="uint8", fit=False):
    g = {n: torch.from_numpy(np.ascontiguousarray(v)).to(device) for n, v in d.items()}
    det = fn(g["hm"], g["hps"], g["wh"], g["hm_hp"], *[g.get(n) for n in _OPT], K=k, rep_mode=rep_mode, fit_gaussian=fit,
             balance=2.0, legacy_bool_mask=(sem == "bool"))
    return det.cpu().numpy()


def _oracle(d, k, rep_mode, sem="uint8"):
    return odec.object_pose_decode(d["hm"], d["hps"], wh=d["wh"], obj_scale=d.get("scale"), reg=d.get("reg"),
                                   hm_hp=d["hm_hp"], hp_offset=d.get("hp_offset"), K=k, rep_mode=rep_mode,
                                   mask_semantics=sem)


def _assert_records(det, o, fit=False, tag=""):
    r = {n: v.numpy() for n, v in hip.split_detections(torch.from_numpy(det)).items()}
    for n in o:
        if n in ("kps_displacement_std", "obj_scale_uncertainty"):
            np.testing.assert_allclose(r[n], o[n], rtol=3e-6, atol=0, err_msg=tag + n)
        elif fit and n.startswith("kps_heatmap"):
            np.testing.assert_allclose(r[n], o[n], rtol=1e-6, atol=1e-6, err_msg=tag + n)
        else:
            np.testing.assert_array_equal(r[n], o[n], err_msg=tag + n)


def _heads(H, W, kind, seed):
    d = odec.synth_heads(1, seed=seed, H=H, W=W)
    d["hm"], d["hm_hp"], names = E.nine_maps(H, W, E.KINDS[kind], K)
    return d, names


@pytest.mark.parametrize("kind", sorted(E.KINDS))
@pytest.mark.parametrize("H,W", [(64, 128), (66, 128), (2049, 4)], ids=lambda v: str(v))
def test_whole_decode_against_the_oracle(device, H, W, kind):
    """cp_decode and cp_decode_tiled, each against the oracle: an error the two share (they share assoc_kernel) shows."""
    d, names = _heads(H, W, kind, seed=H + W)
    for rep_mode, sem in ((1, "uint8"), (0, "bool"), (1, "bool")):
        o = _oracle(d, K, rep_mode, sem)
        for fn in (hip.decode_raw, hip.decode_raw_tiled):
            tag = "%s %s rep=%d %s " % (fn.__name__, "/".join(sorted(set(names))), rep_mode, sem)
            _assert_records(_decode(fn, d, device, K, rep_mode, sem), o, tag=tag)


def _inside(d, H, W):
    """Joint peaks 12 pixels inside the map: the oracle's Gaussian fit (scipy) refuses the NaN start of a window whose
    centre column lies in the zero padding, as the reference would."""
    edge = np.full((H, W), 1e-6, np.float32)
    edge[12:-12, 12:-12] = 1
    return dict(d, hm_hp=d["hm_hp"] * edge)


@pytest.mark.parametrize("rep_mode", [2, 3, 4])
@pytest.mark.parametrize("H,W,k", [(32, 32, 32), (64, 128, 100)])
def test_rep_modes_2_3_4_against_the_oracle(device, H, W, k, rep_mode):
    """3: the regressed keypoints; 4: the heat-map keypoints; 2: a Gaussian fit without the tracking heads
    (lib/models/decode.py sets fit_gaussian for it)."""
    d = odec.synth_heads(1, seed=7 * H + rep_mode, H=H, W=W)
    fit = rep_mode == 2
    if fit:
        d = _inside(d, H, W)
    o = _oracle(d, k, rep_mode)
    for fn in (hip.decode_raw, hip.decode_raw_tiled):
        _assert_records(_decode(fn, d, device, k, rep_mode, fit=fit), o, fit=fit, tag="%s rep=%d " % (fn.__name__, rep_mode))
    if rep_mode != 2:   # the mode decides which keypoints a record carries
        assert not np.array_equal(o["kps"], _oracle(d, k, 1)["kps"])


# ---------------------------------------------------------------------------------------------------------------------
# assoc_kernel's comparisons on their boundaries: one hand-built 16 x 16 case (decode_edge_cases.assoc_case)


@pytest.mark.parametrize("fn", ["decode_raw", "decode_raw_tiled"])
def test_association_boundaries_against_the_oracle(device, fn):
    d = E.assoc_case()
    for rep_mode, sem in ((1, "uint8"), (0, "uint8"), (1, "bool")):
        o = _oracle(d, E.ASSOC_K, rep_mode, sem)
        if (rep_mode, sem) == (1, "uint8"):
            E.assoc_check(d, o)
        det = _decode(getattr(hip, fn), d, device, E.ASSOC_K, rep_mode, sem)
        _assert_records(det, o, tag="%s rep=%d %s " % (fn, rep_mode, sem))


def test_heat_map_keypoint_right_of_the_map_keeps_minus_10000(device):
    """hx >= W: the reference raises IndexError there; the record keeps -10000 in its three heat-map fields and every
    other record equals the oracle's for the same inputs without that joint peak."""
    d, without, (k, j) = E.assoc_beyond_right_edge()
    with pytest.raises(IndexError):
        _oracle(d, E.ASSOC_K, 1)
    o = _oracle(without, E.ASSOC_K, 1)
    det = _decode(hip.decode_raw, d, device, E.ASSOC_K, 1)
    r = {n: v.numpy().copy() for n, v in hip.split_detections(torch.from_numpy(det)).items()}
    assert np.all(r["kps_heatmap_mean"][0, k, 2 * j:2 * j + 2] == -10000) and r["kps_heatmap_height"][0, k, j] == -10000
    assert np.all(r["kps_heatmap_std"][0, k, 2 * j:2 * j + 2] == -10000)
    assert np.all(r["kps"][0, k, 2 * j:2 * j + 2] == E.BEYOND_XY)   # the association itself took the peak
    for n, v in o.items():   # that joint of that record aside, nothing moved
        got, want = r[n], v.copy()
        if n.startswith("kps_heatmap") or n == "kps":
            w = 1 if n == "kps_heatmap_height" else 2
            got[0, k, w * j:w * j + w] = want[0, k, w * j:w * j + w] = 0
        np.testing.assert_array_equal(got, want, err_msg=n)
