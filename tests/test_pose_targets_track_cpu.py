"""CPU tests of the tracking task's training targets (no GPU): the host restatement tests/pose_targets_track_ref.py
against the reference-built goldens (and against the reference's live __getitem__ where that tree is present), the
events the golden cases must contain, the host build of pose_targets_track_common.h against the restatement object by
object, the C ABI's declarations, layouts and refusals with no device, and the Python layer's packing and refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from centerpose_amd import hip
from centerpose_amd.pose_targets import PoseTargets, num_symmetry
from centerpose_amd.pose_targets_track import (NUM_DRAWS, TrackPoseTargets, draw_track_noise, pack_track_annotations,
                                               track_target_keys)
from tests import pose_target_cases as PC
from tests import pose_target_track_cases as TC
from tests import pose_targets_track_ref as TR

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(REPO, "tests", "golden", "pose_targets_track_ref.npz")
MAPS = ("hm", "hm_hp", "pre_hm", "pre_hm_hp")
RECORDS = ("pt_image", "pt_objects", "ptk_image", "ptk_pre_objects", "ptk_cur_objects")
D = hip.PTK_DRAW


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def golden_records(gold, name):
    return {k: gold[name + "/" + k] for k in RECORDS}


def golden_arrays(gold, name, opt):
    """The golden case's ret as dense [1, ...] arrays."""
    S, Rr, H, W = num_symmetry(opt), opt.output_res, opt.input_h, opt.input_w
    shape = {"hm": (1, S, 1, Rr, Rr), "hm_hp": (1, S, 8, Rr, Rr), "pre_hm": (1, 1, H, W), "pre_hm_hp": (1, 8, H, W)}
    out = {}
    for k in track_target_keys(opt):
        if k in MAPS:
            m = np.zeros(shape[k], np.float32)
            m.reshape(-1)[gold["%s/%s_idx" % (name, k)]] = gold["%s/%s_val" % (name, k)]
            out[k] = m
        else:
            out[k] = gold["%s/%s" % (name, k)][None]
    return out


def restate(recs, opt):
    """Batched records -> the restatement's arrays ([B, ...]) and its per-object dicts."""
    return TR.batch_targets(recs, num_symmetry(opt), opt.output_res, TR.options(opt), opt.use_absolute_scale)


def restate_case(gold, name):
    opt = TC.make_opt(TC.CASES[name][1])
    return opt, restate({k: v[None] for k, v in golden_records(gold, name).items()}, opt)


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_restatement_equals_goldens(gold, name):
    opt, r = restate_case(gold, name)
    for k, v in golden_arrays(gold, name, opt).items():
        assert r[k].dtype == v.dtype and r[k].shape == v.shape, k
        assert np.array_equal(r[k].view(np.uint8), v.view(np.uint8)), k  # floats and maps bit for bit


def _covers(hm, x, y, r):
    """The draw's window meets the map."""
    H, W = hm.shape
    return max(0, x - r) < min(W, x + r + 1) and max(0, y - r) < min(H, y + r + 1)


def test_goldens_cover_the_events(gold):
    """Each event the cases were written for is in the golden file (read off the restatement, which the test above pins
    to the reference's arrays)."""
    res = {n: restate_case(gold, n) for n in TC.CASES}
    pre = {n: res[n][1]["pre"][0] for n in res}

    def opt(n):
        return res[n][0]

    # a symmetric chair whose chosen variant filters the current frame, and a lost centre that leaves all variants in
    g, p = gold, pre["chair_filter"]
    assert g["chair_filter/pt_objects"][:2, 0].tolist() == [4, 4] and p[0]["chosen"] is not None
    assert g["chair_filter/reg_mask"][:, 0].tolist() == [int(s == p[0]["chosen"]) for s in range(4)]
    lost = [q for q in p if q["kept"] and any(c == 0 and k == 0 for c, _, _, k in q["draws"])]
    assert p[1] in lost and p[1]["chosen"] is None and g["chair_filter/reg_mask"][:, 1].all()
    # the lost centre under tracking_label_mode 1 (None: no tracking target) and 0 (the noisy centre)
    assert opt("chair_filter").tracking_label_mode == 1 and p[1]["cts"] is None
    assert not g["chair_filter/tracking_mask"][:, 1].any() and g["chair_filter/tracking_mask"][p[0]["chosen"], 0] == 1
    p0 = pre["label0_plain"]
    assert opt("label0_plain").tracking_label_mode == 0 and any(k == 0 for _, _, _, k in p0[0]["draws"])
    assert p0[0]["cts"] is not None and g["label0_plain/tracking_mask"][0, 0] == 1
    # a noisy centre that leaves the input: absent from the lists, its current twin untracked
    pl = pre["leave_clip"]
    assert pl[0]["geom"] is not None and not pl[0]["kept"]
    assert g["leave_clip/reg_mask"][0, 0] == 1 and g["leave_clip/tracking_mask"][0, 0] == 0
    # a false-positive centre and a false-positive joint: two draws on one channel
    for n in ("chair_filter", "label0_plain", "center3d"):
        ch = [[c for c, _, _, _ in q["draws"]] for q in pre[n]]
        assert any(c.count(0) == 2 for c in ch), n
        assert any(c.count(j) == 2 for c in ch for j in range(1, 9)), n
    # a lost joint under both label modes: NaN (mode 1) and the noisy point with mask 1 (mode 0)
    assert np.isnan(pre["chair_filter"][2]["pts"][3]).all() and pre["chair_filter"][2]["pmask"][3] == 0
    assert any(c == 2 and k == 0 for c, _, _, k in p0[1]["draws"]) and p0[1]["pmask"][1] == 1
    assert g["chair_filter/tracking_hp_mask"][:, 2, 6:8].sum() == 0 and g["chair_filter/hps_mask"][:, 2, 6:8].any()
    # hm_heat_random / hm_hp_heat_random on and off: peaks below 1 against peaks of exactly 1
    assert opt("chair_filter").hm_heat_random and opt("chair_filter").hm_hp_heat_random
    assert not opt("label0_plain").hm_heat_random and not opt("label0_plain").hm_hp_heat_random
    assert all(0 < k < 1 for q in pre["chair_filter"][2:] for _, _, _, k in q["draws"] if k)
    assert any(k == 1 for q in p0 for c, _, _, k in q["draws"] if c == 0)
    assert any(k == 1 for q in p0 for c, _, _, k in q["draws"] if c > 0)
    # a joint whose noisy position falls outside the map: once with its window still overlapping, once without
    hm = np.zeros((opt("leave_clip").input_h, opt("leave_clip").input_w))
    out = [[(x, y) for c, x, y, k in q["draws"] if c > 0 and k and not (0 <= x < hm.shape[1] and 0 <= y < hm.shape[0])]
           for q in pl]
    assert any(_covers(hm, x, y, pl[1]["radius"]) for x, y in out[1])
    assert any(not _covers(hm, x, y, pl[2]["radius"]) for x, y in out[2])
    # a previous object out of frame with 4 against 5 visible corners
    pf = pre["out_flip_twice"]
    assert pf[2]["geom"] is None and not pf[2]["kept"] and pf[3]["kept"]
    # flip on
    assert g["out_flip_twice/pt_image"][8] == 1 and g["chair_filter/pt_image"][8] == 0
    # rot != 0 with a zero-area box
    assert g["rot_flat/pt_image"][9] != 0 and pre["rot_flat"][1]["kept"] and 0.0 in pre["rot_flat"][1]["geom"][:2]
    # center_3D
    assert opt("center3d").center_3D and any(q["kept"] for q in pre["center3d"])
    # two previous objects with the same id: the first wins
    ids = g["out_flip_twice/ptk_pre_objects"][:4, hip.PTK_PRE["id"]]
    assert ids[0] == ids[1] == g["out_flip_twice/ptk_cur_objects"][0, 0] and pf[0]["kept"] and pf[1]["kept"]
    ct = g["out_flip_twice/ind"][0, 0] % 64, g["out_flip_twice/ind"][0, 0] // 64
    want = np.float32([pf[0]["cts"][0] - ct[0], pf[0]["cts"][1] - ct[1]])
    assert np.array_equal(g["out_flip_twice/tracking"][0, 0], want) and pf[0]["cts"] != pf[1]["cts"]
    # cup: previous objects skipped by their 'mug', and a current frame skipped by the LAST previous object's
    assert g["cup_mug_pre/ptk_pre_objects"][:4, hip.PTK_PRE["skip"]].tolist() == [1, 0, 1, 0]
    assert g["cup_mug_pre/ptk_cur_objects"][:3, 1].tolist() == [0, 0, 0] and g["cup_mug_pre/reg_mask"].any()
    assert g["cup_mug_cur/ptk_cur_objects"][:2, 1].tolist() == [1, 1] and not g["cup_mug_cur/reg_mask"].any()
    assert pre["cup_mug_cur"][0]["kept"] and (g["cup_mug_cur/pre_hm_val"] > 0).any()
    # the variant count carried across the frames: the last previous object's 4 into the first current object
    assert g["cup_mug_pre/ptk_pre_objects"][:4, 0].tolist() == [6, 4, 1, 4] and g["cup_mug_pre/pt_objects"][0, 0] == 4
    # the second resolution
    assert g["big/pre_hm_hp_idx"].max() > 8 * 256 * 256 and opt("big").input_w == 384


def test_restatement_equals_live_reference():
    if not PC.reference_available():
        pytest.skip("the reference tree is not present")
    for seed in range(200, 214):
        res = (64, 96)[seed % 2]
        opt, anns, pre, w, h, sd, draws = TC.random_case(seed, output_res=res, input_res=4 * res, input_w=4 * res,
                                                         input_h=4 * res)
        recs, ret = TC.reference_case(opt, anns, pre, w, h, sd, draws)
        r = restate({k: v[None] for k, v in recs.items()}, opt)
        for k in track_target_keys(opt):
            assert r[k][0].dtype == ret[k].dtype and r[k][0].shape == ret[k].shape, (seed, k)
            assert np.array_equal(r[k][0].view(np.uint8), ret[k].view(np.uint8)), (seed, k)


def _host():
    out = os.path.join(REPO, "tests", "_build", "libcp_pose_targets_track_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(REPO, "tests", "native", "pose_targets_track_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
    L = ctypes.CDLL(out)
    L.ptk_host_pre_object.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return L


def random_records(rng, n_images, opt, max_pre_objs=None, n_objects=None, edits=()):
    """Packed records of synthetic pairs of frames with random affines (scale, shift, rotation, flip), stacked."""
    S, Rr = num_symmetry(opt), opt.output_res
    kinds = ["pose", "pose", "pose", "edge", "twin", "corner_neg", "out4", "out5", "negy", "flat"]
    syms = ["True", "False", None] if S >= 4 else [None]
    out = []
    while len(out) < n_images:
        w, h = (640, 480) if rng.random() < 0.5 else (480, 640)
        n = int(rng.integers(1, 11)) if n_objects is None else n_objects
        specs = [(syms[int(rng.integers(len(syms)))], kinds[int(rng.integers(len(kinds)))] if n_objects is None else "pose")
                 for _ in range(n)]
        anns = TC.name_objects(PC.synth_annotations(rng, specs, w, h))
        npre = n if max_pre_objs is None else max_pre_objs
        spec = [(k % n, None if rng.random() < 0.8 or n_objects else "obj_%d" % rng.integers(n), False) for k in range(npre)]
        pre = TC.previous_frame(rng, anns, spec)
        a = np.deg2rad(rng.uniform(-30, 30)) if rng.random() < 0.5 else 0.0
        c = np.array([w / 2 + rng.uniform(-80, 80), h / 2 + rng.uniform(-80, 80)])
        ts = []
        for size in ((Rr, Rr), (opt.input_w, opt.input_h)):
            s = max(w, h) * rng.uniform(0.7, 1.3) / max(size)
            M = np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]]) / s
            ts.append(np.hstack([M, (np.array(size) / 2 - M @ (c + rng.uniform(-10, 10, 2)))[:, None]]))
        draws = TC.apply_edits(draw_track_noise(rng, npre), edits)
        try:
            out.append(pack_track_annotations(anns, pre, ts[0], ts[1], w, h, rng.random() < 0.5, np.rad2deg(a), opt, draws,
                                              max_pre_objs=max_pre_objs))
        except ValueError:  # a symmetric current object past the previous frame's end: the packer refuses it
            continue
    return {k: np.stack([r[k] for r in out]) for k in out[0]}


def test_host_build_equals_restatement():
    L = _host()
    rng = np.random.default_rng(6)
    out = np.zeros(103, np.float64)
    n = 0
    for S, cat in ((4, "chair"), (12, "bottle"), (1, "camera"), (6, "cup")):
        for trial in range(6):
            opt = TC.make_opt(dict(c=cat, num_symmetry=S, center_3D=bool(trial & 1), tracking_label_mode=(trial >> 1) & 1,
                                   hm_heat_random=trial % 3 != 0, hm_hp_heat_random=trial % 3 != 1,
                                   hm_disturb=(0.05, 0.8)[trial % 2], hm_hp_disturb=(0.02, 0.6)[(trial // 2) % 2],
                                   input_w=(256, 320)[trial % 2], pre_hm=trial != 4, pre_hm_hp=trial != 5))
            op = TR.options(opt)
            ov = np.array([float(getattr(op, k)) for k in TR.OPT_NAMES])
            recs = random_records(rng, 10, opt)
            for b in range(10):
                im = np.ascontiguousarray(TR.pre_image(recs["pt_image"][b], recs["ptk_image"][b]))
                for k in range(int(recs["ptk_image"][b, hip.PTK_IMG["num_pre"]])):
                    ob = np.ascontiguousarray(recs["ptk_pre_objects"][b, k])
                    L.ptk_host_pre_object(im.ctypes.data, ob.ctypes.data, S, ov.ctypes.data, out.ctypes.data)
                    r = TR.pre_object(im, ob, S, op)
                    n += 1
                    where = (S, trial, b, k)
                    assert out[0] == r["kept"] and out[1] == r["id"], where
                    assert out[2] == (-1 if r["chosen"] is None else r["chosen"]), where
                    assert out[3] == (r["cts"] is None), where
                    if r["cts"] is not None:
                        assert tuple(out[4:6]) == r["cts"], where
                    assert np.array_equal(out[6:22].astype(np.float32).view(np.uint32), r["pts"].reshape(-1).view(np.uint32))
                    assert np.array_equal(out[22:30], r["pmask"]), where
                    draws = [tuple(out[31 + 4 * i + 1:31 + 4 * i + 4]) + (i // 2,) for i in range(18) if out[31 + 4 * i]]
                    want = [(float(x), float(y), float(kk), c) for c, x, y, kk in r["draws"]]
                    assert sorted(draws) == sorted(want), where  # the peaks bit for bit
                    if draws:
                        assert out[30] == r["radius"], where
    assert n >= 1000, n


def test_symbols_exported_and_declared():
    names = ["cp_pose_targets_track_workspace_bytes", "cp_pose_targets_track"]
    assert all(n in hip.exported_symbols() for n in names)
    hdr = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    for n in names:
        assert re.search(r"\b%s\(" % n, hdr), n
    so = hip.LIB_PATH
    if os.path.exists(so):
        nm = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
        for n in names:
            assert re.search(r"\bT %s$" % n, nm, re.M), n
    # the record layouts are stated once per language: the header, the shared device/host header and the binding
    common = open(os.path.join(REPO, "centerpose_amd", "csrc", "pose_targets_track_common.h")).read()
    for src in (hdr, common):
        for name, v in (("IMG_STRIDE", hip.PTK_IMG_STRIDE), ("PRE_STRIDE", hip.PTK_PRE_STRIDE),
                        ("CUR_STRIDE", hip.PTK_CUR_STRIDE)):
            assert "#define CP_PTK_%s %d\n" % (name, v) in src, name
        for group, table in (("IMG", hip.PTK_IMG), ("PRE", hip.PTK_PRE), ("DRAW", hip.PTK_DRAW), ("CUR", hip.PTK_CUR)):
            for k, v in table.items():
                assert "#define CP_PTK_%s_%s %d\n" % (group, k.upper(), v) in src, (group, k)
        assert len(re.findall(r"#define CP_PTK_", src)) == 3 + sum(map(len, (hip.PTK_IMG, hip.PTK_PRE, hip.PTK_DRAW,
                                                                             hip.PTK_CUR)))
    assert hip.PTK_PRE["draws"] + hip.PTK_NUM_DRAWS <= hip.PTK_PRE_STRIDE and NUM_DRAWS == hip.PTK_NUM_DRAWS + 1
    assert D["joints"] + 8 * D["joint_stride"] == hip.PTK_NUM_DRAWS
    # field for field: the binding's descriptor has the C struct's size (natural alignment on both sides)
    probe = os.path.join(REPO, "tests", "_build", "ptk_sizeof")
    os.makedirs(os.path.dirname(probe), exist_ok=True)
    code = '#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) { printf("%%zu %%zu %%zu", ' \
           'sizeof(cp_pose_targets_track_desc), offsetof(cp_pose_targets_track_desc, hm_disturb), ' \
           'offsetof(cp_pose_targets_track_desc, out_pre_hm)); return 0; }\n' % os.path.join(REPO, "include", "centerpose_hip.h")
    subprocess.run(["gcc", "-x", "c", "-", "-o", probe], input=code, text=True, check=True)
    sizes = [int(v) for v in subprocess.run([probe], capture_output=True, text=True, check=True).stdout.split()]
    T = hip.PoseTargetsTrackDesc
    assert sizes == [ctypes.sizeof(T), T.hm_disturb.offset, T.out_pre_hm.offset]


def _desc(B=2, S=4, K=10, Kp=10):
    recs = {"pt_image": np.zeros((B, hip.PT_IMG_STRIDE)), "pt_objects": np.zeros((B, K, hip.PT_OBJ_STRIDE)),
            "ptk_image": np.zeros((B, hip.PTK_IMG_STRIDE)), "ptk_pre_objects": np.zeros((B, Kp, hip.PTK_PRE_STRIDE)),
            "ptk_cur_objects": np.zeros((B, K, hip.PTK_CUR_STRIDE))}
    img = recs["pt_image"]
    img[:, hip.PT_IMG["width"]], img[:, hip.PT_IMG["height"]], img[:, hip.PT_IMG["num_objs"]] = 640, 480, 2
    recs["pt_objects"][:, :, 0] = 1
    recs["ptk_image"][:, hip.PTK_IMG["num_pre"]] = 3
    recs["ptk_pre_objects"][:, :, 0] = 1
    track = dict(input_w=256, input_h=256, down_ratio=4, pre_hm=1, pre_hm_hp=1, tracking=1, tracking_hp=1)
    d = hip.pose_targets_track_desc(recs, S, 64, {n: 1 for n in hip.PT_FLAGS}, track, {})
    for n in hip.PT_OUTPUTS:
        setattr(d.cur, "out_" + n, 4096)  # never dereferenced: every descriptor below is refused on the host
    for n in hip.PTK_OUTPUTS:
        setattr(d, "out_" + n, 4096)
    return d, recs


@pytest.mark.parametrize("case, msg", [
    ("cur_S0", "S must be >= 1"), ("cur_nullhm", "null output pointer"), ("cur_toomany", "num_objs 11"),
    ("nullrec", "null record pointer"), ("nullprehm", "options turn on"), ("nulltracking", "options turn on"),
    ("nullhpmask", "options turn on"), ("misaligned", "16-byte aligned"), ("input_w", "input_w / input_h"),
    ("input_big", "input_w / input_h"), ("down_ratio", "down_ratio"), ("Kp", "max_pre_objs must be"),
    ("toomanypre", "has 11 previous objects, outside [0, max_pre_objs = 10]"), ("negpre", "-1 previous objects"),
    ("variants", "previous object 1 has 4 symmetry variants, outside [1, S = 1]"),
    ("idsym", "id_symmetry_pre 4, outside [0, 4)"), ("noworkspace", "null workspace"), ("smallworkspace", "too small")])
def test_c_abi_refusals_without_device(case, msg):
    L = hip.lib()
    d, recs = _desc(S=1 if case == "variants" else 4)
    ws, nbytes = None, 0
    if case == "cur_S0":
        d.cur.S = 0
    elif case == "cur_nullhm":
        d.cur.out_hm = None
    elif case == "cur_toomany":
        recs["pt_image"][1, hip.PT_IMG["num_objs"]] = 11
    elif case == "nullrec":
        d.pre_objects = None
    elif case == "nullprehm":
        d.out_pre_hm = None
    elif case == "nulltracking":
        d.out_tracking = None
    elif case == "nullhpmask":
        d.out_tracking_hp_mask = None
    elif case == "misaligned":
        d.out_pre_hm_hp = 4096 + 8
    elif case == "input_w":
        d.input_w = 0
    elif case == "input_big":
        d.input_w = d.input_h = 65536
    elif case == "down_ratio":
        d.down_ratio = 0
    elif case == "Kp":
        d.max_pre_objs = hip.PT_MAX_OBJS + 1
    elif case == "toomanypre":
        recs["ptk_image"][1, hip.PTK_IMG["num_pre"]] = 11
    elif case == "negpre":
        recs["ptk_image"][0, hip.PTK_IMG["num_pre"]] = -1
    elif case == "variants":
        recs["ptk_pre_objects"][0, 1, 0] = 4
    elif case == "idsym":
        recs["ptk_pre_objects"][1, 2, 0], recs["ptk_pre_objects"][1, 2, hip.PTK_PRE["idsym"]] = 4, 4
    elif case == "smallworkspace":
        ws, nbytes = 4096, L.cp_pose_targets_track_workspace_bytes(ctypes.byref(d)) - 1
        assert nbytes > 0
    rc = L.cp_pose_targets_track(None, ctypes.byref(d), ws, nbytes)
    assert rc == hip.CP_ERR_INVALID
    assert msg in L.cp_last_error().decode()


def test_workspace_query():
    L = hip.lib()
    d, _ = _desc()
    cur = L.cp_pose_targets_workspace_bytes(ctypes.byref(d.cur))
    assert L.cp_pose_targets_track_workspace_bytes(ctypes.byref(d)) > cur > 0
    d.max_pre_objs = 0
    assert L.cp_pose_targets_track_workspace_bytes(ctypes.byref(d)) == 0


def test_draw_track_noise():
    for rng in (np.random.default_rng(3), np.random.RandomState(3), None):
        if rng is None:
            np.random.seed(3)
        d = draw_track_noise(rng, 500)
        assert d.shape == (500, NUM_DRAWS) and d.dtype == np.float64
        j = d[:, D["joints"]:hip.PTK_NUM_DRAWS].reshape(500, 8, D["joint_stride"])
        tn = np.concatenate([d[:, :2].ravel(), j[:, :, :2].ravel()])
        assert np.abs(tn).max() <= 3 and np.abs(tn).max() > 2.5 and abs(tn.std() - 0.9866) < 0.03  # truncnorm(-3, 3)
        for u in (d[:, D["ct_lost"]], d[:, D["ct_heat"]], d[:, D["ct_fp"]], j[:, :, D["j_lost"]], j[:, :, D["j_fp"]], d[:, 64]):
            assert 0 <= u.min() and u.max() < 1 and abs(u.mean() - 0.5) < 0.07
        assert 0 <= d[:, D["ct_fp_peak"]].min() and 0.3 < d[:, D["ct_fp_peak"]].max() < 0.4
        assert 0 <= j[:, :, D["j_fp_peak"]].min() and 0.25 < j[:, :, D["j_fp_peak"]].max() < 0.3
        nrm = np.concatenate([d[:, D["ct_fp_noise"]:D["ct_fp_noise"] + 2].ravel(), j[:, :, 4:6].ravel()])
        assert np.abs(nrm).max() > 3 and abs(nrm.std() - 1) < 0.05
    assert draw_track_noise(None, 0).shape == (0, NUM_DRAWS)


def _frames(rng, specs, pre_spec, w=640, h=480):
    anns = TC.name_objects(PC.synth_annotations(rng, specs, w, h))
    return anns, TC.previous_frame(rng, anns, pre_spec)


def test_packer():
    rng = np.random.default_rng(0)
    eye = np.eye(2, 3)
    specs = [(None, "pose"), ("True", "pose"), (None, "pose"), ("False", "pose"), (None, "pose")]
    anns, pre = _frames(rng, specs, [(4, None, False), (0, "obj_9", False), (1, None, False)])
    opt = TC.make_opt(c="bottle", num_symmetry=6)
    draws = draw_track_noise(rng, 3)
    draws[:, 64] = [0.99, 0.5, 0.26]
    r = pack_track_annotations(anns, pre, eye, 2 * eye, 640, 480, True, 5.0, opt, draws)
    # the variant count: carried inside the previous frame (6, 6, 4), then ACROSS the frames into the current one
    assert r["ptk_pre_objects"][:3, 0].tolist() == [6, 6, 4]
    assert r["pt_objects"][:5, 0].tolist() == [4, 4, 4, 1, 1]
    assert r["ptk_pre_objects"][:3, hip.PTK_PRE["idsym"]].tolist() == [5, 3, 1]  # int(u * n)
    # id codes: small integers per sample, equal where opt.c + name.split('_')[1] is
    pid, cid = r["ptk_pre_objects"][:3, hip.PTK_PRE["id"]], r["ptk_cur_objects"][:5, 0]
    assert pid[0] == cid[4] and pid[2] == cid[1] and pid[1] not in cid and len(set(cid)) == 5
    assert max(pid.max(), cid.max()) <= 5
    assert r["ptk_image"][:7].tolist() == [2, 0, 0, 0, 2, 0, 3] and r["ptk_pre_objects"].shape == (10, 128)
    assert np.array_equal(r["ptk_pre_objects"][:3, 64:], draws[:, :64])
    assert np.array_equal(r["ptk_image"][7:23], np.ravel(pre["camera_data"]["camera_projection_matrix"]))
    # where the previous frame's loop ends on the category's count, the current records are pack_annotations' own
    from centerpose_amd.pose_targets import pack_annotations
    anns2, pre2 = _frames(rng, specs, [(0, None, False), (2, None, False)])
    r2 = pack_track_annotations(anns2, pre2, eye, eye, 640, 480, False, 0.0, TC.make_opt(c="bottle", num_symmetry=6,
                                                                                         pre_hm_hp=False),
                                draw_track_noise(rng, 2), max_pre_objs=4)
    plain = pack_annotations(anns2, eye, 640, 480, False, 0.0, TC.make_opt(c="bottle", num_symmetry=6))
    assert np.array_equal(r2["pt_image"], plain["pt_image"]) and np.array_equal(r2["pt_objects"], plain["pt_objects"])
    assert r2["ptk_pre_objects"].shape == (4, 128)
    # ValueErrors
    with pytest.raises(ValueError, match="max_pre_objs is 2"):
        pack_track_annotations(anns, pre, eye, eye, 640, 480, False, 0.0, opt, draws, max_pre_objs=2)
    with pytest.raises(ValueError, match="id_symmetry_pre_list"):  # current object 3.. beyond the previous frame, S > 1
        pack_track_annotations(anns, {"camera_data": pre["camera_data"], "objects": pre["objects"][:1]}, eye, eye, 640,
                               480, False, 0.0, opt, draws[:1])
    with pytest.raises(ValueError, match="S = 1"):
        pack_track_annotations(anns, pre, eye, eye, 640, 480, False, 0.0, TC.make_opt(c="camera"), draws)
    with pytest.raises(ValueError, match="draws must be"):
        pack_track_annotations(anns, pre, eye, eye, 640, 480, False, 0.0, opt, draws[:2])
    # cup: the previous objects' own skips and the current frame's, from the LAST previous object
    cup = TC.make_opt(c="cup", mug=False, num_symmetry=6)
    pre["objects"][1]["mug"], pre["objects"][2]["mug"] = True, True
    r = pack_track_annotations(anns, pre, eye, eye, 640, 480, False, 0.0, cup, draws)
    assert r["ptk_pre_objects"][:3, hip.PTK_PRE["skip"]].tolist() == [0, 1, 1] and r["ptk_cur_objects"][:5, 1].all()
    with pytest.raises(ValueError, match="needs a previous object"):
        pack_track_annotations(anns, {"camera_data": pre["camera_data"], "objects": []}, eye, eye, 640, 480, False, 0.0,
                               cup, draws[:0])


def test_python_refusals():
    with pytest.raises(NotImplementedError, match="data_generation_mode_ratio"):
        TrackPoseTargets(TC.make_opt(data_generation_mode_ratio=0.5))
    for name in ("dense_hp", "mse_loss"):
        with pytest.raises(NotImplementedError, match=name):
            TrackPoseTargets(TC.make_opt({name: True}))
    with pytest.raises(NotImplementedError, match="split"):
        TrackPoseTargets(TC.make_opt(), split="val")
    with pytest.raises(NotImplementedError, match="debug"):
        TrackPoseTargets(TC.make_opt(debug=1))
    with pytest.raises(ValueError, match="tracking_task"):
        TrackPoseTargets(PC.make_opt())
    with pytest.raises(ValueError, match="max_pre_objs"):
        TrackPoseTargets(TC.make_opt(), max_pre_objs=65)
    t = TrackPoseTargets(TC.make_opt(pre_hm=False, tracking_hp=False), max_pre_objs=32)
    assert (t.K, t.Kp) == (10, 32) and "pre_hm" not in t.keys and "tracking_hp" not in t.keys
    assert t.keys[-3:] == ["pre_hm_hp", "tracking", "tracking_mask"]
    # PoseTargets still refuses the tracking options, and names the class that builds them
    for name in ("tracking_task", "pre_hm", "pre_hm_hp", "tracking", "tracking_hp"):
        with pytest.raises(NotImplementedError, match=name):
            PoseTargets(PC.make_opt({name: True}))
    with pytest.raises(NotImplementedError, match="TrackPoseTargets"):
        PoseTargets(PC.make_opt(tracking_task=True))
