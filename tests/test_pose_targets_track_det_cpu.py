"""CPU tests of the tracking task's training targets with the detector in the loop (no GPU): the host restatement
tests/pose_targets_track_det_ref.py against the reference-built goldens (and against the reference's live __getitem__
with a stub detector where that tree is present), the events the golden cases must contain, the condition the cases
are built under (no near-tie in any argmin), the host build of pose_targets_track_det_common.h against the restatement
image by image and object by object, the packer's new records, the C ABI's declarations, layouts and refusals with no
device, and the Python layer's refusals."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from centerpose_amd import hip
from centerpose_amd.pose_targets import num_symmetry
from centerpose_amd.pose_targets_track import (TrackPoseTargets, draw_generation_mode, draw_track_noise,
                                               pack_track_annotations, track_target_keys)
from tests import pose_target_cases as PC
from tests import pose_target_track_cases as TC
from tests import pose_target_track_det_cases as DC
from tests import pose_targets_track_det_ref as DR
from tests import pose_targets_track_ref as TR

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(REPO, "tests", "golden", "pose_targets_track_det_ref.npz")
MAPS = ("hm", "hm_hp", "pre_hm", "pre_hm_hp")
RECORDS = ("pt_image", "pt_objects", "ptk_image", "ptk_pre_objects", "ptk_cur_objects", "ptk_gen", "ptk_det_meta")
NAMES = sorted(DC.CASES) + [n + "@0" for n in DC.MODE0]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def case_opt(name):
    return DC.make_opt(DC.CASES[name.split("@")[0]]["over"])


def golden_records(gold, name):
    return {k: gold[name + "/" + k] for k in RECORDS}


def golden_rows(gold, name):
    return gold[name + "/det_post"], int(gold[name + "/det_count"]), gold[name + "/det_pnp"]


def golden_arrays(gold, name, opt):
    """The golden case's ret as dense arrays (no batch axis)."""
    S, Rr, H, W = num_symmetry(opt), opt.output_res, opt.input_h, opt.input_w
    shape = {"hm": (S, 1, Rr, Rr), "hm_hp": (S, 8, Rr, Rr), "pre_hm": (1, H, W), "pre_hm_hp": (8, H, W)}
    out = {}
    for k in track_target_keys(opt):
        if k in MAPS:
            m = np.zeros(shape[k], np.float32)
            m.reshape(-1)[gold["%s/%s_idx" % (name, k)]] = gold["%s/%s_val" % (name, k)]
            out[k] = m
        else:
            out[k] = gold["%s/%s" % (name, k)]
    return out


def restate(recs, rows, opt):
    """One image's records and detector rows -> the restatement's arrays and per-object dicts."""
    boxes = DC.boxes_of(recs, *rows, opt)
    return DR.image_targets(recs, boxes, num_symmetry(opt), opt.output_res, TR.options(opt), DR.det_options(opt),
                            opt.use_absolute_scale), boxes


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_goldens(gold, name):
    opt = case_opt(name)
    r, _ = restate(golden_records(gold, name), golden_rows(gold, name), opt)
    for k, v in golden_arrays(gold, name, opt).items():
        assert same_bits(r[k], v), k  # floats and maps bit for bit


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_cases_have_no_near_tie(gold, name):
    """No argmin of a case hangs on the order in which a float64 sum was taken: the two smallest norms of every box
    differ by more than 1e-9 relative or are exactly equal, likewise the boxes competing for one object."""
    opt = case_opt(name)
    recs = golden_records(gold, name)
    assert DC.no_near_tie(recs, DC.boxes_of(recs, *golden_rows(gold, name), opt))


def test_goldens_cover_the_events(gold):
    """Each event the cases were written for is in the golden file (read off the restatement, which the test above pins
    to the reference's arrays)."""
    res, boxes, slots = {}, {}, {}
    for n in DC.CASES:
        recs, rows = golden_records(gold, n), golden_rows(gold, n)
        res[n], boxes[n] = restate(recs, rows, case_opt(n))
        slots[n] = DR.boxes_from_records(*rows, 640, 480, case_opt(n).c, return_slots=True)[1] if n != "rect" else None
    pre = {n: res[n]["pre"] for n in res}
    opt = case_opt
    # no boxes at all: no detection, and detections none of which becomes a box; nothing is drawn, label mode 0 tracks
    assert int(gold["empty/det_count"]) == 0 and int(gold["no_boxes/det_count"]) == 3 and not boxes["no_boxes"]
    for n in ("empty", "no_boxes"):
        assert all(q["kept"] and not q["draws"] for q in pre[n]) and not res[n]["pre_hm"].any()
    assert opt("no_boxes").tracking_label_mode == 0 and gold["no_boxes/tracking_mask"].sum() == 3
    assert opt("empty").tracking_label_mode == 1 and gold["empty/tracking_mask"].sum() == 0
    # a box rejected by the shell rule: slot 4 solved (status 1) and is no box; slot 1 failed
    assert gold["plain_hp2/det_pnp"][[1, 4], 0].tolist() == [0, 1] and slots["plain_hp2"] == [0, 2, 3, 5]
    # ... and one that the 3-point rule rejects and the 6-point rule keeps
    assert slots["flipped_l0"] == [0, 1] and int(gold["flipped_l0/det_count"]) == 3
    assert slots["chair_s4"] == [0, 1, 2, 3]
    # two boxes with the same argmin: the nearer wins
    nl = res["plain_hp2"]["norms"]
    assert np.argmin(nl, 1).tolist() == [1, 0, 1, 3] and nl[0, 1] < nl[2, 1] and res["plain_hp2"]["match"] == [1, 0, None, 3]
    # an exact tie between twin annotations: the lowest index wins, the twin goes without
    nl = res["twins_hp0"]["norms"]
    assert nl[0, 1] == nl[0, 2] and res["twins_hp0"]["match"][1:3] == [0, None]
    # several boxes whose nearest object is one and the same, all farther than 1000: dropped
    nl = res["far_multi"]["norms"]
    assert (np.argmin(nl, 1) == 0).all() and nl.min() > 1000 and res["far_multi"]["match"] == [None, None]
    # a single far match is accepted
    assert res["far_single"]["norms"][0, 0] > 1000 and res["far_single"]["match"] == [0]
    assert pre["far_single"][0]["event"]["drawn"] == 8 and res["far_single"]["pre_hm"].any()
    # an annotation with an invisible centre among visible ones: -10000 rows, never matched, still in the lists
    inst = DR.instances_2d(gold["invisible_mix/pt_image"], gold["invisible_mix/ptk_pre_objects"], 3)
    assert (inst[1] == -10000).all() and inst[0].min() > 0 and res["invisible_mix"]["match"] == [1, None, 0]
    assert pre["invisible_mix"][1]["kept"] and pre["invisible_mix"][1]["cts"] is None
    # a detector point outside the input: from kps (render_hmhp_mode 0) and from the reprojection (3)
    assert pre["twins_hp0"][3]["event"] == {"outside": 1, "radius0": 0, "drawn": 7}
    assert pre["invisible_mix"][0]["event"] == {"outside": 1, "radius0": 0, "drawn": 7}
    # radius_detector <= 0 gates the joints under render_hmhp_mode 0 and not the centre
    assert pre["twins_hp0"][0]["event"]["radius0"] == 8 and [c for c, _, _, _ in pre["twins_hp0"][0]["draws"]] == [0]
    assert pre["rect"][0]["event"]["radius0"] == 8
    # score == 0 under render_hm_mode 1: the score read is the image's last box's, so no centre is drawn and no variant
    # chosen, whatever the matched box's own score
    assert opt("plain_hp2").render_hm_mode == 1 and gold["plain_hp2/det_post"][5, 0] == 0 and gold["plain_hp2/det_post"][0, 0] > 0
    assert all(k == 0 for q in pre["plain_hp2"] for c, _, _, k in q["draws"] if c == 0)
    assert all(q["chosen"] is None for q in pre["plain_hp2"]) and not res["plain_hp2"]["pre_hm"].any()
    assert any(q["chosen"] is not None for q in pre["twins_hp0"]) and res["twins_hp0"]["pre_hm"].any()
    # both tracking_label_modes with a matched object, all four render_hmhp_modes with joints drawn, both render_hm_modes
    for mode in (0, 1):
        assert any(opt(n).tracking_label_mode == mode and any(m is not None for m in res[n]["match"]) for n in res)
        assert any(opt(n).render_hm_mode == mode and res[n]["pre_hm"].any() for n in res)
    for mode in range(4):
        assert any(opt(n).render_hmhp_mode == mode and res[n]["pre_hm_hp"].any() for n in res), mode
    # peaks: 1 under render_hmhp_mode 1 / 3, kps_heatmap_height (float32 values) under 0 / 2
    assert all(k == 1 for c, _, _, k in pre["far_single"][0]["draws"])
    hs = set(np.float32(gold["plain_hp2/det_post"][:6, 112:120]).astype(np.float64).ravel().tolist())
    assert all(k in hs for q in pre["plain_hp2"] for c, _, _, k in q["draws"] if c > 0)
    # a flipped frame, a chair (S = 4) whose chosen variant filters the current frame, a rectangular input
    assert gold["flipped_l0/pt_image"][8] == 1 and gold["rect/pt_image"][8] == 1 and gold["plain_hp2/pt_image"][8] == 0
    assert gold["chair_s4/ind"].shape[0] == 4 and gold["chair_s4/pt_objects"][0, 0] == 4
    ch = pre["chair_s4"][0]["chosen"]
    assert ch is not None and gold["chair_s4/reg_mask"][:, 0].tolist() == [int(s == ch) for s in range(4)]
    assert (opt("rect").input_w, opt("rect").input_h) == (320, 256) and res["rect"]["pre_hm"].shape == (1, 256, 320)
    # the same sample in both modes, for the batch that mixes them
    assert gold["plain_hp2@0/ptk_gen"][0] == 0 and gold["plain_hp2/ptk_gen"][0] == 1
    assert np.array_equal(gold["plain_hp2@0/ptk_pre_objects"], gold["plain_hp2/ptk_pre_objects"])
    assert not same_bits(golden_arrays(gold, "plain_hp2@0", opt("plain_hp2"))["pre_hm_hp"], res["plain_hp2"]["pre_hm_hp"])


def test_mixed_batch_restatement(gold):
    """A batch of modes (0, 1, 0): each image is its own golden."""
    opt = case_opt("plain_hp2")
    names = ("plain_hp2@0", "plain_hp2", "plain_hp2@0")
    recs = {k: np.stack([gold[n + "/" + k] for n in names]) for k in RECORDS}
    boxes = [DC.boxes_of(golden_records(gold, n), *golden_rows(gold, n), opt) for n in names]
    r = DR.batch_targets(recs, boxes, num_symmetry(opt), opt.output_res, TR.options(opt), DR.det_options(opt))
    for b, n in enumerate(names):
        for k, v in golden_arrays(gold, n, opt).items():
            assert same_bits(r[k][b], v), (n, k)


def test_restatement_equals_live_reference():
    if not PC.reference_available():
        pytest.skip("the reference tree is not present")
    matched = 0
    for seed in range(300, 314):
        res = (64, 96)[seed % 2]
        opt, anns, pre, w, h, sd, draws = DC.random_case(seed, output_res=res, input_res=4 * res, input_w=4 * res,
                                                         input_h=4 * res)
        pre0 = pack_track_annotations(anns, pre, np.eye(2, 3), np.eye(2, 3), w, h, opt.flip >= 1.0, 0.0, opt, draws)
        slots = DC.random_slots(np.random.default_rng([seed, 5]), pre0, 1 + seed % 7)
        recs, rows, ret = DC.reference_case(opt, anns, pre, w, h, sd, draws, slots)
        r, boxes = restate(recs, rows, opt)
        assert DC.no_near_tie(recs, boxes), seed
        matched += sum(m is not None for m in r["match"])
        for k in track_target_keys(opt):
            assert same_bits(r[k], ret[k]), (seed, k)
    assert matched >= 10, matched


# ---- the host build of the shared header ----

def _host():
    out = os.path.join(REPO, "tests", "_build", "libcp_pose_targets_track_det_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(REPO, "tests", "native", "pose_targets_track_det_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
    L = ctypes.CDLL(out)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.ptkd_host_match.argtypes = [vp, vp, ci, ci, vp, vp, ci, ci, vp]
    L.ptkd_host_pre_object.argtypes = [vp, vp, vp, ctypes.c_double, ci, vp, vp, vp]
    return L


def test_host_build_equals_restatement():
    L = _host()
    rng = np.random.default_rng(16)
    out, n, n_matched = np.zeros(103, np.float64), 0, 0
    for S, cat in ((4, "chair"), (1, "camera"), (12, "bottle"), (1, "shoe")):
        for trial in range(16):
            opt = DC.make_opt(dict(c=cat, num_symmetry=S, center_3D=bool(trial & 1), tracking_label_mode=(trial >> 1) & 1,
                                   render_hmhp_mode=trial % 4, render_hm_mode=(trial >> 2) & 1,
                                   input_w=(256, 320)[trial % 2], pre_hm=trial != 9, pre_hm_hp=trial != 10))
            op, dop = TR.options(opt), DR.det_options(opt)
            ov = np.array([float(getattr(op, k)) for k in TR.OPT_NAMES])
            dv = np.array([dop.render_hm_mode, dop.render_hmhp_mode, hip.PTK_CAT_RULE[cat]], np.int32)
            for _ in range(5):
                recs, (post, count, pnp) = DC.random_image(rng, opt)
                npre = int(recs["ptk_image"][hip.PTK_IMG["num_pre"]])
                img = np.ascontiguousarray(recs["pt_image"])
                pobj = np.ascontiguousarray(recs["ptk_pre_objects"])
                boxes, slot_of = DR.boxes_from_records(post, count, pnp, int(img[6]), int(img[7]), cat, return_slots=True)
                sel, _ = DR.match(DR.instances_2d(img, pobj, npre), boxes) if boxes else ([None] * npre, None)
                m = np.zeros((npre, 64), np.float64)
                L.ptkd_host_match(img.ctypes.data, pobj.ctypes.data, npre, int(dv[2]), post.ctypes.data, pnp.ctypes.data, count,
                                  post.shape[0], m.ctypes.data)
                assert m[:, 0].tolist() == [-1 if s is None else slot_of[s] for s in sel], (S, trial)
                last = boxes[-1][4]["score"] if boxes else 0.0
                assert (m[:, 1] == last).all()
                im = np.ascontiguousarray(TR.pre_image(img, recs["ptk_image"]))
                scale = float(recs["ptk_gen"][hip.PTK_GEN["radius_scale"]])
                for k in range(npre):
                    L.ptkd_host_pre_object(im.ctypes.data, pobj[k].ctypes.data, m[k].ctypes.data, scale, S, ov.ctypes.data,
                                           dv.ctypes.data, out.ctypes.data)
                    r = DR.pre_object_det(im, pobj[k], None if sel[k] is None else boxes[sel[k]], last, scale, S, op, dop)
                    n, n_matched = n + 1, n_matched + (sel[k] is not None)
                    where = (S, trial, k)
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
    assert n >= 1000 and 200 <= n_matched <= n - 200, (n, n_matched)


# ---- the packer ----

def _sample(rng):
    opt = DC.make_opt(dict(c="camera"))
    anns = TC.name_objects(PC.synth_annotations(rng, [(None, "pose")] * 3, 640, 480))
    pre = TC.previous_frame(rng, anns, [(0, None, False), (2, None, False)])
    pre["camera_data"]["intrinsics"] = {"fx": 700.0, "fy": 710.0, "cx": 320.5, "cy": 239.5}
    return opt, anns, pre, draw_track_noise(rng, 2)


def test_packer_generation_records():
    from centerpose_amd.lib.utils.image import get_affine_transform

    opt, anns, pre, draws = _sample(np.random.default_rng(2))
    t_out, t_in = np.array([[0.1, 0, 1], [0, 0.1, 2.0]]), np.array([[0.4, 0, 3], [0, 0.4, 4.0]])
    base = pack_track_annotations(anns, pre, t_out, t_in, 640, 480, False, 0.0, opt, draws)
    assert sorted(base) == ["pt_image", "pt_objects", "ptk_cur_objects", "ptk_image", "ptk_pre_objects"]  # as before
    c, s = np.array([310.0, 250.0], np.float32), 700.0
    for mode in (0, 1):
        gen = dict(mode=mode, c=c, s=s, aug_s=1.125, intrinsics=pre["camera_data"]["intrinsics"])
        r = pack_track_annotations(anns, pre, t_out, t_in, 640, 480, False, 0.0, opt, draws, generation=gen)
        assert sorted(set(r) - set(base)) == ["ptk_det_meta", "ptk_gen"]
        for k, v in base.items():  # the existing records stay bit-identical
            assert same_bits(r[k], v), k
        assert r["ptk_gen"].dtype == np.float64 and r["ptk_gen"].tolist() == [mode, 1.125, 0, 0]
        m = r["ptk_det_meta"]
        assert m.dtype == np.float64 and m.shape == (12,)
        assert np.array_equal(m[:6], get_affine_transform(c, s, 0, (opt.output_res, opt.output_res), inv=1).reshape(-1))
        assert m[6] == s / opt.output_res and m[7] == 0 and m[8:].tolist() == [700.0, 710.0, 320.5, 239.5]
    r = pack_track_annotations(anns, pre, t_out, t_in, 640, 480, False, 0.0, opt, draws,
                               generation=dict(c=c, s=s, aug_s=1.0, intrinsics=pre["camera_data"]["intrinsics"]))
    assert r["ptk_gen"][0] == 1  # a dict without 'mode' is mode 1
    with pytest.raises(ValueError, match="mode"):
        pack_track_annotations(anns, pre, t_out, t_in, 640, 480, False, 0.0, opt, draws,
                               generation=dict(mode=2, c=c, s=s, aug_s=1.0, intrinsics=pre["camera_data"]["intrinsics"]))


def test_draw_generation_mode():
    rng = np.random.default_rng(4)
    assert abs(np.mean([draw_generation_mode(rng, 0.3) for _ in range(4000)]) - 0.3) < 0.03
    assert draw_generation_mode(rng, 0.0) == 0 and draw_generation_mode(rng, 1.0) == 1
    np.random.seed(5)
    u = np.random.RandomState(5).random_sample()
    assert draw_generation_mode(None, 0.5) == int(u < 0.5)  # numpy's global state, one uniform, as :465


# ---- the Python layer's refusals (no device is touched) ----

class _Model:
    tracking_task = False

    def detect(self, *a, **k):
        raise AssertionError("not reached")


def test_python_refusals():
    opt = DC.make_opt(dict(c="camera", data_generation_mode_ratio=0.3))
    with pytest.raises(NotImplementedError, match="data_generation_mode_ratio"):
        TrackPoseTargets(opt)
    with pytest.raises(NotImplementedError, match="rep_mode 2"):
        TrackPoseTargets(opt, detector=_Model(), det_opt=SimpleNamespace(rep_mode=2))
    with pytest.raises(ValueError, match="K must be"):
        TrackPoseTargets(opt, detector=_Model(), det_opt=SimpleNamespace(K=129))
    with pytest.raises(ValueError, match="render_hm"):
        TrackPoseTargets(DC.make_opt(dict(c="camera", render_hmhp_mode=4)), detector=_Model())
    with pytest.raises(ValueError, match="tracking inputs"):
        TrackPoseTargets(opt, detector=SimpleNamespace(tracking_task=True, detect=None))
    # the reference's CenterPoseTrack options (main_CenterPoseTrack.py) are accepted with a detector
    main = DC.make_opt(dict(c="camera", data_generation_mode_ratio=0.3, render_hm_mode=1, render_hmhp_mode=2,
                            tracking_label_mode=1))
    t = TrackPoseTargets(main, detector=_Model())
    assert t.det == {"vis_thresh": 0.3, "nms": False, "K": 100, "rep_mode": 1}  # opts().init's
    assert t.render == {"render_hm_mode": 1, "render_hmhp_mode": 2, "cat_rule": 0}
    # a mode-1 record without pre_img, and without a detector
    rng = np.random.default_rng(3)
    _, anns, pre, draws = _sample(rng)
    gen = dict(mode=1, c=np.array([320.0, 240.0], np.float32), s=640.0, aug_s=1.0, intrinsics=pre["camera_data"]["intrinsics"])
    r = pack_track_annotations(anns, pre, np.eye(2, 3), np.eye(2, 3), 640, 480, False, 0.0, main, draws, generation=gen)
    recs = {k: v[None] for k, v in r.items()}
    with pytest.raises(ValueError, match="pre_img"):
        t(recs)
    with pytest.raises(ValueError, match="no detector"):
        TrackPoseTargets(DC.make_opt(dict(c="camera", data_generation_mode_ratio=0)))(recs)


# ---- the C ABI ----

def test_symbols_exported_and_declared():
    names = ["cp_pose_targets_track_det_workspace_bytes", "cp_pose_targets_track_det"]
    assert all(n in hip.exported_symbols() for n in names)
    hdr = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    for n in names:
        assert re.search(r"\b%s\(" % n, hdr), n
    assert "#define CP_ABI_VERSION 7\n" in hdr and hip.lib().cp_abi_version() == 7
    mk = open(os.path.join(REPO, "centerpose_amd", "csrc", "Makefile")).read()
    assert "pose_targets_track_det.hip" in mk and "pose_targets_track_det_common.h" in mk
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    for n in names:
        assert re.search(r"\bT %s$" % n, nm, re.M), n
    # the record layout is stated once per language
    common = open(os.path.join(REPO, "centerpose_amd", "csrc", "pose_targets_track_det_common.h")).read()
    for src in (hdr, common):
        assert "#define CP_PTKD_GEN_STRIDE %d\n" % hip.PTK_GEN_STRIDE in src
        assert "#define CP_PTKD_MAX_K %d\n" % hip.PTK_DET_MAX_K in src
        for k, v in hip.PTK_GEN.items():
            assert "#define CP_PTKD_GEN_%s %d\n" % (k.upper(), v) in src
    # field for field: the binding's descriptor has the C struct's size and offsets
    probe = os.path.join(REPO, "tests", "_build", "ptkd_sizeof")
    os.makedirs(os.path.dirname(probe), exist_ok=True)
    code = '#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) { printf("%%zu %%zu %%zu %%zu", ' \
           'sizeof(cp_pose_targets_track_det_desc), offsetof(cp_pose_targets_track_det_desc, det_post), ' \
           'offsetof(cp_pose_targets_track_det_desc, K_det), offsetof(cp_pose_targets_track_det_desc, gen)); return 0; }\n' \
           % os.path.join(REPO, "include", "centerpose_hip.h")
    subprocess.run(["gcc", "-x", "c", "-", "-o", probe], input=code, text=True, check=True)
    sizes = [int(v) for v in subprocess.run([probe], capture_output=True, text=True, check=True).stdout.split()]
    T = hip.PoseTargetsTrackDetDesc
    assert sizes == [ctypes.sizeof(T), T.det_post.offset, T.K_det.offset, T.gen.offset]


def _desc(B=2, S=4, K=10, Kp=10):
    recs = {"pt_image": np.zeros((B, hip.PT_IMG_STRIDE)), "pt_objects": np.zeros((B, K, hip.PT_OBJ_STRIDE)),
            "ptk_image": np.zeros((B, hip.PTK_IMG_STRIDE)), "ptk_pre_objects": np.zeros((B, Kp, hip.PTK_PRE_STRIDE)),
            "ptk_cur_objects": np.zeros((B, K, hip.PTK_CUR_STRIDE)), "ptk_gen": np.zeros((B, hip.PTK_GEN_STRIDE))}
    img = recs["pt_image"]
    img[:, hip.PT_IMG["width"]], img[:, hip.PT_IMG["height"]], img[:, hip.PT_IMG["num_objs"]] = 640, 480, 2
    recs["pt_objects"][:, :, 0] = 1
    recs["ptk_image"][:, hip.PTK_IMG["num_pre"]] = 3
    recs["ptk_pre_objects"][:, :, 0] = 1
    recs["ptk_gen"][:, 0], recs["ptk_gen"][:, 1] = (0, 1), 1.0
    track = dict(input_w=256, input_h=256, down_ratio=4, pre_hm=1, pre_hm_hp=1, tracking=1, tracking_hp=1)
    d = hip.PoseTargetsTrackDetDesc()
    d.track = hip.pose_targets_track_desc(recs, S, 64, {n: 1 for n in hip.PT_FLAGS}, track, {})
    for n in hip.PT_OUTPUTS:
        setattr(d.track.cur, "out_" + n, 4096)  # never dereferenced: every descriptor below is refused on the host
    for n in hip.PTK_OUTPUTS:
        setattr(d.track, "out_" + n, 4096)
    d.det_post, d.det_count, d.det_pnp, d.gen = 4096, 4096, 4096, recs["ptk_gen"].ctypes.data
    d.K_det, d.render_hm_mode, d.render_hmhp_mode, d.cat_rule = 100, 1, 2, 0
    return d, recs


@pytest.mark.parametrize("case, msg", [
    ("null", "null descriptor"), ("track_Kp", "max_pre_objs must be"), ("track_nullrec", "null record pointer"),
    ("nullpost", "null detector record"), ("nullcount", "null detector record"), ("nullpnp", "null detector record"),
    ("nullgen", "null gen record"), ("misaligned_post", "aligned"), ("misaligned_count", "aligned"), ("K0", "K_det must be"),
    ("K129", "K_det must be"), ("mode2", "image 1 has data generation mode 2"), ("modehalf", "image 0 has data generation mode 0.5"),
    ("scale_nan", "image 1 has a radius scale that is not finite"), ("hm2", "render_hm_mode"), ("hmhp4", "render_hmhp_mode"),
    ("hmhp_neg", "render_hmhp_mode"), ("cat3", "cat_rule"), ("noworkspace", "null workspace"), ("smallworkspace", "too small")])
def test_c_abi_refusals_without_device(case, msg):
    L = hip.lib()
    d, recs = _desc()
    ws, nbytes = None, 0
    ref = ctypes.byref(d)
    if case == "null":
        ref = None
    elif case == "track_Kp":
        d.track.max_pre_objs = hip.PT_MAX_OBJS + 1
    elif case == "track_nullrec":
        d.track.pre_objects = None
    elif case == "nullpost":
        d.det_post = None
    elif case == "nullcount":
        d.det_count = None
    elif case == "nullpnp":
        d.det_pnp = None
    elif case == "nullgen":
        d.gen = None
    elif case == "misaligned_post":
        d.det_post = 4096 + 4
    elif case == "misaligned_count":
        d.det_count = 4096 + 2
    elif case == "K0":
        d.K_det = 0
    elif case == "K129":
        d.K_det = 129
    elif case == "mode2":
        recs["ptk_gen"][1, 0] = 2
    elif case == "modehalf":
        recs["ptk_gen"][0, 0] = 0.5
    elif case == "scale_nan":
        recs["ptk_gen"][1, 1] = np.nan
    elif case == "hm2":
        d.render_hm_mode = 2
    elif case == "hmhp4":
        d.render_hmhp_mode = 4
    elif case == "hmhp_neg":
        d.render_hmhp_mode = -1
    elif case == "cat3":
        d.cat_rule = 3
    elif case == "smallworkspace":
        ws, nbytes = 4096, L.cp_pose_targets_track_det_workspace_bytes(ctypes.byref(d)) - 1
        assert nbytes > 0
    rc = L.cp_pose_targets_track_det(None, ref, ws, nbytes)
    assert rc == hip.CP_ERR_INVALID
    assert msg in L.cp_last_error().decode()


def test_workspace_query():
    L = hip.lib()
    d, _ = _desc()
    track = L.cp_pose_targets_track_workspace_bytes(ctypes.byref(d.track))
    n = L.cp_pose_targets_track_det_workspace_bytes(ctypes.byref(d))
    assert n >= track + 2 * hip.PTK_GEN_STRIDE * 8 + 2 * 10 * 64 * 8 and n % 256 == 0
    d.track.max_pre_objs = 0
    assert L.cp_pose_targets_track_det_workspace_bytes(ctypes.byref(d)) == 0
    assert L.cp_pose_targets_track_det_workspace_bytes(None) == 0
