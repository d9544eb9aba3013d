"""CPU tests of the ObjectPose training targets (no GPU): the host restatement tests/pose_targets_ref.py against the
reference-built goldens (and against the reference's live __getitem__ where that tree is present), the host build of
pose_targets_common.h against the restatement object by object, the C ABI's declarations and refusals with no device,
and the Python layer's refusals and record packing."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from centerpose_amd import hip
from centerpose_amd.pose_targets import PoseTargets, num_symmetry, pack_annotations, target_keys
from tests import pose_target_cases as PC
from tests import pose_targets_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(REPO, "tests", "golden", "pose_targets_ref.npz")
MAPS = ("hm", "hm_hp")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def golden_arrays(gold, name, opt):
    """The golden case's ret as dense [1, S, ...] arrays."""
    S, Rr = num_symmetry(opt), opt.output_res
    out = {}
    for k in target_keys(opt):
        if k in MAPS:
            m = np.zeros((1, S, 1 if k == "hm" else 8, Rr, Rr), np.float32)
            m.reshape(-1)[gold["%s/%s_idx" % (name, k)]] = gold["%s/%s_val" % (name, k)]
            out[k] = m
        else:
            out[k] = gold["%s/%s" % (name, k)][None]
    return out


def restate(recs_img, recs_obj, opt):
    return R.batch_targets(recs_img, recs_obj, num_symmetry(opt), opt.output_res, opt.center_3D, opt.use_absolute_scale)


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_restatement_equals_goldens(gold, name):
    opt = PC.make_opt(PC.CASES[name][1])
    r = restate(gold[name + "/pt_image"][None], gold[name + "/pt_objects"][None], opt)
    for k, v in golden_arrays(gold, name, opt).items():
        assert r[k].dtype == v.dtype and r[k].shape == v.shape, k
        assert np.array_equal(r[k].view(np.uint8), v.view(np.uint8)), k  # maps bit for bit


def test_goldens_cover_the_edge_cases(gold):
    def objs(name):
        return gold[name + "/pt_objects"]

    # chair: symmetric, carried over, non-symmetric, carried over (1), symmetric
    assert objs("chair_carry")[:5, 0].tolist() == [4, 4, 1, 1, 4]
    assert gold["chair_carry/reg_mask"][1:, 0].all() and not gold["chair_carry/reg_mask"][1:, 2].any()
    assert objs("bottle_s12")[:3, 0].tolist() == [12, 4, 1] and gold["bottle_s12/reg_mask"].shape == (12, 10)
    cam = gold["camera_s1/reg_mask"][0]
    assert cam[2] == 0 and cam[3] == 1  # centre out of frame: 4 visible corners dropped, 5 kept
    assert gold["camera_s1/hps_mask"][0, 1, :2].tolist() == [0, 0]  # the corner at x = -0.5: stored 0, not visible
    assert gold["flip_on/pt_image"][8] == 1 and gold["flip_off/pt_image"][8] == 0
    wh, rm = gold["rot_flat/wh"][0], gold["rot_flat/reg_mask"][0]
    assert gold["rot_flat/pt_image"][9] != 0 and rm[1] == 1 and (wh[1] == 0).any()  # zero-area box kept under rotation
    assert gold["scale_abs_unc/hps_uncertainty"].any() and "scale_abs_unc/scale_uncertainty" in gold.files
    assert (gold["camera_s1/scale"][0, 4, 0] < 0)  # |scale| / scale[1] with scale[1] < 0
    assert gold["many/pt_image"][10] == 10  # 12 objects in the file, max_objs = 10
    hm = golden_arrays(gold, "many", PC.make_opt(PC.CASES["many"][1]))["hm"]
    assert (hm == 1.0).sum() < 10  # twins share pixels: overlapping Gaussians


def test_restatement_equals_live_reference():
    if not PC.reference_available():
        pytest.skip("the reference tree is not present")
    for seed in range(100, 112):
        cat = ("chair", "bottle", "camera")[seed % 3]
        res = (128, 96, 64)[seed % 3]
        opt, anns, w, h, sd = PC.random_case(seed, cat, n_obj=3 + seed % 6, output_res=res, input_res=4 * res)
        recs, ret = PC.reference_case(opt, anns, w, h, sd)
        r = restate(recs["pt_image"][None], recs["pt_objects"][None], opt)
        for k in target_keys(opt):
            assert r[k][0].dtype == ret[k].dtype and np.array_equal(r[k][0], ret[k]), (seed, k)


def _host():
    out = os.path.join(REPO, "tests", "_build", "libcp_pose_targets_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(REPO, "tests", "native", "pose_targets_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
    L = ctypes.CDLL(out)
    L.pt_host_object.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    return L


def random_records(rng, n_images, S, Rr, category):
    """Packed records of synthetic images with a random output affine (scale, shift, rotation, flip)."""
    kinds = ["pose", "pose", "edge", "twin", "corner_neg", "out4", "out5", "negy", "flat"]
    syms = ["True", "False", None] if S >= 4 else [None]
    opt = PC.make_opt(dict(c=category, num_symmetry=S, output_res=Rr))
    imgs, objs = [], []
    for _ in range(n_images):
        w, h = (640, 480) if rng.random() < 0.5 else (480, 640)
        specs = [(syms[int(rng.integers(len(syms)))], kinds[int(rng.integers(len(kinds)))])
                 for _ in range(int(rng.integers(0, 13)))]
        anns = PC.synth_annotations(rng, specs, w, h)
        s = max(w, h) * rng.uniform(0.6, 1.4) / Rr
        a = np.deg2rad(rng.uniform(-30, 30)) if rng.random() < 0.5 else 0.0
        c = np.array([w / 2 + rng.uniform(-80, 80), h / 2 + rng.uniform(-80, 80)])
        M = np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]]) / s
        t = np.hstack([M, (np.array([Rr / 2, Rr / 2]) - M @ c)[:, None]])
        rec = pack_annotations(anns, t, w, h, rng.random() < 0.5, np.rad2deg(a), opt)
        imgs.append(rec["pt_image"])
        objs.append(rec["pt_objects"])
    return np.stack(imgs), np.stack(objs)


def test_host_build_equals_restatement():
    L = _host()
    rng = np.random.default_rng(5)
    out = np.zeros(52, np.float64)
    n = 0
    for S, cat in ((4, "chair"), (12, "bottle"), (1, "camera"), (6, "cup")):
        Rr = int(rng.choice([64, 96, 128]))
        imgs, objs = random_records(rng, 24, S, Rr, cat)
        for b in range(imgs.shape[0]):
            for k in range(int(imgs[b, R.I["num_objs"]])):
                for s in range(int(objs[b, k, 0])):
                    flags = n % 4  # center_3D (1), use_absolute_scale (2)
                    img, ob = np.ascontiguousarray(imgs[b]), np.ascontiguousarray(objs[b, k])
                    L.pt_host_object(img.ctypes.data, ob.ctypes.data, s, S, Rr, flags, out.ctypes.data)
                    r = R.object_targets(img, ob, s, S, Rr, bool(flags & 1), bool(flags & 2))
                    n += 1
                    assert out[0] == (r is not None), (S, b, k, s)
                    if r is None:
                        continue
                    assert out[1] == r["radius"] and tuple(out[2:4]) == r["ct"] and out[4] == r["ind"]
                    for lo, hi, key in ((5, 7, "wh"), (7, 9, "reg"), (9, 12, "scale")):
                        assert np.array_equal(out[lo:hi].astype(np.float32), np.asarray(r[key]).astype(np.float32)), key
                    ok = {j: (x, y) for j, x, y in r["joints"]}
                    for j in range(8):
                        assert out[12 + j] == (j in ok)
                        if j in ok:
                            assert tuple(out[20 + 2 * j:22 + 2 * j]) == ok[j]
                            assert tuple(out[36 + 2 * j:38 + 2 * j]) == (ok[j][0] - r["ct"][0], ok[j][1] - r["ct"][1])
    assert n >= 1000, n


def test_symbols_exported_and_declared():
    names = ["cp_pose_targets_workspace_bytes", "cp_pose_targets"]
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
    common = open(os.path.join(REPO, "centerpose_amd", "csrc", "pose_targets_common.h")).read()
    for src in (hdr, common):
        assert "#define CP_PT_IMG_STRIDE %d" % hip.PT_IMG_STRIDE in src
        assert "#define CP_PT_OBJ_STRIDE %d" % hip.PT_OBJ_STRIDE in src
        for k, v in hip.PT_IMG.items():
            assert "#define CP_PT_IMG_%s %d" % (k.upper(), v) in src, k
        for k, v in hip.PT_OBJ.items():
            assert "#define CP_PT_OBJ_%s %d" % ({"kps3d": "KPS3D"}.get(k, k.upper()), v) in src, k


def _desc(B=2, S=4, K=10):
    img = np.zeros((B, hip.PT_IMG_STRIDE))
    img[:, hip.PT_IMG["width"]], img[:, hip.PT_IMG["height"]] = 640, 480
    img[:, hip.PT_IMG["num_objs"]] = 2
    obj = np.zeros((B, K, hip.PT_OBJ_STRIDE))
    obj[:, :, 0] = 1
    d = hip.pose_targets_desc(img, obj, S, 64, {n: 1 for n in hip.PT_FLAGS}, {})
    for n in hip.PT_OUTPUTS:
        setattr(d, "out_" + n, 4096)  # never dereferenced: every descriptor below is refused on the host
    return d, img, obj


@pytest.mark.parametrize("case, msg", [
    ("S0", "S must be >= 1"), ("Sneg", "S must be >= 1"), ("nullimg", "null record pointer"),
    ("nullhm", "null output pointer"), ("nullhmhp", "options turn on"), ("toomany", "num_objs 11"),
    ("variants", "has 4 symmetry variants, outside [1, S = 1]"), ("zero_variants", "0 symmetry variants"),
    ("K", "max_objs"), ("joints", "num_joints"), ("misaligned", "16-byte aligned"), ("noworkspace", "null workspace")])
def test_c_abi_refusals_without_device(case, msg):
    L = hip.lib()
    d, img, obj = _desc(S=1 if case == "variants" else 4)
    if case == "S0":
        d.S = 0
    elif case == "Sneg":
        d.S = -3
    elif case == "nullimg":
        d.images = None
    elif case == "nullhm":
        d.out_hm = None
    elif case == "nullhmhp":
        d.out_hm_hp = None
    elif case == "toomany":
        img[1, hip.PT_IMG["num_objs"]] = 11
    elif case == "variants":
        obj[0, 1, 0] = 4
    elif case == "zero_variants":
        obj[1, 0, 0] = 0
    elif case == "K":
        d.max_objs = hip.PT_MAX_OBJS + 1
    elif case == "joints":
        d.num_joints = 9
    elif case == "misaligned":
        d.out_hm = 4096 + 4
    rc = L.cp_pose_targets(None, ctypes.byref(d), None, 0)
    assert rc == hip.CP_ERR_INVALID
    assert msg in L.cp_last_error().decode()


def test_python_refusals_and_packing():
    for name in ("tracking_task", "pre_hm", "pre_hm_hp", "tracking", "tracking_hp", "dense_hp", "mse_loss"):
        with pytest.raises(NotImplementedError, match=name):
            PoseTargets(PC.make_opt({name: True}))
    with pytest.raises(NotImplementedError, match="split"):
        PoseTargets(PC.make_opt(), split="val")
    with pytest.raises(NotImplementedError, match="debug"):
        PoseTargets(PC.make_opt(debug=1))
    rng = np.random.default_rng(0)
    anns = PC.synth_annotations(rng, [(None, "pose"), ("True", "pose"), (None, "pose"), ("False", "pose"),
                                      (None, "pose")], 640, 480)
    r = pack_annotations(anns, np.eye(2, 3), 640, 480, False, 0.0, PC.make_opt(c="chair"))
    assert r["pt_objects"][:5, 0].tolist() == [4, 4, 4, 1, 1]  # the reference's carry-over (:962-966)
    r = pack_annotations(anns, np.eye(2, 3), 640, 480, False, 0.0, PC.make_opt(c="bottle", num_symmetry=6))
    assert r["pt_objects"][:5, 0].tolist() == [6, 4, 4, 1, 1]
    with pytest.raises(ValueError, match="S = 1"):
        pack_annotations(anns, np.eye(2, 3), 640, 480, False, 0.0, PC.make_opt(c="camera"))
    many = PC.synth_annotations(rng, [(None, "pose")] * 13, 640, 480)
    r = pack_annotations(many, np.eye(2, 3), 640, 480, True, 5.0, PC.make_opt(c="camera"))
    assert r["pt_image"][hip.PT_IMG["num_objs"]] == 10 and r["pt_objects"].shape == (10, hip.PT_OBJ_STRIDE)
    assert r["pt_image"][hip.PT_IMG["flipped"]] == 1 and r["pt_image"][hip.PT_IMG["rot"]] == 5.0
