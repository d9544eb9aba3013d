"""GPU tests of the tracking task's training targets with the detector in the loop (cp_pose_targets_track_det,
TrackPoseTargets with a detector): the kernels on hand-made device detection records against the numpy restatement and
against the reference-built goldens, bit for bit; a batch that mixes the modes against cp_pose_targets_track; a repeated
call; and the whole chain -- detector, post-process, PnP, matching, targets -- on a synthetic dlav1_34 model against the
restatement fed with ObjectPoseDetector.run_batch's boxes, without a host synchronisation."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from centerpose_amd import hip, synth
from centerpose_amd.lib.utils.image import get_affine_transform
from centerpose_amd.pose_targets import num_symmetry
from centerpose_amd.pose_targets_track import TrackPoseTargets, draw_track_noise, pack_track_annotations, track_target_keys
from tests import pose_target_cases as PC
from tests import pose_target_track_cases as TC
from tests import pose_target_track_det_cases as DC
from tests import pose_targets_track_det_ref as DR
from tests import pose_targets_track_ref as TR

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(REPO, "tests", "golden", "pose_targets_track_det_ref.npz")
MAPS = ("hm", "hm_hp", "pre_hm", "pre_hm_hp")
RECORDS = ("pt_image", "pt_objects", "ptk_image", "ptk_pre_objects", "ptk_cur_objects", "ptk_gen", "ptk_det_meta")


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


class _NoModel:
    """Stands where the detector would: these tests hand the detections over themselves."""
    tracking_task = False

    def detect(self, *a, **k):
        raise AssertionError("the detector is not to be run here")


def targets_of(opt, max_pre_objs=None):
    return TrackPoseTargets(opt, max_pre_objs=max_pre_objs, detector=_NoModel())


def upload(rows, device):
    """[(post, count, pnp)] per image -> the device tensors of hip.postprocess / hip.pnp_from_post."""
    post = torch.from_numpy(np.stack([r[0] for r in rows])).to(device)
    count = torch.tensor([r[1] for r in rows], dtype=torch.int32, device=device)
    pnp = torch.from_numpy(np.stack([r[2] for r in rows])).to(device)
    return post, count, pnp


def restate(recs, rows, opt):
    boxes = [DC.boxes_of({k: v[b] for k, v in recs.items()}, *rows[b], opt) for b in range(len(rows))]
    return DR.batch_targets(recs, boxes, num_symmetry(opt), opt.output_res, TR.options(opt), DR.det_options(opt),
                            opt.use_absolute_scale)


def assert_same(out, want, keys, where=""):
    for k in keys:
        a, b = out[k].cpu().numpy(), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (where, k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (where, k)


def golden_arrays(gold, name, opt):
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


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_device_equals_goldens(device, gold, name):
    """Every event of the golden cases (tests/test_pose_targets_track_det_cpu.py lists them), against the reference's
    own arrays."""
    opt = DC.make_opt(DC.CASES[name]["over"])
    recs = {k: gold[name + "/" + k][None] for k in RECORDS}
    rows = [(gold[name + "/det_post"], int(gold[name + "/det_count"]), gold[name + "/det_pnp"])]
    out = targets_of(opt)(recs, detections=upload(rows, device))
    want = {k: v[None] for k, v in golden_arrays(gold, name, opt).items()}
    assert_same(out, want, track_target_keys(opt), name)


def small_opt(input_w, **over):
    o = dict(c="camera", input_res=128, input_w=input_w, input_h=128, output_res=32, render_hm_mode=1, render_hmhp_mode=0)
    o.update(over)
    return DC.make_opt(o)


def hand_made(seed, opt, counts, modes, Kp):
    """B = len(counts) images with K_det = 100 rows each, the first counts[b] of them detections."""
    rng = np.random.default_rng(seed)
    per = [DC.random_image(rng, opt, mode=m, n_slots=n, K=100, max_pre_objs=Kp) for n, m in zip(counts, modes)]
    return {k: np.stack([p[0][k] for p in per]) for k in per[0][0]}, [p[1] for p in per]


# both 64-lane passes and the ragged tail (37, 100), one and no detection; 10 and 64 previous-object slots; a rectangular input
SHAPES = [("sq_k10", 128, 10, (0, 1, 37), dict(render_hmhp_mode=0, tracking_label_mode=1)),
          ("rect_k64", 160, 64, (100, 37, 1), dict(render_hmhp_mode=2, tracking_label_mode=0)),
          ("sq_chair", 128, 10, (37, 100, 5), dict(c="chair", render_hmhp_mode=3, render_hm_mode=0, center_3D=True)),
          ("rect_hp1", 160, 10, (100, 0, 37), dict(render_hmhp_mode=1, tracking_label_mode=1, c="shoe"))]


@pytest.mark.parametrize("name, input_w, Kp, counts, over", SHAPES, ids=[s[0] for s in SHAPES])
def test_hand_made_records_equal_restatement(device, name, input_w, Kp, counts, over):
    opt = small_opt(input_w, **over)
    recs, rows = hand_made(41 + len(name), opt, counts, (1, 1, 1), Kp)
    assert [r[1] for r in rows] == list(counts) and rows[0][0].shape == (100, 120)
    t = targets_of(opt, max_pre_objs=Kp)
    out = t(recs, detections=upload(rows, device))
    want = restate(recs, rows, opt)
    assert sum(m is not None for ms in want["match"] for m in ms) >= 2  # the detections do land on objects
    assert_same(out, want, track_target_keys(opt), name)
    # a second call with the same inputs is bitwise identical
    again = t(recs, detections=upload(rows, device))
    for k in track_target_keys(opt):
        assert torch.equal(out[k], again[k]), k


def test_mixed_batch_equals_both_entry_points(device):
    """Modes (0, 1, 0): images 0 and 2 are exactly cp_pose_targets_track's, image 1 the restatement's mode 1."""
    opt = small_opt(128, render_hmhp_mode=2)
    recs, rows = hand_made(77, opt, (37, 37, 100), (0, 1, 0), 10)
    assert recs["ptk_gen"][:, 0].tolist() == [0, 1, 0]
    out = targets_of(opt)(recs, detections=upload(rows, device))
    plain = TrackPoseTargets(DC.make_opt(dict(vars(opt), data_generation_mode_ratio=0)))(
        {k: v for k, v in recs.items() if k not in ("ptk_gen", "ptk_det_meta")}, device=device)
    want = restate(recs, rows, opt)
    for k in track_target_keys(opt):
        for b in (0, 2):
            assert torch.equal(out[k][b], plain[k][b]), (k, b)
        assert not torch.equal(out["pre_hm_hp"][1], plain["pre_hm_hp"][1])
    assert_same(out, want, track_target_keys(opt))


def test_golden_mixed_batch(device, gold):
    opt = DC.make_opt(DC.CASES["plain_hp2"]["over"])
    names = ("plain_hp2@0", "plain_hp2", "plain_hp2@0")
    recs = {k: np.stack([gold[n + "/" + k] for n in names]) for k in RECORDS}
    rows = [(gold[n + "/det_post"], int(gold[n + "/det_count"]), gold[n + "/det_pnp"]) for n in names]
    out = targets_of(opt)(recs, detections=upload(rows, device))
    want = {k: np.stack([golden_arrays(gold, n, opt)[k] for n in names]) for k in track_target_keys(opt)}
    assert_same(out, want, track_target_keys(opt))


def test_refused_before_launch(device):
    opt = small_opt(128)
    recs, rows = hand_made(5, opt, (1,), (1,), 10)
    post, count, pnp = upload(rows, device)
    t = targets_of(opt)
    with pytest.raises(ValueError, match="float64"):
        t(recs, detections=(post.float(), count, pnp))
    with pytest.raises(ValueError, match="K_det must be"):
        t(recs, detections=(post.repeat(1, 2, 1)[:, :129].contiguous(), count, pnp.repeat(1, 2, 1)[:, :129].contiguous()))
    bad = dict(recs, ptk_gen=recs["ptk_gen"] * 2)
    with pytest.raises(ValueError, match="data generation mode 2"):
        t(bad, detections=(post, count, pnp))


def test_end_to_end_with_detector(device, tmp_path):
    """A seeded synthetic dlav1_34 detector, B = 2 at 128 x 128: TrackPoseTargets(opt, detector=model)(records, pre_img)
    against the restatement fed with ObjectPoseDetector.run_batch's boxes for the same images.  The annotations are the
    detector's own boxes moved by a few pixels, so matches occur.  run_batch and the targets read the same
    cp_postprocess / cp_pnp_from_post rows of the same decode, so every key is compared bit for bit."""
    from centerpose_amd.lib.detectors.detector_factory import detector_factory
    from centerpose_amd.lib.models.model import create_model, save_model
    from centerpose_amd.lib.opts import opts

    o = opts().parser.parse_args(["--arch", "dlav1_34", "--c", "cup", "--debug", "5", "--vis_thresh", "0.02"])
    o.obj_scale, o.use_pnp, o.rep_mode = True, True, 1
    o = opts().init(opts().parse(o))
    ck = os.path.join(str(tmp_path), "synthetic_dlav1_34.pth")
    m = create_model(o.arch, o.heads, o.head_conv, o)
    m.load_state_dict(synth.make_state_dict("dlav1_34", o.heads), strict=True)
    save_model(ck, 1, m)
    o.load_model = ck
    det = detector_factory[o.task](o)
    B, w, h = 2, 640, 480
    x = synth.frames(B, seed=21, h=128, w=128)
    c, s = np.array([w / 2.0, h / 2.0], np.float32), float(max(w, h))
    fx = 1.1 * w
    meta = {"c": c, "s": s, "out_height": 32, "out_width": 32, "width": w, "height": h, "inp_height": 128, "inp_width": 128,
            "camera_matrix": np.array([[fx, 0, w / 2.0], [0, fx, h / 2.0], [0, 0, 1.0]])}
    boxes = [r["boxes"] for r in det.run_batch(x, [dict(meta) for _ in range(B)])]
    assert sum(len(b) for b in boxes) >= 2, [len(b) for b in boxes]  # (an image without a box is a case of its own)
    opt = DC.make_opt(dict(c="cup", mug=False, num_symmetry=6, input_res=128, input_w=128, input_h=128, output_res=32,
                           render_hm_mode=1, render_hmhp_mode=2, tracking_label_mode=1, data_generation_mode_ratio=0.3))
    rng = np.random.default_rng(8)
    per = []
    for b in range(B):
        nb = min(len(boxes[b]), 6)
        n = max(nb, 2)
        anns = TC.name_objects(PC.synth_annotations(rng, [(None, "pose")] * n, w, h))
        pre = TC.previous_frame(rng, anns, [(k, None, False) for k in range(n)])
        for k in range(nb):  # the annotation of object k: box k of the detector, a few pixels off
            pts = np.asarray(boxes[b][k][0], np.float64) * [w, h] + rng.uniform(-3, 3, (9, 2))
            pre["objects"][k]["projected_cuboid"] = [[float(px), float(py)] for px, py in pts]
        pre["camera_data"]["intrinsics"] = {"fx": fx, "fy": fx, "cx": w / 2.0, "cy": h / 2.0}
        gen = dict(mode=1, c=c, s=s, aug_s=1.0, intrinsics=pre["camera_data"]["intrinsics"])
        per.append(pack_track_annotations(anns, pre, get_affine_transform(c, s, 0, [32, 32]),
                                          get_affine_transform(c, s, 0, [128, 128]), w, h, False, 0.0, opt,
                                          draw_track_noise(rng, n), generation=gen))
    recs = {k: np.stack([p[k] for p in per]) for k in per[0]}
    t = TrackPoseTargets(opt, detector=det.model, det_opt=det.opt)
    pre_img = x.to(device)
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        out = t(recs, pre_img=pre_img)  # the first call allocates and captures
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out2 = t(recs, pre_img=pre_img)  # no host synchronisation inside
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    want = DR.batch_targets(recs, boxes, num_symmetry(opt), opt.output_res, TR.options(opt), DR.det_options(opt))
    assert sum(mm is not None for ms in want["match"] for mm in ms) >= 2
    assert any(p["event"]["drawn"] for ps in want["pre"] for p in ps)
    assert_same(out, want, track_target_keys(opt), "first call")
    assert_same(out2, want, track_target_keys(opt), "replayed")
