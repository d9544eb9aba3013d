"""Seeding the device tracker from annotations and its ground-truth previous-frame maps (MI355X): cp_track_seed /
``DeviceTracker.seed`` against the host build of the same functions and the mirror's records, and
``BatchedTracking(..., device_tracker=True)`` in the reference's evaluation modes against the host tracker on the same
inputs and against tests/golden/track_run_seeded.json (the REFERENCE's own run(), tools/make_track_seed_goldens.py)."""
import contextlib
import copy
import io
import types

import numpy as np
import pytest
import torch

from centerpose_amd import hip
from centerpose_amd.lib.utils.image import draw_gaussian_records, get_affine_transform
from oracle.tools import make_goldens as mg
from oracle.tools import track_golden as tg
from tests import test_tracking_loop as ttl
from tests import track_seed_cases as sc
from tests.test_track_seed_cpu import (_gt_metas, _identity_vm, _params, _post_from_dict, _vm, gold, host,  # noqa: F401
                                       host_seed, mirror_gt_records, seeded_detector)

pytestmark = pytest.mark.gpu
B, K = 3, 100


def _raw(dt):
    """(hdr int32 [4 + 4 B], tracks [2, B, cap, STRIDE]) of the device state, without read()'s overflow check."""
    raw = dt.state.cpu().numpy()
    hdr = raw[: (4 + 4 * dt.B) * 4].view(np.int32).copy()
    return hdr, raw[dt.hdr_bytes:].view(np.float64).reshape(2, dt.B, dt.cap, hip.TRACK_STRIDE).copy()


def _posts(dets_per_video, device):
    post, cnt = np.zeros((B, K, hip.POST_STRIDE)), []
    for b, dets in enumerate(dets_per_video):
        for i, d in enumerate(dets):
            post[b, i] = _post_from_dict(d)
        cnt.append(len(dets))
    return torch.from_numpy(post).to(device), torch.tensor(cnt, dtype=torch.int32, device=device)


def test_device_seed_matches_host_build_and_leaves_others_alone(device, host):  # noqa: F811
    """Video 0 is seeded with the case list, video 1 holds tracks of an earlier frame and is passed over (count -1), video 2
    holds tracks and is reset (count 0)."""
    P = _params(mg.TrackOpt(False))
    dt = hip.DeviceTracker(B, P, np.stack([_identity_vm()] * B), device, 512, 512)
    frame = mg.tracker_frames()[0]
    dt.step(*_posts([[], frame, frame[:3]], device))
    hdr0, tr0 = _raw(dt)
    recs0 = dt.recs.cpu().numpy().copy()
    assert hdr0[4 + 4 * 1] > 0 and hdr0[4 + 4 * 2] > 0 and (recs0[1, :, :, 0] >= 0).any()
    given = sc.annotations(0)
    seeds, counts = hip.pack_seeds([given, None, []], P)
    assert counts.tolist() == [6, -1, 0]
    dt.seed(seeds, counts)
    lists = dt.read()
    want, want_recs, idc, _ = host_seed(host, P, _identity_vm(), seeds[0], gt=0, hm_plane=0, hp_plane0=B)
    assert len(lists[0]) == len(want) == 5
    for t, g in zip(lists[0], want):
        assert (int(t[0]), int(t[1]), int(t[2])) == (int(g[0]), 1, 1)
        np.testing.assert_allclose(t, g, rtol=1e-9, atol=1e-9)
    hdr1, tr1 = _raw(dt)
    recs1 = dt.recs.cpu().numpy()
    assert hdr1[4:7].tolist() == [5, idc, 0]
    np.testing.assert_allclose(recs1[0], want_recs, rtol=1e-9, atol=0)
    # video 1: list, header and records bit for bit as they were
    assert hdr1[0] == hdr0[0] and np.array_equal(hdr1[8:12], hdr0[8:12])
    assert tr1[:, 1].tobytes() == tr0[:, 1].tobytes() and recs1[1].tobytes() == recs0[1].tobytes()
    assert len(lists[1]) == hdr0[8] and lists[1].tobytes() == tr0[hdr0[0], 1, :hdr0[8]].tobytes()
    # video 2: empty, ids start again, nothing to draw
    assert len(lists[2]) == 0 and hdr1[12:15].tolist() == [0, 0, 0] and (recs1[2, :, :, 0] == -1).all()
    # a seeded list is a list like any other: the next frame continues it
    dt.step(*_posts([[], [], []], device))
    assert [len(a) for a in dt.read()] == [5, len(lists[1]), 0]


def test_device_seed_truncates_and_reports_overflow(device):
    P = _params(mg.TrackOpt(False), cap=4)
    dt = hip.DeviceTracker(B, P, np.stack([_identity_vm()] * B), device, 512, 512)
    a = sc.annotations(0)
    strong = [copy.deepcopy(a[i % 3]) for i in range(6)]
    for i, s in enumerate(strong):
        s["score"] = 0.4 + 0.05 * i
    seeds, counts = hip.pack_seeds([strong[:2] + [a[3]] + strong[2:], None, None], P)
    dt.seed(seeds, counts)
    assert dt.dropped() == [2, 0, 0]
    with pytest.raises(RuntimeError, match="more than cap"):
        dt.check()
    hdr, tr = _raw(dt)
    assert hdr[4:7].tolist() == [4, 4, 2]
    assert tr[hdr[0], 0, :4, 0].tolist() == [1, 2, 3, 4]
    np.testing.assert_allclose(tr[hdr[0], 0, :4, 4], [0.4, 0.45, 0.5, 0.55])


def test_device_seed_refuses_bad_arguments_before_the_state_moves(device):
    P = _params(mg.TrackOpt(False))
    dt = hip.DeviceTracker(B, P, np.stack([_identity_vm()] * B), device, 512, 512)
    seeds, counts = hip.pack_seeds([sc.annotations(0), None, None], P)
    dt.seed(seeds, counts)
    hdr0, tr0 = _raw(dt)
    for bad in (lambda: dt.seed(seeds[:2], counts[:2]), lambda: dt.seed(seeds[:, :, :100], counts),
                lambda: dt.seed(seeds, np.array([9, -1, -1], np.int32)), lambda: dt.seed(seeds, counts, [1, 0])):
        with pytest.raises(RuntimeError):
            bad()
    hdr1, tr1 = _raw(dt)
    assert np.array_equal(hdr0, hdr1) and tr0.tobytes() == tr1.tobytes()


def test_device_ground_truth_records_and_planes(device, monkeypatch):
    """``dt.recs`` after a ground-truth seeding == the mirror's ``_track_records`` in 'gt' mode, exactly (a frame with the
    identity crop, a cropped 640 x 480 frame, and a video whose maps are not the ground-truth ones); ``render()`` ==
    ``draw_gaussian_records`` of them, plane by plane, within the tolerances tests/test_tracking_loop._compare applies to the
    previous-frame maps (sum rtol 1e-5 / atol 1e-4, maximum rtol 1e-6, the same pixels non-zero)."""
    det = seeded_detector(monkeypatch, "-1", sc.MODES["gt_every"])
    P = _params(mg.TrackOpt(False), pre_thresh=0.5)
    m0, m1 = _gt_metas()
    metas = [m0, m1, m0]
    dt = hip.DeviceTracker(B, P, np.stack([_vm(m) for m in metas]), device, 512, 512)
    given = [sc.annotations(0), sc.annotations(1), sc.annotations(0)]
    given[0][0]["score"] = given[2][0]["score"] = 0.31   # a track; below pre_thresh, which the ground-truth branch does not apply
    seeds, counts = hip.pack_seeds(given, P, [True, True, False])
    dt.seed(seeds, counts, [True, True, False])
    recs = dt.recs.cpu().numpy()
    want = np.zeros((B, dt.cap, 9, 5))
    want[:, :, :, 0] = -1
    for b in (0, 1):
        det.tracker.init_track({"id": 0, "pre_dets": copy.deepcopy(given[b])})
        w = mirror_gt_records(det, det.tracker.tracks, metas[b])
        hm, hp = w[:, :1], w[:, 1:]
        hm[hm[:, :, 0] >= 0, 0] = b
        hp[hp[:, :, 0] >= 0, 0] += B + 8 * b - 1
        want[b, :len(w)] = w
    assert np.array_equal(recs[:2], want[:2])
    assert (recs[0, :5, 0, 0] == [0, 0, 0, 0, -1]).all() and recs[0, 3, 1:, 1].min() < 0 and recs[0, 3, 1:, 1].max() >= 512
    # video 2 is drawn from its tracks ('kps' mode here): pre_thresh applies, visible vertices only
    assert recs[2, 0, 0, 0] == -1 and recs[2, 1, 0, 0] == 2
    v = recs[2][recs[2, :, :, 0] >= 0]
    assert len(v) and (v[:, 1] >= 0).all() and (v[:, 1] < 512).all() and (v[:, 2] >= 0).all() and (v[:, 2] < 512).all()
    hm, hp = dt.render()
    planes = torch.cat([hm.reshape(B, 512, 512), hp.reshape(8 * B, 512, 512)]).cpu().numpy()
    ref = draw_gaussian_records([tuple(r) for r in recs.reshape(-1, 5) if r[0] >= 0], 9 * B, 512, 512)
    assert ref[:B + 16].max() == 1.0
    for c in range(9 * B):
        assert int((planes[c] > 0).sum()) == int((ref[c] > 0).sum()), c
        np.testing.assert_allclose(planes[c].astype(np.float64).sum(), ref[c].astype(np.float64).sum(), rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(planes[c].max(), ref[c].max(), rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
N_STEPS = 7   # video b sees frame (step + b) % 5: every video passes id 0 at another step, video 0 twice


class _RotatedEngine(object):
    """The stub network for B videos that are ``b`` frames apart."""

    def __init__(self, stub, device):
        self.stub, self.device, self.calls = stub, device, 0
        self.last_pre_hm = self.last_pre_hm_hp = None

    def forward(self, images, pre_images=None, pre_hms=None, pre_hm_hp=None, sigmoid_hm=True):
        assert images.shape[0] == B and (pre_images is None or pre_images.shape == images.shape)
        self.last_pre_hm = None if pre_hms is None else pre_hms.detach().cpu().clone()
        self.last_pre_hm_hp = None if pre_hm_hp is None else pre_hm_hp.detach().cpu().clone()
        out = {}
        for k in self.stub.frames[0]:
            v = torch.cat([self.stub.frames[(self.calls + b) % tg.N_FRAMES][k] for b in range(B)])
            out[k] = (torch.sigmoid(v) if (sigmoid_hm and k in ("hm", "hm_hp")) else v).contiguous().to(self.device)
        self.calls += 1
        return out


def _run_batched(det, device, mode, device_tracker):
    from centerpose_amd.lib.detectors.batch_tracking import BatchedTracking

    eng = _RotatedEngine(det.model, device)
    det.model._engine = lambda: eng
    bt = BatchedTracking(det, B, device_tracker=device_tracker)
    inputs = tg.frame_inputs(get_affine_transform)
    frames = [[] for _ in range(B)]
    with contextlib.redirect_stdout(io.StringIO()):
        for s in range(N_STEPS):
            ids = [(s + b) % tg.N_FRAMES for b in range(B)]
            images = torch.from_numpy(np.stack([inputs[f][0] for f in ids]))
            metas = []
            for f in ids:
                m = copy.deepcopy(inputs[f][1])
                seeds = sc.pre_dets_for(mode, f)
                if seeds is not None:
                    m["pre_dets"] = seeds
                metas.append(m)
            outs = bt.step(images, metas)
            for b in range(B):
                view = types.SimpleNamespace(model=types.SimpleNamespace(
                    last_pre_hm=None if eng.last_pre_hm is None else eng.last_pre_hm[b:b + 1],
                    last_pre_hm_hp=None if eng.last_pre_hm_hp is None else eng.last_pre_hm_hp[b:b + 1]))
                fr = tg.summarise({"results": outs[b]["results"], "boxes": outs[b]["boxes"]}, view)
                fr["keys"] = None   # run()'s timing keys are not part of a batched step
                frames[b].append(fr)
    return frames, bt


@pytest.mark.parametrize("mode,baseline", [("gt_first", False), ("gt_every", False), ("gt_first_empty", False),
                                           ("gt_first", True)])
def test_batched_tracking_seeded_device_matches_host_and_reference(device, monkeypatch, mode, baseline):
    """Three videos one frame apart, so that one is (re-)seeded at ``meta['id'] == 0`` while the others go on: every frame
    of every video on the device tracker == the host tracker on the same inputs, and == the reference's own run() from the
    step at which the video was last seeded (TRACK_ARGV modes; there is no reference run of the baseline mode)."""
    det = seeded_detector(monkeypatch, "0", sc.MODES[mode], baseline)
    assert type(det.tracker).__name__ == ("Tracker_baseline" if baseline else "Tracker")
    dev_frames, bt = _run_batched(det, device, mode, True)
    host_frames, _ = _run_batched(det, device, mode, False)
    assert bt.dev is not None and bt.times["steps"] == N_STEPS
    for b in range(B):
        ttl._compare(dev_frames[b], host_frames[b])
    if baseline:
        return
    g, n_gold = gold(mode), 0
    for b in range(B):
        seeded = False
        for s in range(N_STEPS):
            f = (s + b) % tg.N_FRAMES
            seeded = seeded or f == 0
            if seeded:   # (with --gt_pre_hm_hmhp every frame is re-seeded, but frame f > 0 of an unseeded start has other ids)
                ttl._compare([dev_frames[b][s]], [dict(g[f], keys=None)])
                n_gold += 1
    assert n_gold == 7 + 3 + 4
    if mode == "gt_first_empty":
        assert all(fr["pre_hm_sum"] == 0 for v in dev_frames for fr in v)
    else:
        assert dev_frames[1][4]["pre_hm_hp_nonzero"] == g[0]["pre_hm_hp_nonzero"] > 0   # video 1 seeded at step 4


@pytest.mark.parametrize("config", ["refined_kalman_only", "no_previous_maps"])
def test_batched_tracking_seeded_without_previous_maps(device, monkeypatch, config):
    """The two evaluation modes of the reference's benchmark that seed the tracker but feed the network no previous-frame
    maps (shell_eval_video_CenterPoseTrack.py MODE_1: --refined_Kalman without the tracking task, MODE_7: the tracking task
    without pre_hm / pre_hm_hp), both with --gt_pre_hm_hmhp_first: device tracker == host tracker, frame by frame."""
    from centerpose_amd.lib.utils.tracker import Tracker_baseline

    det = seeded_detector(monkeypatch, "0", sc.MODES["gt_first"])
    if config == "refined_kalman_only":
        det.opt.tracking_task, det.opt.refined_Kalman = False, True
        det.tracker = Tracker_baseline(det.opt)
    det.opt.pre_hm = det.opt.pre_hm_hp = False
    dev_frames, bt = _run_batched(det, device, "gt_first", True)
    host_frames, _ = _run_batched(det, device, "gt_first", False)
    assert [t["tracking_id"] for t in dev_frames[0][0]["tracks"]] == [1, 2, 3, 4, 5]
    assert bt.dev.P.baseline == (config == "refined_kalman_only")
    maps = ("pre_hm_sum", "pre_hm_max", "pre_hm_hp_sum", "pre_hm_hp_nonzero")
    for b in range(B):
        for fr in dev_frames[b] + host_frames[b]:
            assert all(fr[k] is None for k in maps)   # the network was fed no previous-frame maps ...
            fr.update({k: 0 for k in maps})           # ... so there is none to compare
        ttl._compare(dev_frames[b], host_frames[b])


def test_batched_tracking_refuses_what_the_host_tracker_cannot_do(device, monkeypatch):
    """Ground-truth maps due without 'pre_dets', and seeds drawn by the branch that reads the filter read-out: RuntimeError
    naming the key, before the device state and the loop's own view of the frame move."""
    from centerpose_amd.lib.detectors.batch_tracking import BatchedTracking

    det = seeded_detector(monkeypatch, "0", sc.MODES["gt_first"])
    eng = _RotatedEngine(det.model, device)
    det.model._engine = lambda: eng
    bt = BatchedTracking(det, B, device_tracker=True)
    img, meta = tg.frame_inputs(get_affine_transform)[0]
    images = torch.from_numpy(np.stack([img] * B))
    with contextlib.redirect_stdout(io.StringIO()):
        bt.step(images, [dict(copy.deepcopy(meta), pre_dets=sc.annotations(0)) for _ in range(B)])
        hdr0, tr0 = _raw(bt.dev)
        recs0, pre0, calls0 = bt.dev.recs.cpu().numpy().copy(), bt.pre_images, eng.calls
        metas = [dict(copy.deepcopy(meta), pre_dets=sc.annotations(0)) for _ in range(B)]
        del metas[1]["pre_dets"]
        with pytest.raises(RuntimeError, match="pre_dets.*host tracker"):
            bt.step(images, metas)
    hdr1, tr1 = _raw(bt.dev)
    assert np.array_equal(hdr0, hdr1) and tr0.tobytes() == tr1.tobytes() and bt.dev.recs.cpu().numpy().tobytes() == recs0.tobytes()
    assert bt.frames == 1 and bt.pre_images is pre0 and eng.calls == calls0
    assert [len(a) for a in bt.dev.read()] == [5] * B
    # no ground-truth flag: the first frame's seeds would be drawn from 'kps_mean_kf' / 'kps_pnp_kf'
    det2 = seeded_detector(monkeypatch, "0", [])
    det2.model._engine = lambda: eng
    bt2 = BatchedTracking(det2, B, device_tracker=True)
    with pytest.raises(RuntimeError, match="kps_mean_kf.*host tracker"):
        bt2.step(images, [dict(copy.deepcopy(meta), pre_dets=sc.annotations(0)) for _ in range(B)])
    assert bt2.dev is None and bt2.pre_images is None and bt2.frames == 0
