"""The device tracker and the device post-process on non-finite detections (MI355X): cp_track_step and cp_postprocess on
the inputs of tests/track_poison_cases.py, against the host build of the same source, which tests/
test_track_nonfinite_cpu.py pins to the oracles and to the Python mirrors.

These tests are legitimate because trk_munkres bounds every loop by the algorithm's own structure (track_common.h): the
association kernel terminates whatever a frame holds.  What they add on the device: one video's bad frame does not touch its
neighbours in the batch, nothing is dropped, and nothing non-finite reaches cp_render_gaussians.
"""
import numpy as np
import pytest
import torch

from centerpose_amd import hip
from oracle.tools import make_goldens as mg
from tests import track_poison_cases as pc
from tests.test_post_logic_cpu import _run as _post_run
from tests.test_post_logic_cpu import host as post_host  # noqa: F401
from tests.test_track_logic_cpu import TR, HostTracker, _post_from_dict, host  # noqa: F401
from tests.track_poison_driver import track_params, video_meta

B, K, BAD = 3, 100, 1   # three videos one frame apart (test_device_tracker_matches_reference_tracker_golden); video 1 is poisoned


def _posts(frames):
    return [np.stack([_post_from_dict(d, True) for d in dets]) if dets else np.zeros((0, hip.POST_STRIDE)) for dets in frames]


def _device_run(device, mode, videos):
    """`videos`: per video its frames' post arrays.  -> (per step: lists [B], render records [B, cap, 9, 5], planes
    [9 B, 512, 512]), with video b lagging b frames behind and idle outside its sequence."""
    P = track_params(mode, {"cap": hip.TRACK_CAP})
    dt = hip.DeviceTracker(B, P, np.stack([video_meta()] * B), device, 512, 512)
    n_frames = len(videos[0])
    out = []
    for f in range(n_frames + B - 1):
        post, cnt = np.zeros((B, K, hip.POST_STRIDE)), np.zeros(B, np.int32)
        for b in range(B):
            if 0 <= f - b < n_frames:
                p = videos[b][f - b]
                post[b, :len(p)], cnt[b] = p, len(p)
        dt.step(torch.from_numpy(post).to(device), torch.from_numpy(cnt).to(device))
        recs = dt.recs.cpu().numpy().copy()
        dt.render()
        planes = dt.planes.cpu().clone()
        out.append((dt.read(), recs, planes))
    assert dt.dropped() == [0] * B      # cp_track_status: no list entry was dropped
    return out


def _host_run(L, mode, posts):
    ht = HostTracker(L, track_params(mode), video_meta())
    return [ht.step(p) for p in posts]


def _assert_records_drawable(recs, what):
    r = np.asarray(recs).reshape(-1, 5)
    r = r[r[:, 0] != -1]
    assert np.isfinite(r).all(), what
    assert (r[:, 0] >= 0).all() and (r[:, 0] < 9 * B).all(), what
    assert ((r[:, 1] >= 0) & (r[:, 1] < 512) & (r[:, 2] >= 0) & (r[:, 2] < 512) & (r[:, 3] >= 0) & (r[:, 3] <= 512)).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("mode", pc.GPU_MODES)
def test_device_tracker_on_poisoned_videos(device, host, mode):  # noqa: F811
    """cp_track_step with exactly one of three videos poisoned, every association-poison and payload-poison case of
    tests/track_poison_cases.py.  The two clean videos are bit-identical to the same batch without the poison -- lists,
    render records and drawn planes; the poisoned video's lists are the host build's (ids, age, active exact, the filter
    read-out to rtol 1e-9, the scale pool to 1e-6: the tolerances of test_device_tracker_matches_reference_tracker_golden;
    under payload poison the poisoned track's own filter is left unspecified); cp_track_status reports nothing dropped;
    every render record is channel -1 or finite and inside the input, and what cp_render_gaussians draws is finite."""
    frames = mg.tracker_mode(mode)[0]
    clean_posts = _posts(frames)
    clean = _device_run(device, mode, [clean_posts] * B)
    cases = [("assoc/" + name, pc.assoc_video(frames, keys, value, position)[0], None)
             for name, keys, value, position in pc.assoc_cases()]
    pf, pi = pc.PAYLOAD_AT
    own_score = float(frames[pf][pi]["score"])
    cases += [("payload/%s-%s" % (key, vname), pc.poisoned(frames, [pc.PAYLOAD_AT], (key,), value), own_score)
              for key, vname, value in pc.PAYLOAD_CASES]
    for name, bad_frames, own in cases:
        bad_posts = _posts(bad_frames)
        got = _device_run(device, mode, [bad_posts if b == BAD else clean_posts for b in range(B)])
        want = _host_run(host, mode, bad_posts)
        own_ids = set()
        for f, ((lists, recs, planes), (c_lists, c_recs, c_planes)) in enumerate(zip(got, clean)):
            what = (mode, name, f)
            for b in range(B):
                if b == BAD:
                    continue
                assert torch.equal(torch.from_numpy(lists[b]), torch.from_numpy(c_lists[b])), what
                assert recs[b].tobytes() == c_recs[b].tobytes(), what
                sel = [b] + list(range(B + 8 * b, B + 8 * b + 8))
                assert torch.equal(planes[sel], c_planes[sel]), what
            _assert_records_drawable(recs, what)
            assert bool(torch.isfinite(planes).all()), what
            if not 0 <= f - BAD < len(frames):
                continue
            mine, (theirs, _) = lists[BAD], want[f - BAD]
            assert len(mine) == len(theirs), what
            for t, g in zip(mine, theirs):
                assert (int(t[0]), int(t[1]), int(t[2])) == (int(g[0]), int(g[1]), int(g[2])), what
                if own is not None and (float(g[TR["POST"]]) == own or int(g[0]) in own_ids):
                    own_ids.add(int(g[0]))   # the poisoned track, here and while it is matched or coasts
                    continue
                np.testing.assert_allclose(t[TR["POST"] + 28:TR["POST"] + 30], g[TR["POST"] + 28:TR["POST"] + 30], rtol=1e-12)
                np.testing.assert_allclose(t[409:441], g[409:441], rtol=1e-9, atol=1e-9, err_msg=str(what))
                np.testing.assert_allclose(t[441:447], g[441:447], rtol=1e-6, atol=1e-12, err_msg=str(what))


@pytest.mark.gpu
@pytest.mark.parametrize("nms", [True, False])
def test_device_postprocess_on_non_finite_scores_and_boxes(device, post_host, nms):  # noqa: F811
    """cp_postprocess, B = 2, K = 8: image 0 holds the poisoned records of tests/track_poison_cases.py, image 1 the clean
    ones.  Counts and records equal the host build's (rtol 1e-9, the tolerance of the device post-process against its
    golden), and the clean image does not notice its neighbour."""
    from centerpose_amd.lib.utils.image import get_affine_transform

    dets, metas = mg.host_cases()
    meta = np.zeros((2, 8))
    for b, m in enumerate(metas):
        meta[b, :6] = get_affine_transform(m["c"], m["s"], 0, (m["out_width"], m["out_height"]), inv=1).reshape(-1)
        meta[b, 6] = m["s"] / max(m["out_width"], m["out_height"])
    thr = mg.HostOpt.vis_thresh
    clean1 = pc.post_inputs(dets, 1, None)[1]
    want1 = _post_run(post_host, clean1, meta[1], thr, nms)
    for case in [None] + sorted(pc.POST_CASES):
        raw0 = pc.post_inputs(dets, 0, case)[1]
        raw = np.stack([raw0, clean1])
        rec, cnt = hip.postprocess(torch.from_numpy(raw).to(device), meta, thr, nms=nms)
        rec, cnt = rec.cpu().numpy(), cnt.cpu().numpy()
        want0 = _post_run(post_host, raw0, meta[0], thr, nms)
        for b, want in ((0, want0), (1, want1)):
            assert int(cnt[b]) == len(want), (case, b, int(cnt[b]), len(want))
            np.testing.assert_allclose(rec[b, :len(want)], want, rtol=1e-9, atol=1e-9, err_msg=str((case, b)))
        if case is None:
            first1 = rec[1, :int(cnt[1])].copy()
        assert rec[1, :int(cnt[1])].tobytes() == first1.tobytes(), case
