"""The overlay on the device: cp_draw_primitives against tests/draw_ref.py bit for bit on the whole pitched buffer (pad bytes
and uncovered pixels included), independence of the images of a batch and reproducibility, the two device list builders
against the mirror's ``Debugger`` fed with the same records read back, and the end-to-end paths: ``--debug 4`` writes the
reference's file, ``run_batch(..., draw=frames)`` draws without changing the records."""
import os

import numpy as np
import pytest
import torch

from centerpose_amd import hip
from centerpose_amd.hip import draw as hd
from tests import draw_cases as dc
from tests import draw_ref, scene

pytestmark = pytest.mark.gpu


def _device_draw(device, buf, b, h, w, pitch, prims):
    """``buf`` (pitched uint8 [b * h * pitch]) with ``prims`` drawn by the device; the frames are a strided view of the buffer."""
    t = torch.from_numpy(np.array(buf, np.uint8)).to(device)
    frames = t.as_strided((b, h, w, 3), (h * pitch, pitch, 3, 1))
    hd.draw_primitives(frames, torch.from_numpy(np.ascontiguousarray(prims, np.int32)).to(device))
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def drawn(device):
    """Every case once: name -> (background, prims, the oracle's buffer, the device's buffer)."""
    out = {}
    for name, fn in (("edge", dc.edge_case), ("order", dc.order_case), ("many", dc.many_case)):
        prims, bg = fn(), dc.background()
        out[name] = (bg, prims, draw_ref.draw_pitched(bg, dc.B, dc.H, dc.W, dc.PITCH, prims),
                     _device_draw(device, bg, dc.B, dc.H, dc.W, dc.PITCH, prims))
    return out


@pytest.mark.parametrize("case", ["edge", "order", "many"])
def test_primitives(drawn, case):
    bg, prims, want, got = drawn[case]
    assert not np.array_equal(want, bg)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing bytes (offset -> image, row, byte): %s" % [
        (int(o), int(o // (dc.H * dc.PITCH)), int(o // dc.PITCH % dc.H), int(o % dc.PITCH)) for o in bad[:8]]
    if case == "many":
        assert np.array_equal(got.reshape(dc.B, -1)[0], bg.reshape(dc.B, -1)[0])   # the image without a primitive


def test_a_one_pixel_frame(device):
    prims, h, w, pitch = dc.tiny_case()
    bg = np.array([9, 8, 7], np.uint8)
    assert np.array_equal(_device_draw(device, bg, 1, h, w, pitch, prims), draw_ref.draw_pitched(bg, 1, h, w, pitch, prims))


@pytest.mark.parametrize("case", ["edge", "many"])
def test_an_image_alone_equals_the_image_in_the_batch_and_runs_repeat(device, drawn, case):
    bg, prims, _, got = drawn[case]
    n = dc.H * dc.PITCH
    for b in range(dc.B):
        alone = _device_draw(device, bg[b * n:(b + 1) * n], 1, dc.H, dc.W, dc.PITCH, prims[b:b + 1])
        assert np.array_equal(alone, got[b * n:(b + 1) * n]), b
    assert np.array_equal(_device_draw(device, bg, dc.B, dc.H, dc.W, dc.PITCH, prims), got)


def test_contiguous_frames_and_own_workspace(device):
    """Packed rows (pitch = 3 W, every row of image 0 dword aligned) and a caller's workspace: the same pixels."""
    prims = dc.edge_case()
    bg = dc.background(pitch=3 * dc.W, seed=8)
    frames = torch.from_numpy(bg).to(device).view(dc.B, dc.H, dc.W, 3)
    ws = torch.empty(hd.workspace_bytes(dc.B, prims.shape[1]), dtype=torch.uint8, device=device)
    hd.draw_primitives(frames, torch.from_numpy(prims).to(device), ws=ws)
    assert np.array_equal(frames.cpu().numpy().reshape(-1), draw_ref.draw_pitched(bg, dc.B, dc.H, dc.W, 3 * dc.W, prims))
    with pytest.raises(ValueError, match="workspace too small"):
        hd.draw_primitives(frames, torch.from_numpy(prims).to(device), ws=ws[:-16])


CONFIGS = [dict(), dict(show_axes=True), dict(paper_display=True), dict(debugger_theme='black', show_axes=True)]


@pytest.mark.parametrize("fields", CONFIGS)
@pytest.mark.parametrize("counts", [None, (0, 8)])
def test_builders_detections(device, fields, counts):
    """cp_draw_detections read back against the list the ``Debugger`` path builds from the same records as result dicts."""
    post, count, pnp, cam = dc.synthetic_records()
    if counts is not None:
        count = np.array(counts, np.int32)
    w, h = dc.W * 4, dc.H * 4
    show_axes = bool(fields.get("show_axes"))
    params = hd.draw_params(None, width=w, height=h, vis_thresh=dc.VIS, theme=int(fields.get("debugger_theme", "white") == "white"),
                            show_axes=int(show_axes), paper_display=int(bool(fields.get("paper_display"))))
    dev = lambda a: torch.from_numpy(a).to(device)
    out = torch.full((2, 8 * hip._structs.DRAW_SLOTS, 8), -7, dtype=torch.int32, device=device)
    got = hd.draw_detections(dev(post), dev(count), dev(pnp), cam, params, out=out).cpu().numpy()
    dicts = dc.record_dicts(post, count, pnp, w, h, show_axes)
    S = hip._structs.DRAW_SLOTS
    for b in range(2):
        assert dc.slots_drawn(got[b]) == [tuple(p) for p in dc.debugger_prims(dicts[b], h, w, cam[b], **fields)], b
        assert not got[b, int(count[b]) * S:].any()       # the slots of absent records are cleared, not left as they were
    assert sum(len(dc.slots_drawn(g)) for g in got) > 50
    # without poses there are no cuboids; without intrinsics no axes
    bare = hd.draw_detections(dev(post), dev(count), None, None, params).cpu().numpy()
    assert {p[0] for p in dc.slots_drawn(bare)} <= {dc.RECT}
    no_cam = hd.draw_detections(dev(post), dev(count), dev(pnp), None, params).cpu().numpy()
    assert not no_cam.reshape(2, 8, S, 8)[:, :, hip._structs.DRAW_SLOT["axes"]:].any()


META = {"c": np.array([256.0, 256.0], np.float32), "s": 512.0, "out_height": 128, "out_width": 128, "width": 512,
        "height": 512, "inp_height": 512, "inp_width": 512, "camera_matrix": scene.K_DEMO}


def _stub_detector(device, tmp_path, B, extra=()):
    """The pose-chain tests' detector with the engine's forward replaced by heads rendered from known cuboid poses."""
    from tests.test_gpu_pose_chain import _detector

    det = _detector(tmp_path, extra=list(extra))
    det.opt.show_axes = True
    det.opt.cam_intrinsic = scene.K_DEMO
    heads, scenes = scene.render(B, 2, seed=77)
    g = {k: torch.from_numpy(v).to(device) for k, v in heads.items()}

    class Stub(object):
        sel = slice(0, B)

        def forward(self, images, *a, **kw):
            return {k: v[Stub.sel].contiguous().clone() for k, v in g.items()}

    det.model._engine = lambda: Stub()
    return det, Stub


def test_builders_tracks(device, tmp_path):
    """cp_draw_tracks on a two-frame cp_track_step state of two videos against the ``Debugger`` path on the tracks read back;
    with ``labels`` the 'ID:<n>' rectangle and glyphs equal the host-built ones."""
    from centerpose_amd.lib.utils.image import get_affine_transform

    B = 2
    det, _ = _stub_detector(device, tmp_path, B)
    metas = [dict(META, trans_input=get_affine_transform(META["c"], META["s"], 0, [512, 512])) for _ in range(B)]
    o = det.opt
    P = hip.TrackParams(new_thresh=0.3, pre_thresh=0.3, R=o.R, conf_lo=30, conf_hi=90, max_age=o.max_age, kalman=1, scale_pool=0,
                        use_pnp=1, hps_uncertainty=int(bool(o.hps_uncertainty)), show_axes=1, cat_rule=0, render_hm_mode=1,
                        render_hmhp_mode=2, pre_hm=1, pre_hm_hp=1, K=o.K, cap=16, hungarian=0, baseline=0)
    # (conf_lo / conf_hi: wide enough that the rendered heads' fused std, which has no uncertainty head behind it, still gives
    # vertex confidences above the 0.25 that puts a track into `boxes`; no scale pool: the rendered heads have no scale
    # uncertainty to weigh its samples with)
    dt = hip.DeviceTracker(B, P, hip.track_vmeta(metas), device, 512, 512)
    det._skip_host_dets = True
    try:
        det.process(torch.zeros(B, 3, 512, 512, device=device), None, None, None, None)
    finally:
        det._skip_host_dets = False
    rec, cnt, poses = det.post_pnp_device(metas)
    dt.step(rec, cnt, poses)
    dt.step(rec, cnt, poses)
    lists = dt.read()
    cam = hd.cam_rows(metas)
    n_label = 0
    for labels in (False, True):
        params = hd.draw_params(o, width=512, height=512, labels=labels, tracking_task=1, show_axes=1)
        got = hd.draw_tracks(dt.state, B, dt.cap, cam, params).cpu().numpy()
        for b in range(B):
            tracks = [hip.track_record_to_dict(r) for r in lists[b]]
            shown = [t for t in tracks if t["in_boxes"]]
            assert len(shown) >= 1, [(t['tracking_id'], t['age'], int(r[3]), list(r[447:455])) for t, r in zip(tracks, lists[b])]
            want = dc.debugger_prims(shown, 512, 512, cam[b], labels=labels, vis_thresh=o.vis_thresh, tracking_task=True,
                                     show_axes=True, debugger_theme=o.debugger_theme)
            assert dc.slots_drawn(got[b]) == [tuple(p) for p in want], (labels, b)
            n_label += sum(p[0] == dc.GLYPH for p in want)
            assert any(p[0] == dc.SEG and p[5] == 5 for p in want)   # the axes of kps_3d_cam_kf
    assert n_label >= 2 * len("ID:1")


def test_end_to_end_debug_4_and_run_batch_draw(device, tmp_path, monkeypatch):
    from PIL import Image

    from centerpose_amd.lib.utils import debugger as dbg_mod

    B = 2
    det, Stub = _stub_detector(device, tmp_path, B)
    o = det.opt
    o.debug = 4
    # ---- run(path) with --debug 4: the PNG under the reference's file name, equal to the oracle on the Debugger's list ----
    frame = np.random.RandomState(4).randint(0, 256, (512, 512, 3)).astype(np.uint8)
    path = os.path.join(str(tmp_path), "00003.png")
    Image.fromarray(frame[:, :, ::-1]).save(path)
    o.demo, o.demo_save = path, os.path.join(str(tmp_path), "out")
    made = []

    Base = dbg_mod.Debugger

    class Recording(Base):
        def __init__(self, *a, **k):
            Base.__init__(self, *a, **k)
            made.append(self)

    monkeypatch.setattr(dbg_mod, "Debugger", Recording)
    Stub.sel = slice(0, 1)
    ret = det.run(path, meta_inp={"camera_matrix": scene.K_DEMO})
    assert len(made) == 1 and made[0].device.type == "cuda" and len(ret["results"]) >= 2
    png = os.path.join(o.demo_save, "00003", "00003_out_img_pred.png")
    assert os.path.exists(png) and os.path.exists(os.path.join(o.demo_save, "00003", "00003.json"))
    got = np.asarray(Image.open(png).convert("RGB"))[:, :, ::-1]
    prims = made[0].primitives("out_img_pred")
    kinds = {p[0] for p in prims}
    assert {dc.RECT, dc.FILL, dc.GLYPH, dc.DISC, dc.SEG} <= kinds and any(p[0] == dc.SEG and p[5] == 5 for p in prims)
    want = draw_ref.draw_image(frame.copy(), prims)
    assert np.array_equal(got, want) and not np.array_equal(want, frame)

    # ---- run_batch(..., draw=frames): frames drawn on the device, records as without ----
    Stub.sel = slice(0, B)
    x = torch.zeros(B, 3, 512, 512)
    metas = [dict(META) for _ in range(B)]
    def records():
        """The records of the last run_batch, bit for bit: the counts and, per image, its count[b] post-processed and PnP rows
        as int64 words (rows past the count are no records: cp_postprocess never writes them)."""
        cnt = det.post_dev[1].clone()
        n = [int(v) for v in cnt.cpu()]
        return cnt, [det.post_dev[0][b, :n[b]].clone().view(torch.int64) for b in range(B)], \
            [det.pnp_dev[b, :n[b]].clone().view(torch.int64) for b in range(B)]

    det.run_batch(x, metas)
    cnt0, rec0, pnp0 = records()
    assert min(int(v) for v in cnt0.cpu()) >= 2
    bg = np.random.RandomState(6).randint(0, 256, (B, 512, 512, 3)).astype(np.uint8)
    frames = torch.from_numpy(bg).to(device)
    outs = det.run_batch(x, metas, draw=frames)
    cnt1, rec1, pnp1 = records()
    assert torch.equal(cnt1, cnt0)
    assert all(torch.equal(a, b) for a, b in zip(rec1, rec0)) and all(torch.equal(a, b) for a, b in zip(pnp1, pnp0))
    drawn = frames.cpu().numpy()
    for b in range(B):
        lst = dc.debugger_prims(list(outs[b]["results"]), 512, 512, hd.cam_rows(metas)[b], vis_thresh=o.vis_thresh, show_axes=True,
                                debugger_theme=o.debugger_theme)
        assert len(lst) >= 40   # more than one object's box, vertices, edges, crosses and axes
        assert np.array_equal(drawn[b], draw_ref.draw_image(bg[b].copy(), lst)), b
    with pytest.raises(RuntimeError, match="draw"):
        hd.draw_primitives(frames.cpu(), torch.zeros(B, 1, 8, dtype=torch.int32, device=device))
