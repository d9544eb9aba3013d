"""The overlay without a device: the host build of centerpose_amd/csrc/draw_common.h (tests/native/draw_host.cpp) and the numpy
path of the package against tests/draw_ref.py on the case list, the segment rule against float64 geometry, the font, the
refusals of cp_draw_primitives, the per-record lists against the mirror's ``Debugger``, and that ``Debugger`` against the
reference's own sequence of drawing calls (tests/golden/draw_calls.json, tools/make_draw_goldens.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

from centerpose_amd import hip
from centerpose_amd.hip import draw as hd
from tests import draw_cases as dc
from tests import draw_ref

REPO = dc.REPO


@pytest.fixture(scope="module")
def host():
    return dc.host_lib()


@pytest.mark.parametrize("case", ["edge", "order", "many"])
def test_host_build_and_numpy_path_equal_the_oracle(host, case):
    prims = {"edge": dc.edge_case, "order": dc.order_case, "many": dc.many_case}[case]()
    bg = dc.background()
    want = draw_ref.draw_pitched(bg, dc.B, dc.H, dc.W, dc.PITCH, prims)
    assert not np.array_equal(want, bg)
    got = dc.host_draw(host, bg, dc.B, dc.H, dc.W, dc.PITCH, prims)
    assert np.array_equal(got, want)
    pad = want.reshape(dc.B, dc.H, dc.PITCH)[:, :, 3 * dc.W:]
    assert np.array_equal(pad, bg.reshape(dc.B, dc.H, dc.PITCH)[:, :, 3 * dc.W:])
    if case == "many":
        assert np.array_equal(want.reshape(dc.B, -1)[0], bg.reshape(dc.B, -1)[0])   # image 0 has no primitive
    for b in range(dc.B):   # the package's numpy path (frames that are not on a device)
        img = bg.reshape(dc.B, dc.H, dc.PITCH)[b, :, :3 * dc.W].reshape(dc.H, dc.W, 3).copy()
        hd.rasterize_host(img, prims[b])
        assert np.array_equal(img, want.reshape(dc.B, dc.H, dc.PITCH)[b, :, :3 * dc.W].reshape(dc.H, dc.W, 3))


def test_a_one_pixel_frame(host):
    prims, h, w, pitch = dc.tiny_case()
    bg = np.array([9, 8, 7], np.uint8)
    want = draw_ref.draw_pitched(bg, 1, h, w, pitch, prims)
    # the far disc misses, the fill covers, the segment through (0, 0) covers after it; the radius-0 disc at (1, 0) and the empty
    # corner of the glyph's bitmap miss: the segment's colour stays
    assert want.tolist() == [0x66, 0x55, 0x44]
    assert np.array_equal(dc.host_draw(host, bg, 1, h, w, pitch, prims), want)


def test_painters_order(host):
    prims = dc.order_case()
    bg = np.zeros(dc.B * dc.H * dc.PITCH, np.uint8)
    out = dc.host_draw(host, bg, dc.B, dc.H, dc.W, dc.PITCH, prims).reshape(dc.B, dc.H, dc.PITCH)
    px = lambda b, x, y: tuple(out[b, y, 3 * x:3 * x + 3])
    assert px(0, 60, 21) == (0, 0, 255) and px(1, 60, 21) == (255, 0, 0)   # all three cover (60, 21): the last one wins
    assert not np.array_equal(out[0], out[1])


def test_segment_rule_against_float64_distance(host):
    """Every ordered pair of the endpoint set (zero-length included), every t in 1..16, every pixel of a 40 x 40 grid: covered
    iff 4 dist^2 <= t^2 in float64, where the float64 margin |4 dist^2 - t^2| is at least 1e-9 (the other points are exact ties
    or too close to call in floating point; the integer rule decides them, and they are under 1 % of the grid points)."""
    pts = [(5, 7), (30, 12), (18, 35), (-6, 20), (44, 3), (21, 22)]
    G = 40
    cases = [(a, b, t) for a in pts for b in pts for t in range(1, 17)]
    prims = np.zeros((len(cases), 1, 8), np.int32)
    for i, (a, b, t) in enumerate(cases):
        prims[i, 0] = (dc.SEG, a[0], a[1], b[0], b[1], t, 0xFFFFFF, 0)
    got = dc.host_draw(host, np.zeros(len(cases) * G * G * 3, np.uint8), len(cases), G, G, 3 * G, prims)
    got = got.reshape(len(cases), G, G, 3)[..., 0] == 255
    Y, X = np.mgrid[0:G, 0:G].astype(np.float64)
    excluded = wrong = 0
    for i, (a, b, t) in enumerate(cases):
        dx, dy = float(b[0] - a[0]), float(b[1] - a[1])
        L2 = dx * dx + dy * dy
        u = np.clip(((X - a[0]) * dx + (Y - a[1]) * dy) / L2, 0.0, 1.0) if L2 > 0 else np.zeros_like(X)
        d2 = (X - (a[0] + u * dx)) ** 2 + (Y - (a[1] + u * dy)) ** 2
        margin = 4 * d2 - t * t
        sure = np.abs(margin) >= 1e-9
        excluded += int((~sure).sum())
        wrong += int(((margin <= 0) != got[i])[sure].sum())
    share = excluded / float(len(cases) * G * G)
    print("segment rule: %d cases, %d grid points, excluded share %.5f, wrong %d" % (len(cases), len(cases) * G * G, share, wrong))
    assert share < 0.01
    assert wrong == 0


def test_font_and_text_layout(host):
    for code in range(-3, 300):
        assert host.cp_draw_host_glyph(code) == hd.glyph_bits(code), code
    for ch in hd.REQUIRED_CHARS:
        bits = hd.glyph_bits(ord(ch))
        assert 0 <= bits < 1 << 35                      # inside the 5 x 7 cell
        assert (bits != 0) == (ch != " "), ch           # the space only advances the pen
    drawn = set(hd.FONT)
    assert set(hd.REQUIRED_CHARS) - {" "} <= drawn
    assert all(hd.glyph_bits(c) == 0 for c in range(256) if chr(c) not in drawn)
    assert len({hd.glyph_bits(ord(c)) for c in drawn}) == len(drawn)   # no two characters share a bitmap
    assert hd.text_size("", 2) == (0, 14) and hd.text_size("ID:7", 2) == (46, 14) and hd.text_size("8", 1) == (5, 7)
    g = hd.text_primitives("ID:7", 10, 20, 2, 0x010203)
    assert [p[1] for p in g] == [10, 22, 34, 46] and all(p[0] == dc.GLYPH and p[2] == 20 and p[5] == 2 for p in g)
    # a glyph drawn at scale 3 is its bitmap in 3 x 3 blocks
    img = np.zeros((21, 15, 3), np.uint8)
    hd.rasterize_host(img, [(dc.GLYPH, 0, 0, 0, 0, 3, 0xFFFFFF, ord("4"))])
    rows = hd.FONT["4"]
    want = np.array([[(rows[y // 3] >> (4 - x // 3)) & 1 for x in range(15)] for y in range(21)], bool)
    assert np.array_equal(img[..., 0] == 255, want)
    assert hip.draw is hd and hd.pack_primitives([], 3).shape == (3, 8) and hd.pack_primitives([[], g], 5).shape == (2, 5, 8)
    with pytest.raises(ValueError):
        hd.pack_primitives(g, 3)


def test_refusals_touch_nothing():
    L = hip.lib()
    B, P, H, W = 2, 5, 7, 9
    pitch = 3 * W + 1
    need = L.cp_draw_workspace_bytes(B, P)
    assert need > 0 and need % 16 == 0
    assert L.cp_draw_workspace_bytes(0, P) == 0 and L.cp_draw_workspace_bytes(B, 0) == 0
    assert L.cp_draw_workspace_bytes(B, 65537) == 0 and L.cp_draw_workspace_bytes(B, 65536) > 0
    # host memory stands in for the device buffers: a refused call must not even look at them
    frames = np.full(B * H * pitch, 7, np.uint8)
    prims = np.full((B, P, 8), 1, np.int32)
    ws = np.full(need + 64, 5, np.uint8)
    wp = (ws.ctypes.data + 15) // 16 * 16
    f, p = frames.ctypes.data, prims.ctypes.data

    def refused(text, *args):
        assert L.cp_draw_primitives(None, *args) == hip.CP_ERR_INVALID
        assert text in L.cp_last_error().decode(), L.cp_last_error()

    refused("null argument", None, B, H, W, pitch, p, P, wp, need)
    refused("null argument", f, B, H, W, pitch, None, P, wp, need)
    refused("null argument", f, B, H, W, pitch, p, P, None, need)
    refused("B must be >= 1", f, 0, H, W, pitch, p, P, wp, need)
    refused("P must be in", f, B, H, W, pitch, p, 0, wp, need)
    refused("P must be in", f, B, H, W, pitch, p, 65537, wp, need)
    refused("H and W must be in", f, B, 8193, W, pitch, p, P, wp, need)
    refused("H and W must be in", f, B, H, 8193, 3 * 8193, p, P, wp, need)
    refused("H and W must be in", f, B, 0, W, pitch, p, P, wp, need)
    refused("pitch_bytes below 3 W", f, B, H, W, 3 * W - 1, p, P, wp, need)
    refused("workspace too small", f, B, H, W, pitch, p, P, wp, need - 16)   # one entry short
    refused("workspace too small", f, B, H, W, pitch, p, P, wp, need - 1)
    refused("16-byte aligned", f, B, H, W, pitch, p, P, wp + 4, need)
    assert (frames == 7).all() and (prims == 1).all() and (ws == 5).all()
    dp = hip.draw.draw_params(width=W, height=H)
    assert ctypes.sizeof(dp) == dc.host_lib().cp_draw_host_params_bytes()
    assert L.cp_draw_detections(None, None, p, None, None, 1, 1, ctypes.byref(dp), p) == hip.CP_ERR_INVALID
    assert L.cp_draw_detections(None, p, p, None, None, 1, 129, ctypes.byref(dp), p) == hip.CP_ERR_INVALID
    assert L.cp_draw_detections(None, p, p, None, None, 1, 1, None, p) == hip.CP_ERR_INVALID
    assert L.cp_draw_tracks(None, p, 1, 129, None, ctypes.byref(dp), p) == hip.CP_ERR_INVALID
    dp.width = 0
    assert L.cp_draw_tracks(None, p, 1, 8, None, ctypes.byref(dp), p) == hip.CP_ERR_INVALID
    assert "width and height" in L.cp_last_error().decode()


CONFIGS = [dict(), dict(show_axes=True), dict(paper_display=True), dict(debugger_theme='black', show_axes=True), dict(reg_bbox=False)]


@pytest.mark.parametrize("fields", CONFIGS)
def test_record_lists_equal_the_debugger_path(host, fields):
    """draw_build_record (the host build of what the device builders run) against the mirror's ``Debugger`` fed with the same
    records as result dicts: the same primitives in the same order, labels off."""
    post, count, pnp, cam = dc.synthetic_records()
    w, h = dc.W * 4, dc.H * 4
    show_axes = bool(fields.get("show_axes"))
    dicts = dc.record_dicts(post, count, pnp, w, h, show_axes)
    params = hd.draw_params(None, width=w, height=h, vis_thresh=dc.VIS, theme=int(fields.get("debugger_theme", "white") == "white"),
                            show_axes=int(show_axes), paper_display=int(bool(fields.get("paper_display"))),
                            reg_bbox=int(fields.get("reg_bbox", True)))
    n_drawn = 0
    for b in range(post.shape[0]):
        got = []
        for k in range(int(count[b])):
            r, row = post[b, k], pnp[b, k]
            solved = row[0] == 1
            box27 = np.zeros(27)
            if solved:
                loc, quat = (row[4:7], row[24:28]) if show_axes else (row[28:31], row[31:35])
                host.cp_draw_host_cuboid_cam(np.ascontiguousarray(r[2:5]).ctypes.data, np.ascontiguousarray(loc).ctypes.data,
                                             np.ascontiguousarray(quat).ctypes.data, box27.ctypes.data)
            slots = np.full((hip._structs.DRAW_SLOTS, 8), -7, np.int32)
            bbox, proj = np.ascontiguousarray(r[24:28]), np.ascontiguousarray(row[8:24])
            host.cp_draw_host_record(ctypes.addressof(params), float(r[0]), bbox.ctypes.data, proj.ctypes.data if solved else None,
                                     box27.ctypes.data if solved else None, cam[b].ctypes.data, -1.0, slots.ctypes.data)
            got += dc.slots_drawn(slots)
        want = dc.debugger_prims(dicts[b], h, w, cam[b], **fields)
        assert got == [tuple(p) for p in want]
        n_drawn += len(got)
    assert (n_drawn > 100) == bool(fields.get("reg_bbox", True))


def test_track_labels_equal_host_glyphs(host):
    params = hd.draw_params(None, width=300, height=200, vis_thresh=dc.VIS, tracking_task=1, labels=1, theme=0)
    bbox = np.array([40.7, 60.2, 120.9, 150.1])
    for tid in (0, 7, 105, 4294967296):
        slots = np.zeros((hip._structs.DRAW_SLOTS, 8), np.int32)
        host.cp_draw_host_record(ctypes.addressof(params), 0.8, bbox.ctypes.data, None, None, None, float(tid), slots.ctypes.data)
        d = {'score': 0.8, 'bbox': bbox, 'tracking_id': tid}
        want = dc.debugger_prims([d], 200, 300, None, labels=True, tracking_task=True, debugger_theme='black')
        assert dc.slots_drawn(slots) == [tuple(p) for p in want]
        assert len(want) == 2 + len("ID:%d" % tid)


def _golden():
    with open(os.path.join(REPO, "tests", "golden", "draw_calls.json")) as f:
        return json.load(f)


def test_debugger_makes_the_references_calls_in_its_order():
    """Which things are drawn, with which integer coordinates, thickness or radius, colour and text, and in what order: the
    mirror's log against the calls the reference's Debugger made under its own save_results / show_results."""
    from tools import make_draw_goldens as mg

    g = _golden()
    assert g["frame"] == [mg.H, mg.W] and g["vis_thresh"] == mg.VIS
    mine = mg.mirror_calls()
    assert sorted(mine) == sorted(g["calls"]) == sorted(n for n, _, _ in mg.SETS)
    for name, calls in g["calls"].items():
        assert mine[name] == calls, name
    kinds = {c[0] for calls in g["calls"].values() for c in calls}
    assert kinds == {"rectangle", "circle", "line", "putText", "imwrite"}
    assert ["imwrite", "00007_out_img_pred.png"] in g["calls"]["save_black"]   # the reference's file name
    # the named category-0 colours are the reference's
    for name, theme in (("save_black", "black"), ("save_white_tracking", "white")):
        b, gr, r = g["calls"][name][0][3]
        assert b | gr << 8 | r << 16 == hip._structs.DRAW_CAT0[theme]


def test_the_same_comparison_live_where_the_reference_is_present():
    from oracle.tools import ref_harness as rh
    from tools import make_draw_goldens as mg

    if not rh.available():
        pytest.skip("reference tree not present")
    assert mg.record_reference() == _golden()["calls"]


def test_heat_map_views_are_refused_by_name():
    from centerpose_amd.lib.utils.debugger import Debugger

    d = Debugger(theme='white')
    for name in ("gen_colormap", "gen_colormap_hp", "add_blend_img", "add_arrow", "add_coco_hp_paper"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(d, name)(None)
    d.show_all_imgs(pause=True)


def test_saved_png_is_the_rendered_log(tmp_path):
    from PIL import Image

    from centerpose_amd.lib.utils.debugger import Debugger

    d = Debugger(theme='black', device='cpu')
    img = np.random.RandomState(2).randint(0, 256, (50, 70, 3)).astype(np.uint8)
    d.add_img(img, img_id='out_img_pred')
    d.add_coco_bbox([5.5, 20.2, 60.9, 45.1], 0, 0.87, id=12, img_id='out_img_pred')
    d.add_obj_scale([5.5, 20.2, 60.9, 45.1], [0.5, 1.0, 0.25], img_id='out_img_pred')
    d.add_coco_hp(np.arange(16) * 3.7 + 2, img_id='out_img_pred', pred_flag='pnp')
    d.save_all_imgs_demo("/somewhere/00012.png", path=str(tmp_path))
    got = np.asarray(Image.open(str(tmp_path / "00012_out_img_pred.png")).convert("RGB"))[:, :, ::-1]
    want = draw_ref.draw_image(img.copy(), d.primitives('out_img_pred'))
    assert np.array_equal(got, want) and not np.array_equal(want, img)
    assert np.array_equal(d.imgs['out_img_pred'], img)   # the stored frame itself is not drawn into
