"""The overlay's case list, shared by tests/test_draw_cpu.py (host build) and tests/test_draw_gpu.py (device): primitive lists
for B = 3 frames of 61 x 83 with a pitch of 3 * 83 + 5 bytes (one and a bit tiles wide, four tiles high) and for a 1 x 1 frame,
the host-build fixture, and the synthetic records of the list builders.  Shapes are the smallest that still cross a tile border
in both directions, leave a partial tile on both sides and make the pitch misalign every other row for dword stores."""
import ctypes
import os
import subprocess

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
B, H, W = 3, 61, 83
PITCH = 3 * W + 5
SEG, DISC, RECT, FILL, GLYPH = 1, 2, 3, 4, 5


def background(b=B, h=H, pitch=PITCH, seed=5):
    return np.random.RandomState(seed).randint(0, 256, b * h * pitch).astype(np.uint8)


def _col(i):
    return ((37 * i + 11) % 256) | ((91 * i + 5) % 256) << 8 | ((53 * i + 200) % 256) << 16


def edge_prims():
    """Every kind on and across the four borders of the frame and across the tile borders (x = 64; y = 16, 32, 48), the sizes
    at both ends of their ranges, degenerate and reversed geometry, what the rule skips."""
    p = []
    xs, ys = (-3, 0, 63, 64, W - 1, W + 2), (-2, 0, 15, 16, 47, 48, H - 1, H + 3)
    for i, t in enumerate((1, 2, 5, 16)):
        p.append((SEG, xs[i], ys[i], xs[i + 2], ys[i + 3], t, 0, 0))          # oblique, across tile and frame borders
        p.append((SEG, -5, ys[i + 1], W + 5, ys[i + 1], t, 0, 0))             # horizontal through the whole frame
        p.append((SEG, xs[i + 1], -4, xs[i + 1], H + 4, t, 0, 0))             # vertical through the whole frame
        p.append((SEG, xs[i + 2], ys[i + 2], xs[i + 2], ys[i + 2], t, 0, 0))  # zero length
        p.append((RECT, xs[i], ys[i], xs[5 - i], ys[7 - i], t, 0, 0))
        p.append((RECT, xs[5 - i], ys[7 - i], xs[i], ys[i], t, 0, 0))         # corners in reversed order
    p.append((SEG, 70, 50, 10, 3, 3, 0, 0))                                   # P1 left of and above P0
    for r, (x, y) in zip((0, 1, 5, 64, 64, 0), ((0, 0), (W - 1, H - 1), (64, 16), (40, 30), (-60, H + 50), (63, 47))):
        p.append((DISC, x, y, 0, 0, r, 0, 0))
    p += [(FILL, 60, 10, 70, 20, 0, 0, 0), (FILL, 70, 36, 58, 28, 0, 0, 0), (FILL, -9, -9, 200, 200, 0, 0, 0),
          (FILL, 0, 47, 82, 48, 7, 0, 0), (FILL, W - 1, H - 1, W - 1, H - 1, 0, 0, 0), (FILL, 2, 2, 2, 9, 0, 0, 0)]
    for i, ch in enumerate("ID:8/-. xop"):                                      # (' ' and 'x' have no bitmap)
        p.append((GLYPH, 58 + 3 * i, 12 + 4 * i, 0, 0, 1 + i % 3, 0, ord(ch)))
    p += [(GLYPH, -4, -6, 0, 0, 8, 0, ord("0")), (GLYPH, W - 3, H - 4, 0, 0, 2, 0, ord("5")), (GLYPH, 30, 20, 0, 0, 8, 0, ord("P"))]
    # fully off the frame
    p += [(SEG, -50, -50, -20, -10, 5, 0, 0), (DISC, 200, 30, 0, 0, 64, 0, 0), (RECT, 100, 70, 150, 90, 2, 0, 0),
          (FILL, -30, 5, -1, 50, 0, 0, 0), (GLYPH, 10, H, 0, 0, 3, 0, ord("1"))]
    # the ends of the coordinate range, and one beyond (skipped whole)
    p += [(SEG, -8192, -8192, 8191, 8191, 16, 0, 0), (SEG, -8192, 8191, 8191, -8192, 1, 0, 0), (SEG, -8193, 0, 50, 50, 5, 0, 0),
          (SEG, 0, 0, 8192, 50, 5, 0, 0), (FILL, -8192, 30, 8191, 31, 0, 0, 0), (FILL, 0, -8193, 50, 50, 0, 0, 0),
          (DISC, 8192, 10, 0, 0, 64, 0, 0), (DISC, 40, 30, 0, -8193, 3, 0, 0), (RECT, -8192, -8192, 8191, 8191, 2, 0, 0),
          (RECT, 5, 5, 40, 8192, 2, 0, 0), (GLYPH, 5, 5, 9000, 0, 2, 0, ord("3")), (SEG, 1 << 30, 0, 5, 5, 2, 0, 0),
          (SEG, -(1 << 31), 3, 5, 5, 2, 0, 0)]
    # sizes out of range, unknown kinds
    p += [(SEG, 5, 5, 50, 40, 0, 0, 0), (SEG, 5, 5, 50, 40, 17, 0, 0), (SEG, 5, 5, 50, 40, -2, 0, 0), (DISC, 30, 30, 0, 0, -1, 0, 0),
          (DISC, 30, 30, 0, 0, 65, 0, 0), (RECT, 5, 5, 50, 40, 0, 0, 0), (RECT, 5, 5, 50, 40, 17, 0, 0), (GLYPH, 5, 5, 0, 0, 0, 0, 48),
          (GLYPH, 5, 5, 0, 0, 9, 0, 48), (GLYPH, 5, 5, 0, 0, 2, 0, 300), (GLYPH, 5, 5, 0, 0, 2, 0, -48), (0, 5, 5, 50, 40, 2, 0, 0),
          (6, 5, 5, 50, 40, 2, 0, 0), (-1, 5, 5, 50, 40, 2, 0, 0), (1 << 20, 5, 5, 50, 40, 2, 0, 0)]
    return [q[:6] + (_col(i),) + q[7:] for i, q in enumerate(p)]


def edge_case():
    """[B, P, 8]: the edge list spread over the three images in turn (each keeps its order), so that no image is one blob."""
    e = edge_prims()
    per = [e[b::B] for b in range(B)]
    P = max(len(x) for x in per) + 3
    out = np.zeros((B, P, 8), np.int32)
    for b in range(B):
        out[b, 2:2 + len(per[b])] = np.asarray(per[b], np.int64)   # (kind-0 slots in front and behind)
    return out


def order_case():
    """Three mutually overlapping primitives, in one order in image 0 and reversed in image 1; image 2 has one of each pair."""
    a = [(FILL, 20, 10, 70, 40, 0, 0x0000FF, 0), (DISC, 60, 30, 0, 0, 25, 0x00FF00, 0), (SEG, 5, 50, 80, 8, 16, 0xFF0000, 0)]
    out = np.zeros((B, 4, 8), np.int32)
    out[0, :3], out[1, 1:], out[2, 0], out[2, 3] = a, a[::-1], a[1], a[0]
    return out


def many_case(P=700):
    """P = 700 slots: image 0 empty, image 1 with every slot active (small primitives all over the frame: more than any staging
    chunk, in one tile too), image 2 with actives only in the last 10 slots."""
    rs = np.random.RandomState(11)
    out = np.zeros((B, P, 8), np.int32)
    kind = rs.randint(1, 6, P)
    x, y = rs.randint(-2, W + 2, P), rs.randint(-2, H + 2, P)
    x[:300], y[:300] = rs.randint(60, 68, 300), rs.randint(12, 20, 300)      # 300 of them at one tile corner
    dx, dy = rs.randint(-6, 7, P), rs.randint(-6, 7, P)
    size = np.where(kind == 5, 1, rs.randint(1, 4, P))
    aux = np.where(kind == 5, rs.randint(48, 58, P), 0)
    col = rs.randint(0, 1 << 24, P)
    out[1] = np.stack([kind, x, y, x + dx, y + dy, size, col, aux], 1)
    out[2, P - 10:] = out[1, :10]
    return out


def tiny_case():
    """A 1 x 1 frame: (prims [1, P, 8], H, W, pitch)."""
    p = [(DISC, 5, 5, 0, 0, 3, 0x010203, 0), (FILL, 0, 0, 0, 0, 0, 0x112233, 0), (SEG, -3, -3, 3, 3, 1, 0x445566, 0),
         (DISC, 1, 0, 0, 0, 0, 0x778899, 0), (GLYPH, 0, 0, 0, 0, 1, 0xABCDEF, ord("1"))]
    return np.asarray(p, np.int32)[None], 1, 1, 3


def host_lib():
    """tests/native/draw_host.cpp built for the host (the same draw_common.h the device compiles)."""
    out = os.path.join(REPO, "tests", "_build", "libcp_draw_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(REPO, "tests", "native", "draw_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
    lib = ctypes.CDLL(out)
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.cp_draw_host_primitives.restype = None
    lib.cp_draw_host_primitives.argtypes = [vp, i, i, i, ctypes.c_size_t, vp, i]
    lib.cp_draw_host_glyph.restype = ctypes.c_ulonglong
    lib.cp_draw_host_glyph.argtypes = [i]
    lib.cp_draw_host_params_bytes.restype = i
    lib.cp_draw_host_cuboid_cam.restype = None
    lib.cp_draw_host_cuboid_cam.argtypes = [vp] * 4
    lib.cp_draw_host_record.restype = None
    lib.cp_draw_host_record.argtypes = [vp, d, vp, vp, vp, vp, d, vp]
    return lib


def host_draw(lib, buf, b, h, w, pitch, prims):
    out = np.array(buf, np.uint8).copy()
    prims = np.ascontiguousarray(prims, np.int32)
    lib.cp_draw_host_primitives(out.ctypes.data, b, h, w, pitch, prims.ctypes.data, prims.shape[1])
    return out


# ---- synthetic records of the list builders ----
VIS = 0.3


def synthetic_records(nb=2, K=8, seed=3, w=W * 4, h=H * 4):
    """(post [nb, K, 120], count [nb], pnp [nb, K, 40], cam [nb, 4]) float64 / int32: plausible records in a w x h frame, then
    the cases a builder can get wrong written over single fields."""
    rs = np.random.RandomState(seed)
    post = np.zeros((nb, K, 120))
    pnp = np.zeros((nb, K, 40))
    post[..., 0] = rs.uniform(0.35, 0.95, (nb, K))
    post[..., 2:5] = rs.uniform(0.5, 1.5, (nb, K, 3))
    x0, y0 = rs.uniform(5, w / 2, (nb, K)), rs.uniform(5, h / 2, (nb, K))
    post[..., 24], post[..., 25] = x0, y0
    post[..., 26], post[..., 27] = x0 + rs.uniform(10, w / 2, (nb, K)), y0 + rs.uniform(10, h / 2, (nb, K))
    post[..., 30:46] = rs.uniform(0, min(w, h), (nb, K, 16))
    pnp[..., 0] = 1
    pnp[..., 8:24] = rs.uniform(-20.7, max(w, h) + 20.7, (nb, K, 16))
    q = rs.normal(size=(nb, K, 4))
    pnp[..., 24:28] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    pnp[..., 31:35] = pnp[..., 24:28][..., ::-1]
    pnp[..., 4:7] = rs.uniform(-0.3, 0.3, (nb, K, 3)) + (0, 0, 2.0)
    pnp[..., 28:31] = pnp[..., 4:7] * (1, -1, -1)
    post[0, 0, 0] = VIS                      # a score equal to vis_thresh: not drawn (strict)
    post[0, 1, 0] = np.nextafter(VIS, 1)     # the next double: drawn
    pnp[0, 2, 0], pnp[0, 3, 0], pnp[0, 4, 0] = 0, 2, -1   # PnP status other than 1: box only
    pnp[0, 5, 8], pnp[0, 5, 11] = np.nan, 1e9   # a NaN and a 1e9 vertex coordinate: their discs and edges withdrawn
    pnp[0, 5, 12:14] = -10000                    # the reference's "no such vertex"
    pnp[0, 6, 8:24] = -rs.uniform(0.2, 30.9, 16)  # negative coordinates: truncation towards zero
    post[0, 6, 24:26] = (-7.9, -0.4)            # a box partly outside the frame, negative corners
    post[0, 7, 26:28] = (w + 40.5, h + 0.9)     # ... and past the right / lower border
    post[1, 0, 24] = np.inf                     # a box with a non-finite corner: withdrawn, the cuboid stays
    post[1, 1, 26] = 1e9
    post[1, 2, 0] = np.nan                      # a NaN score: not drawn
    pnp[1, 3, 4:7] = (0.1, 0.1, 0.0)            # a cuboid centre in the camera plane: axes divide by ~0
    count = np.array([K, K - 3] + [0] * (nb - 2), np.int32)[:nb]
    cam = np.array([[w * 1.1, w * 1.1, w / 2.0, h / 2.0]] * nb)
    return post, count, pnp, cam


def record_dicts(post, count, pnp, w, h, show_axes=False):
    """The records read back as the result dicts ``run_batch`` builds: per image a list of dicts with score, bbox, kps,
    obj_scale and -- where the solve's status is 1 -- what ``finish_detection`` adds (projected_cuboid, kps_3d_cam)."""
    import types

    from centerpose_amd.lib.utils.pnp.cuboid_pnp_shell import finish_detection

    opt = types.SimpleNamespace(c='bike')   # (no visibility reject: it does not decide what is drawn)
    out = []
    for b in range(post.shape[0]):
        items = []
        for k in range(int(count[b])):
            r, row = post[b, k], None if pnp is None else pnp[b, k]
            d = {'score': float(r[0]), 'bbox': r[24:28].copy(), 'kps': r[30:46].copy(), 'obj_scale': r[2:5].astype(np.float32)}
            if row is not None and int(row[0]) == 1:
                loc, quat = (list(row[4:7]), row[24:28].copy()) if show_axes else (list(row[28:31]), row[31:35].copy())
                finish_detection(opt, {'width': w, 'height': h}, d, d['obj_scale'], loc, quat, row[8:24].reshape(8, 2).copy())
            items.append(d)
        out.append(items)
    return out


def debugger_prims(dicts, h, w, cam4=None, labels=False, **fields):
    """What the mirror's ``Debugger`` logs for one image's result dicts under ``save_results``' rule for the box, the cuboid and
    the axes, as the primitives the rule would draw: those with every coordinate in range, the host-formatted text left out
    (``labels``: keep the tracks' label rectangle, re-sized to 'ID:<n>', and its glyphs)."""
    import types

    from centerpose_amd.hip import draw as hd
    from centerpose_amd.lib.detectors.object_pose import ObjectPoseDetector
    from centerpose_amd.lib.utils.debugger import TEXT_SCALE, Debugger

    K = None if cam4 is None else np.array([[cam4[0], 0, cam4[2]], [0, cam4[1], cam4[3]], [0, 0, 1.0]])
    opt = types.SimpleNamespace(vis_thresh=VIS, reg_bbox=True, paper_display=False, tracking_task=False, show_axes=False,
                                cam_intrinsic=K, debugger_theme='white')
    opt.__dict__.update(fields)
    me = types.SimpleNamespace(opt=opt)
    dbg = Debugger(theme=opt.debugger_theme)
    dbg.add_img(np.zeros((h, w, 3), np.uint8), img_id='out_img_pred')
    for d in dicts:
        if d['score'] > opt.vis_thresh and opt.reg_bbox:
            if K is None and (opt.show_axes or opt.paper_display):
                d = {k: v for k, v in d.items() if k not in ('kps_3d_cam', 'kps_3d_cam_kf')}
                try:
                    ObjectPoseDetector._draw_box_and_cuboid(me, dbg, d, opt.paper_display)
                except KeyError:
                    pass
                continue
            n0 = len(dbg.ops['out_img_pred'])
            ObjectPoseDetector._draw_box_and_cuboid(me, dbg, d, opt.paper_display)
            ops = dbg.ops['out_img_pred']
            for i in range(n0, len(ops)):   # the label as the device draws it: 'ID:<n>' alone
                if labels and ops[i][0] == 'putText':
                    txt = 'ID:%d' % d['tracking_id']
                    (x, y), tw = ops[i][2], hd.text_size(txt, TEXT_SCALE)[0]
                    ops[i - 1] = ('rectangle', ops[i - 1][1], (x + tw, ops[i - 1][2][1]), ops[i - 1][3], -1)
                    ops[i] = ('putText', txt, (x, y), ops[i][3])
    prims = dbg.primitives('out_img_pred')
    if not labels:
        prims = [p for p in prims if p[0] not in (FILL, GLYPH)]
    return [p for p in prims if all(-8192 <= v <= 8191 for v in p[1:5])]


def slots_drawn(slots):
    """The non-empty slots of a builder's output [n, 8] as tuples, in order."""
    return [tuple(int(v) for v in p) for p in np.asarray(slots).reshape(-1, 8) if p[0] != 0]
