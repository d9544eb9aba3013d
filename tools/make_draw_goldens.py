"""Writes tests/golden/draw_calls.json: WHICH drawing calls the reference makes for a handful of result dicts, and in what
order -- the sequence of cv2.rectangle / circle / line / putText calls of its ``Debugger`` under
``ObjectPoseDetector.save_results`` / ``show_results``, recorded by a stand-in for cv2 (no pixels: cv2 is not installed, and the
mirror's rasteriser is its own).  tests/test_draw_cpu.py runs the same result dicts through the mirror's ``Debugger`` and
compares its log with these calls: kind, integer coordinates, thickness or radius, colour, text and order.

The stand-in's ``getTextSize`` answers with the mirror's font metrics (``hip.draw.text_size`` at the mirror's label scale), so
the label geometry of ``add_coco_bbox`` / ``add_obj_scale`` is compared too.  Needs the reference tree; data only is written.

  python tools/make_draw_goldens.py
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

PATH = os.path.join(REPO, "tests", "golden", "draw_calls.json")
H, W = 120, 160
VIS = 0.3
CAM = [[180.0, 0.0, 80.0], [0.0, 175.0, 60.0], [0.0, 0.0, 1.0]]


def results():
    """The result dicts every set draws: with and without a cuboid, a score equal to vis_thresh, a box partly outside the
    frame, a -10000 vertex, negative coordinates."""
    rs = np.random.RandomState(17)

    def box3d(z):
        v = rs.uniform(-0.4, 0.4, (8, 3)) + (0.1, -0.05, z)
        return np.vstack([v.mean(0, keepdims=True), v])

    def rec(score, bbox, cuboid, tid):
        d = {'score': score, 'bbox': np.array(bbox), 'tracking_id': tid, 'kps': rs.uniform(5, 110, 16),
             'obj_scale': np.array([0.51234, 1.0, 0.70449], np.float32), 'obj_scale_kf': np.array([0.49871, 1.0, 0.71555])}
        if cuboid is not None:
            d['projected_cuboid'] = np.array(cuboid, np.float64).reshape(8, 2)
            d['kps_3d_cam'], d['kps_3d_cam_kf'] = box3d(2.0), box3d(2.2)
            k = np.vstack([d['projected_cuboid'].mean(0, keepdims=True), d['projected_cuboid']])
            d['kps_pnp_kf'] = k / (W, H)
        return d

    cub = rs.uniform(8.3, 105.7, 16)
    far = rs.uniform(-30.9, 150.2, 16)
    far[4:6] = -10000
    far[7] = -10000
    return [rec(0.9, [10.7, 20.2, 90.9, 100.5], cub, 3), rec(VIS, [30.1, 30.1, 60.6, 60.6], cub + 3, 4),
            rec(0.5, [-5.5, 50.1, 200.3, 130.9], None, 12), rec(0.7, [40.9, 44.4, 120.2, 99.9], far, 105)]


SETS = [  # name, entry point, opt fields over the defaults
    ("save_black", "save_results", dict(debugger_theme='black')),
    ("save_white_tracking", "save_results", dict(debugger_theme='white', tracking_task=True, scale_pool=True)),
    ("save_paper", "save_results", dict(debugger_theme='black', paper_display=True)),
    ("save_axes_white", "save_results", dict(debugger_theme='white', show_axes=True)),
    ("save_axes_tracking", "save_results", dict(debugger_theme='black', show_axes=True, tracking_task=True)),
    ("save_no_bbox", "save_results", dict(debugger_theme='black', reg_bbox=False)),
    ("show_black", "show_results", dict(debugger_theme='black')),
    ("show_axes_tracking", "show_results", dict(debugger_theme='white', show_axes=True, tracking_task=True)),
]


def make_opt(fields, demo_save):
    o = types.SimpleNamespace(vis_thresh=VIS, reg_bbox=True, paper_display=False, tracking_task=False, show_axes=False,
                              obj_scale=True, scale_pool=False, cam_intrinsic=np.array(CAM), demo='clip.mp4', demo_save=demo_save,
                              debugger_theme='black', dataset='objectron', debug=4)
    o.__dict__.update(fields)
    return o


def _plain(v):
    if isinstance(v, (list, tuple, np.ndarray)):
        return [_plain(x) for x in v]
    return int(v) if isinstance(v, (int, np.integer)) or float(v) == int(v) else float(v)


def run_set(detector_cls, debugger_cls, entry, fields, take_log):
    """One set through ``detector_cls.<entry>`` with a ``debugger_cls`` instance; ``take_log(debugger)`` -> the calls."""
    with tempfile.TemporaryDirectory() as tmp:
        opt = make_opt(fields, os.path.join(tmp, "out"))
        me = types.SimpleNamespace(opt=opt, pause=False)
        for name in ("_draw_box_and_cuboid", "_demo_target"):   # (helpers of the mirror's methods)
            if hasattr(detector_cls, name):
                setattr(me, name, types.MethodType(getattr(detector_cls, name), me))
        dbg = debugger_cls(dataset=opt.dataset, ipynb=False, theme=opt.debugger_theme)
        image = np.zeros((H, W, 3), np.uint8)
        if entry == "save_results":
            getattr(detector_cls, entry)(me, dbg, image, results(), "00007.png", None)
        else:
            getattr(detector_cls, entry)(me, dbg, image, results())
        return take_log(dbg)


_SHIMS = ("cv2", "_ext", "progress", "simplejson", "pyrr", "filterpy", "numba", "sklearn.utils.linear_assignment_", "lib")


def record_reference():
    """{set: calls} from the reference's own modules.  What importing them adds to sys.modules (its `lib` package, the stand-ins
    for its third-party imports) and to sys.path is removed again: other code imports the same names under other stand-ins."""
    before, path = set(sys.modules), list(sys.path)
    try:
        return _record_reference()
    finally:
        for name in set(sys.modules) - before:
            if any(name == s or name.startswith(s + ".") for s in _SHIMS):
                del sys.modules[name]
        sys.path[:] = path


def _record_reference():
    from centerpose_amd.hip import draw as hd
    from centerpose_amd.lib.utils import debugger as mirror
    from oracle.tools import ref_harness as rh

    _, _, rop = rh.reference_host_modules()
    from lib.utils import debugger as rdbg   # the reference's, on the path since reference_host_modules()

    log = []
    cv2 = sys.modules["cv2"]
    before = dict(vars(cv2))
    pt = lambda p: [int(p[0]), int(p[1])]
    cv2.FONT_HERSHEY_SIMPLEX, cv2.LINE_AA = 0, 16
    cv2.getTextSize = lambda txt, font, scale, thick: (hd.text_size(txt, mirror.TEXT_SCALE), 0)
    cv2.rectangle = lambda img, p0, p1, c, t=1, **k: log.append(["rectangle", pt(p0), pt(p1), _plain(c), int(t)])
    cv2.circle = lambda img, p, r, c, t=1, **k: log.append(["circle", pt(p), int(r), _plain(c), int(t)])
    cv2.line = lambda img, p0, p1, c, t=1, **k: log.append(["line", pt(p0), pt(p1), _plain(c), int(t)])
    cv2.putText = lambda img, txt, org, font, scale, c, **k: log.append(["putText", txt, pt(org), _plain(c)])
    cv2.imwrite = lambda path, img: log.append(["imwrite", os.path.basename(path)])
    cv2.imshow = lambda *a, **k: None
    cv2.waitKey = lambda *a, **k: 0

    out = {}
    try:
        for name, entry, fields in SETS:
            del log[:]
            run_set(rop.ObjectPoseDetector, rdbg.Debugger, entry, fields, lambda d: None)
            out[name] = list(log)
    finally:   # the recorders leave the stand-in module as they found it
        for k in set(vars(cv2)) - set(before):
            delattr(cv2, k)
        vars(cv2).update(before)
    return out


def mirror_calls():
    """The same sets through the mirror: {set: calls} in the golden's format."""
    from centerpose_amd.lib.detectors.object_pose import ObjectPoseDetector
    from centerpose_amd.lib.utils.debugger import Debugger

    out = {}
    for name, entry, fields in SETS:
        written = []

        class Dbg(Debugger):
            def _write(self, path, img_id):
                written.append(["imwrite", os.path.basename(path)])
                Debugger._write(self, path, img_id)

        def take(d):
            calls = []
            for op in d.ops['out_img_pred']:
                if op[0] == 'putText':
                    calls.append(["putText", op[1], list(op[2]), list(op[3])])
                else:
                    calls.append([op[0], _plain(op[1]), _plain(op[2]), list(op[3]), op[4]])
            return calls + written

        out[name] = run_set(ObjectPoseDetector, Dbg, entry, fields, take)
    return out


def main():
    calls = record_reference()
    with open(PATH, "w") as f:
        json.dump({"frame": [H, W], "vis_thresh": VIS, "calls": calls}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d bytes, %s" % (PATH, os.path.getsize(PATH), ", ".join("%s %d" % (k, len(v)) for k, v in calls.items())))
    cat0 = {s: c[0][3] for s, c in calls.items() if c and c[0][0] == "rectangle" and c[0][4] == 2}
    print("category-0 colour per set (BGR):", cat0)


if __name__ == "__main__":
    main()
