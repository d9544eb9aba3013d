"""Objectron box metrics on the MI355X (cp_box_iou / cp_box_eval, centerpose_amd/csrc/box3d.hip): against the
reference evaluator's own output (tests/golden/box_eval_ref.npz) with the tolerances of tests/test_box_metrics_cpu.py,
against the host build of the same source, run-to-run determinism on a 4096-pair x 100-rotation batch, and
BoxEvaluator on the device against the reference's AP."""
import numpy as np
import pytest
import torch

from centerpose_amd import box_metrics, hip
from tests import test_box_metrics_cpu as cpu

pytestmark = pytest.mark.gpu

host = cpu.host
g = cpu.g


def _dev_eval(*a):
    return hip.box_eval(*a)


def test_box_iou_against_reference(device, g):
    iou = hip.box_iou(g["iou_a"], g["iou_b"])
    assert np.abs(iou - g["iou_ref"]).max() <= cpu.IOU_TOL
    k = g["iou_kind"]
    for kind in (2, 5, 6, 7):
        assert np.all(iou[k == kind] == 0.0)
    # device tensors in place of host arrays
    t = hip.box_iou(torch.from_numpy(g["iou_a"]).to(device), torch.from_numpy(g["iou_b"]).to(device))
    assert np.array_equal(t, iou)


def test_box_eval_against_reference(device, g):
    cpu.check_against_reference(cpu.eval_golden(_dev_eval, g), g)


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def test_device_matches_host_build(device, host, g):
    """same source, no contraction in either build: only the math library's sin / cos / atan2 / hypot differ"""
    iou_d = hip.box_iou(g["iou_a"], g["iou_b"])
    iou_h = cpu.host_iou(host, g["iou_a"], g["iou_b"])
    assert _rel(iou_d, iou_h).max() <= 1e-12
    d = cpu.eval_golden(_dev_eval, g)
    h = cpu.eval_golden(lambda *a: cpu.host_eval(host, *a), g)
    same = d[:, 6] == h[:, 6]
    for p in np.where(~same)[0]:  # a tie to rounding may go either way
        rots = g["ev_rot_iou"][p]
        assert abs(rots[int(d[p, 6])] - rots[int(h[p, 6])]) < cpu.TIE, p
    assert _rel(d[same, :6], h[same, :6]).max() <= 1e-12
    assert np.array_equal(d[:, 7:], h[:, 7:])


def _batch(n, seed):
    from tools.make_box_eval_goldens import box, gl_projection, mo2c, object_pose, project, rot

    rng = np.random.RandomState(seed)
    P = gl_projection()
    pr, gt, p2, M = [], [], [], []
    for _ in range(n):
        R, t, s = object_pose(rng)
        gt.append(box(R, t, s))
        M.append(mo2c(R, t))
        pr.append(box(R @ rot([0, 1, 0], rng.uniform(-np.pi, np.pi)), t + rng.randn(3) * 0.03,
                      s * rng.uniform(0.9, 1.1, 3)))
        p2.append(project(P, gt[-1]) + rng.randn(9, 2) * 0.004)
    return np.array(pr), np.array(gt), np.array(p2), np.array(M), np.repeat(P[None], n, 0)


def test_large_batch_is_deterministic(device, host):
    """4096 pairs x 100 rotations, twice: bit-identical; a sample against the host build"""
    pr, gt, p2, M, P = _batch(4096, 11)
    single = np.zeros(4096, np.int32)
    single[::97] = 1
    a = hip.box_eval(pr, gt, p2, M, P, single, 100)
    b = hip.box_eval(pr, gt, p2, M, P, single, 100)
    assert np.array_equal(a, b, equal_nan=True)
    assert np.all(a[:, 8] == 0) and np.all(a[:, 0] > 0.2)
    idx = np.arange(0, 4096, 37)
    h = cpu.host_eval(host, pr[idx], gt[idx], p2[idx], M[idx], P[idx], single[idx], 100)
    same = a[idx, 6] == h[:, 6]
    assert same.mean() > 0.9
    assert _rel(a[idx][same, :6], h[same, :6]).max() <= 1e-12
    # every other sampled pair: the device's rotation ties the host build's best in the host build's own IoU
    for j in np.where(~same)[0]:
        p = idx[j]
        ious = []
        for r in (int(a[p, 6]), int(h[j, 6])):
            assert r >= 0
            th = 2 * np.pi if r == 99 else r * (2 * np.pi / 99)  # np.linspace(0, 2 pi, 100)[r]
            rb = np.zeros((9, 3))
            host.box_host_rotate(cpu._p(np.ascontiguousarray(pr[p])), th, cpu._p(rb))
            ious.append(cpu.host_iou(host, rb[None], gt[p][None])[0])
        assert abs(ious[0] - ious[1]) < cpu.TIE and abs(ious[1] - h[j, 0]) < 1e-12, (p, ious, h[j, 0])
        assert abs(a[p, 0] - h[j, 0]) < cpu.TIE


def test_evaluator_on_device_against_reference(device, g):
    ev = box_metrics.BoxEvaluator(num_symmetry=int(g["seq_nsym"]))
    ev.evaluate(cpu.sequence_images(g))
    cpu.check_sequence(ev, ev.finalize(), g)


def _pose_detector(tmp_path):
    import os

    from centerpose_amd import synth
    from centerpose_amd.lib.detectors.detector_factory import detector_factory
    from centerpose_amd.lib.models.model import create_model, save_model
    from centerpose_amd.lib.opts import opts

    o = opts().parser.parse_args(["--arch", "dlav1_34", "--c", "cup", "--debug", "5"])
    o.nms, o.obj_scale, o.use_pnp = True, True, True
    opt = opts().init(opts().parse(o))
    ck = os.path.join(str(tmp_path), "synthetic_dlav1_34.pth")
    m = create_model(opt.arch, opt.heads, opt.head_conv, opt)
    m.load_state_dict(synth.make_state_dict("dlav1_34", opt.heads), strict=True)
    save_model(ck, 7, m)
    opt.load_model = ck
    return detector_factory[opt.task](opt), opt


def _labels(objs, K, W, H):
    """Objectron-style labels of the generating cuboids in the frame the detector's PnP returns (show_axes off): the
    solver's OpenGL variant M [R | t] with M = [[0,1,0],[1,0,0],[0,0,-1]] (x and y swapped, z < 0 in front), in units of
    the object height (the network predicts the relative size only, so PnP's translation is t / height), and 2D points
    normalised by the image size -- the projection matrix below maps the OpenGL frame to exactly those after the
    evaluator's viewport swap."""
    from oracle import pnp as opnp

    Mgl = np.array([[0, 1., 0], [1., 0, 0], [0, 0, -1.]])
    inst2d, inst3d, scale, Mo2c = [], [], [], []
    for o in objs:
        V = opnp.cuboid_vertices(o["scale"] * o["height"])
        V = np.vstack([V.mean(0, keepdims=True), V])
        cam = (V @ o["R"].T + o["t"]) / o["height"]
        inst3d.append(cam @ Mgl.T)
        uv = cam[:, :2] / cam[:, 2:3] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
        inst2d.append(uv / [W, H])
        scale.append(o["scale"])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Mgl @ o["R"], Mgl @ o["t"] / o["height"]
        Mo2c.append(T)
    # viewport = swap((P p / w + 1) / 2) = (u / W, v / H) with u = fx y / -z + cx, v = fy x / -z + cy in OpenGL terms
    proj = np.array([[2 * K[1, 1] / H, 0, 1 - 2 * K[1, 2] / H, 0], [0, 2 * K[0, 0] / W, 1 - 2 * K[0, 2] / W, 0],
                     [0, 0, -1.0, -0.1], [0, 0, -1.0, 0]])
    label = {"2d_instance": np.array(inst2d), "3d_instance": np.array(inst3d), "scale_instance": np.array(scale),
             "Mo2c_instance": np.array(Mo2c), "visibility": np.ones(len(objs))}
    return label, proj


def test_detector_boxes_against_generating_cuboids(device, tmp_path):
    """End to end: heads rendered from known cuboid poses (tests/scene.py) through ObjectPoseDetector.run and run_batch
    (device decode, post-process, PnP), their ret['boxes'] evaluated by BoxEvaluator on the device against labels built
    from the generating cuboids: every object found, IoU >= 0.9, AP at IoU 0.5 = 1."""
    from tests import scene

    det, opt = _pose_detector(tmp_path)
    B, n_obj = 2, 3
    heads, scenes = scene.render(B, n_obj, seed=21)
    dev_heads = {k: torch.from_numpy(v).to(device) for k, v in heads.items()}
    eng = det.model._engine()
    feed = {}

    def forward(images, *a, **k):  # the network's heads for the frames being run: the rendered ones
        return {h: v[feed["b"]:feed["b"] + images.shape[0]] for h, v in dev_heads.items()}

    eng.forward = forward
    img = np.zeros((512, 512, 3), np.uint8)
    meta_inp = {"camera_matrix": scene.K_DEMO}
    frames = [_labels(scenes[b], scene.K_DEMO, 512, 512) for b in range(B)]
    plane = (np.zeros(3), np.zeros(3))  # unused with use_absolute_scale

    rets = []
    for b in range(B):
        feed["b"] = b
        rets.append(det.run(img, meta_inp=meta_inp)["boxes"])
    images, meta = det.pre_process(img, 1.0, meta_inp)
    feed["b"] = 0
    batched = [o["boxes"] for o in det.run_batch(torch.cat([images] * B), [meta] * B)]

    for boxes_per_image in (rets, batched):
        assert [len(bx) for bx in boxes_per_image] == [len(s) for s in scenes]
        for nsym in (1, 100):
            ev = box_metrics.BoxEvaluator(num_symmetry=nsym, use_absolute_scale=True)
            rec = ev.evaluate([(bx, lab, plane, proj) for bx, (lab, proj) in zip(boxes_per_image, frames)])
            res = ev.finalize()
            assert res["matched"] == sum(len(s) for s in scenes) and res["flagged"] == 0
            assert rec[:, 0].min() >= 0.9, rec[:, 0]
            assert res["ap"]["iou"][10] == 1.0  # threshold 0.5
            assert rec[:, 5].max() < 0.01 and rec[:, 1].max() < 0.05  # 2D error (normalised), ADD (object heights)
