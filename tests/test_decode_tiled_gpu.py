"""GPU tests of the tiled decode (cp_decode_tiled: peaks_tile_kernel + peaks_merge_kernel + assoc_kernel), which takes
output grids above cp_decode's 32768 pixels (--keep_res on 1280 x 720 video or Objectron's 1440 x 1920 frames,
--input_res 1024):

* bit-identical to cp_decode wherever both accept a shape: band seams (128 x 128 is two bands), sparse, constant,
  negative-valued and fused-sigmoid maps, K = 1 / 100 / 128, a 2048 x 4 map, B = 1 and 32;
* against the CPU oracle at 256 x 256, 184 x 328 and 368 x 488 (pose / tracking heads, rep_mode 0 / 1, both masks);
* the fused in-place sigmoid at 368 x 488 (bands must not overwrite rows a neighbour reads as its halo);
* HipModel.detect and ObjectPoseDetector.run at keep_res / input_res sizes, graph and eager;
* known cuboid poses recovered from a 368 x 488 grid through decode -> post-process -> PnP on the device.
"""
import os

import numpy as np
import pytest
import torch

from centerpose_amd import hip, synth
from oracle import backbone as ob
from oracle import decode as odec
from oracle import pnp as opnp

pytestmark = pytest.mark.gpu

_OPT = ("hps_uncertainty", "scale", "scale_uncertainty", "reg", "hp_offset", "tracking", "tracking_hp")


def _decode(fn, d, device, K=100, rep_mode=1, fit=False, sem="uint8", apply_sigmoid=False):
    g = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in d.items()}
    det = fn(g["hm"], g["hps"], g["wh"], g["hm_hp"], *[g.get(k) for k in _OPT], K=K, rep_mode=rep_mode, fit_gaussian=fit,
             balance=2.0, legacy_bool_mask=(sem == "bool"), apply_sigmoid=apply_sigmoid)
    return det.cpu().numpy(), g


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _maps(kind, B, H, W, seed):
    d = odec.synth_heads(B, seed=seed, H=H, W=W, tracking=(kind == "track"))
    rng = np.random.RandomState(seed + 1)
    if kind == "sparse":
        d["hm"] = d["hm"] * (d["hm"] > 0.9)
        d["hm_hp"] = d["hm_hp"] * (d["hm_hp"] > 0.9)
    elif kind.startswith("const"):
        c = np.float32(float(kind[5:]))
        d["hm"] = np.full_like(d["hm"], c)
        d["hm_hp"] = np.full_like(d["hm_hp"], c)
    elif kind in ("logits", "sigmoid"):  # raw network values: many negative; "sigmoid" lets the decode apply it in place
        d["hm"] = rng.randn(*d["hm"].shape).astype(np.float32) * 3
        d["hm_hp"] = rng.randn(*d["hm_hp"].shape).astype(np.float32) * 3
    return d


def test_tiled_decode_is_bit_identical_to_cp_decode(device):
    cases = []
    for H, W in ((128, 128), (120, 160), (128, 256)):
        for kind in ("synth", "sparse", "const0.5", "const0", "const-0.25", "logits", "sigmoid", "track"):
            for K in (1, 100, 128):
                cases.append((kind, 1, H, W, K))
    cases += [("synth", 32, 128, 128, 100), ("sparse", 32, 128, 128, 128), ("synth", 1, 2048, 4, 100),
              ("sparse", 1, 2048, 4, 128), ("const0.5", 1, 2048, 4, 128)]
    for i, (kind, B, H, W, K) in enumerate(cases):
        d = _maps(kind, B, H, W, seed=400 + i)
        for rep_mode, sem in ((1, "uint8"), (0, "bool")):
            kw = dict(K=K, rep_mode=rep_mode, fit=(kind == "track"), sem=sem, apply_sigmoid=(kind == "sigmoid"))
            a, ga = _decode(hip.decode_raw, d, device, **kw)
            b, gb = _decode(hip.decode_raw_tiled, d, device, **kw)
            tag = "%s B=%d %dx%d K=%d rep=%d" % (kind, B, H, W, K, rep_mode)
            assert np.array_equal(_bits(a), _bits(b)), tag
            if kind == "sigmoid":  # both overwrote the maps with the same values
                assert torch.equal(ga["hm"], gb["hm"]) and torch.equal(ga["hm_hp"], gb["hm_hp"]), tag
            if kind != "synth":
                break


def _oracle(d, K, rep_mode, tracking, sem):
    return odec.object_pose_decode(d["hm"], d["hps"], wh=d["wh"], kps_displacement_std=d.get("hps_uncertainty"),
                                   obj_scale=d["scale"], obj_scale_uncertainty=d.get("scale_uncertainty"), reg=d["reg"],
                                   hm_hp=d["hm_hp"], hp_offset=d["hp_offset"], tracking=d.get("tracking"),
                                   tracking_hp=d.get("tracking_hp"), K=K, rep_mode=rep_mode, tracking_task=tracking,
                                   mask_semantics=sem)


def _assert_matches_oracle(det, o, tracking, tag=""):
    r = {k: v.numpy() for k, v in hip.split_detections(torch.from_numpy(det)).items()}
    for k in o:
        if k in ("kps_displacement_std", "obj_scale_uncertainty"):
            np.testing.assert_allclose(r[k], o[k], rtol=3e-6, atol=0, err_msg=tag + k)
        elif tracking and k.startswith("kps_heatmap"):
            np.testing.assert_allclose(r[k], o[k], rtol=1e-6, atol=1e-6, err_msg=tag + k)
        else:
            np.testing.assert_array_equal(r[k], o[k], err_msg=tag + k)


@pytest.mark.parametrize("H,W,B", [(256, 256, 2), (184, 328, 1), (488, 368, 2)])
@pytest.mark.parametrize("tracking,rep_mode,sem", [(False, 1, "uint8"), (False, 0, "bool"), (True, 1, "uint8")])
def test_tiled_decode_vs_oracle_at_large_grids(device, H, W, B, tracking, rep_mode, sem):
    if tracking:
        B = 1  # the oracle's Gaussian fits run on the host, one per detection and joint
    d = odec.synth_heads(B, seed=H + W + rep_mode, H=H, W=W, tracking=tracking)
    if tracking:
        # the oracle's Gaussian fit (scipy least_squares) refuses the NaN start of a window whose centre column lies in the
        # zero padding, as the reference would; keep the keypoint peaks 12 pixels inside the map
        edge = np.ones((H, W), np.float32) * np.float32(1e-6)
        edge[12:-12, 12:-12] = 1
        d["hm_hp"] = d["hm_hp"] * edge
    det, _ = _decode(hip.decode_raw_tiled, d, device, K=100, rep_mode=rep_mode, fit=tracking, sem=sem)
    _assert_matches_oracle(det, _oracle(d, 100, rep_mode, tracking, sem), tracking)
    if tracking:
        return  # sparse maps: all-zero fit windows, where the oracle (and the reference) refuse the NaN start
    # sparse maps at the same size: fewer than K peaks, the tail is zeros in index order across bands
    d["hm"] = d["hm"] * (d["hm"] > 0.999)
    d["hm_hp"] = d["hm_hp"] * (d["hm_hp"] > 0.999)
    det, _ = _decode(hip.decode_raw_tiled, d, device, K=100, rep_mode=rep_mode, fit=tracking, sem=sem)
    _assert_matches_oracle(det, _oracle(d, 100, rep_mode, tracking, sem), tracking, "sparse ")


def test_tiled_decode_fused_sigmoid_at_368x488(device):
    d = odec.synth_heads(1, seed=21, H=488, W=368)
    logit = lambda p: np.log(np.clip(p, 1e-6, 1 - 1e-6) / (1 - np.clip(p, 1e-6, 1 - 1e-6))).astype(np.float32)
    d_l = dict(d, hm=logit(d["hm"]), hm_hp=logit(d["hm_hp"]))
    det, g = _decode(hip.decode_raw_tiled, d_l, device, K=100, apply_sigmoid=True)
    # every map was overwritten with exactly cp_decode's in-place sigmoid 1 / (1 + expf(-x)), band rows and halo rows
    # alike: cp_decode applied to 64-row slices (<= 32768 pixels each) writes the reference values
    hm_s, hmhp_s = g["hm"].cpu().numpy(), g["hm_hp"].cpu().numpy()
    for k, got in (("hm", hm_s), ("hm_hp", hmhp_s)):
        assert np.abs(got - 1 / (1 + np.exp(-d_l[k].astype(np.float64)))).max() < 1e-6, k
    for y0 in range(0, 488, 64):
        sl = {k: np.ascontiguousarray(v[:, :, y0:y0 + 64]) for k, v in d_l.items()}
        _, gs = _decode(hip.decode_raw, sl, device, K=100, apply_sigmoid=True)
        assert np.array_equal(_bits(gs["hm"].cpu().numpy()), _bits(hm_s[:, :, y0:y0 + 64])), y0
        assert np.array_equal(_bits(gs["hm_hp"].cpu().numpy()), _bits(hmhp_s[:, :, y0:y0 + 64])), y0
    o = odec.object_pose_decode(hm_s, d["hps"], wh=d["wh"], obj_scale=d["scale"], reg=d["reg"], hm_hp=hmhp_s,
                                hp_offset=d["hp_offset"], K=100, rep_mode=1)
    _assert_matches_oracle(det, o, False)
    # and the same as decoding the sigmoided maps directly
    det2, _ = _decode(hip.decode_raw_tiled, dict(d, hm=hm_s, hm_hp=hmhp_s), device, K=100)
    assert np.array_equal(_bits(det), _bits(det2))


def _head_gate(z, zo):
    for k in z:
        ref = torch.sigmoid(zo[k]) if k in ("hm", "hm_hp") else zo[k]
        err = float((z[k].cpu() - ref).abs().max())
        assert err < 1e-3 * max(1.0, float(ref.abs().max())), (k, err)


def test_model_detect_routes_large_grids_to_the_tiled_decode(device):
    """544 x 1024 input -> 136 x 256 = 34816 output pixels: above cp_decode's limit."""
    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("dlav1_34", heads)
    x = synth.frames(1, seed=31, h=544, w=1024)
    zo = ob.dlaseg_forward(sd, x, heads, arch="dlav1")
    model = hip.HipModel("dlav1_34", heads, sd, precision="f16x3")
    xd = x.to(device)
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        for graph in (False, True, True):  # eager, capture + replay, pure replay
            outs, det = model.detect(xd, K=100, rep_mode=1, graph=graph)
            side.synchronize()
            assert tuple(outs["hm"].shape) == (1, 1, 136, 256)
            _head_gate(outs, zo)
            zc = {k: v.cpu().numpy() for k, v in outs.items()}
            o = odec.object_pose_decode(zc["hm"], zc["hps"], wh=zc["wh"], obj_scale=zc["scale"], reg=zc["reg"],
                                        hm_hp=zc["hm_hp"], hp_offset=zc["hp_offset"], K=100, rep_mode=1)
            _assert_matches_oracle(det.cpu().numpy(), o, False, "graph=%s " % graph)


def _demo_opt(extra=()):
    from centerpose_amd.lib.opts import opts

    o = opts().parser.parse_args(["--arch", "dlav1_34", "--c", "cup", "--debug", "5"] + list(extra))
    o.nms = True
    o.obj_scale = True
    o.use_pnp = True
    return opts().init(opts().parse(o))


@pytest.mark.parametrize("frame_hw,extra,grid", [((1920, 1440), ["--keep_res"], (488, 368)),
                                                 ((720, 1280), ["--input_res", "1024"], (256, 256))])
def test_detector_run_at_keep_res_and_input_res(device, tmp_path, frame_hw, extra, grid):
    from centerpose_amd.lib.detectors.detector_factory import detector_factory
    from centerpose_amd.lib.detectors.object_pose import ObjectPoseDetector
    from centerpose_amd.lib.models.model import create_model, save_model
    from tests import scene

    opt = _demo_opt(extra)
    sd = synth.make_state_dict("dlav1_34", opt.heads)
    ck = os.path.join(str(tmp_path), "synthetic_dlav1_34.pth")
    m = create_model(opt.arch, opt.heads, opt.head_conv, opt)
    m.load_state_dict(sd, strict=True)
    save_model(ck, 7, m)
    opt.load_model = ck
    det = detector_factory[opt.task](opt)
    img = np.random.RandomState(3).randint(0, 255, frame_hw + (3,)).astype(np.uint8)
    meta_inp = {"camera_matrix": scene.K_DEMO}
    ret = det.run(img, meta_inp=meta_inp)
    out = ret["output"]
    assert tuple(out["hm"].shape) == (1, 1) + grid
    # the device decode of the returned heads == the oracle decode of the same heads
    o = opt
    z = {k: v.cpu().numpy() for k, v in out.items() if torch.is_tensor(v)}
    dets = odec.object_pose_decode(z["hm"], z["hps"], wh=z["wh"] if o.reg_bbox else None,
                                   kps_displacement_std=z["hps_uncertainty"] if o.hps_uncertainty else None,
                                   obj_scale=z["scale"] if o.obj_scale else None,
                                   obj_scale_uncertainty=z["scale_uncertainty"] if o.obj_scale_uncertainty else None,
                                   reg=z["reg"] if o.reg_offset else None, hm_hp=z["hm_hp"],
                                   hp_offset=z["hp_offset"] if o.reg_hp_offset else None, K=o.K, rep_mode=o.rep_mode,
                                   tracking_task=bool(getattr(o, "tracking_task", False)),
                                   refined_Kalman=bool(getattr(o, "refined_Kalman", False)),
                                   mask_semantics="bool" if getattr(o, "legacy_bool_mask", False) else "uint8")
    _assert_matches_oracle(det.raw_dets.cpu().numpy(), dets, False)
    # ... and the host post-process of the oracle's records gives run()'s results
    _, meta = det.pre_process(img, 1.0, meta_inp)
    assert (meta["out_height"], meta["out_width"]) == grid
    fake = type("S", (), {"opt": opt})()
    ref = ObjectPoseDetector.merge_outputs(fake, [ObjectPoseDetector.post_process(fake, dets, meta, 1)])
    assert len(ret["results"]) == len(ref)
    for a, b in zip(ret["results"], ref):
        for k in ("bbox", "kps", "score", "kps_displacement_mean", "kps_heatmap_mean"):
            np.testing.assert_array_equal(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64), err_msg=k)
    # the batched path (device post-process) at the same geometry gives the same detections
    images, _ = det.pre_process(img, 1.0, meta_inp)
    outs = det.run_batch(images, [meta])
    assert len(outs[0]["results"]) == len(ret["results"])
    for a, b in zip(ret["results"], outs[0]["results"]):
        np.testing.assert_allclose(a["bbox"], b["bbox"], atol=1e-3)
        assert abs(a["score"] - b["score"]) < 1e-5


def _render_rect(B, n_obj, seed, out_h, out_w, cam, sigma=1.5):
    """tests/scene.render on a non-square out_h x out_w grid of a 4x larger image seen through ``cam``."""
    rng = np.random.RandomState(seed)
    f32 = np.float32
    H, W, img_h, img_w = out_h, out_w, 4 * out_h, 4 * out_w
    heads = {"hm": np.zeros((B, 1, H, W), f32), "hm_hp": np.zeros((B, 8, H, W), f32),
             "hps": np.zeros((B, 16, H, W), f32), "wh": np.zeros((B, 2, H, W), f32),
             "reg": np.zeros((B, 2, H, W), f32), "hp_offset": np.zeros((B, 2, H, W), f32),
             "scale": np.ones((B, 3, H, W), f32)}
    ys, xs = np.mgrid[0:H, 0:W]
    scenes = []
    for b in range(B):
        objs, used, tries = [], set(), 0
        while len(objs) < n_obj and tries < 500:
            tries += 1
            scale = np.array([rng.uniform(0.5, 1.5), 1.0, rng.uniform(0.5, 1.5)]) * rng.uniform(0.15, 0.3)
            q = rng.randn(4)
            R = opnp.quat_xyzw_to_matrix(q / np.linalg.norm(q))
            t = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.6, 0.6), rng.uniform(2.0, 4.0)])
            uv = opnp.project_points(opnp.cuboid_vertices(scale), opnp.matrix_to_rodrigues(R), t, cam)
            if uv[:, 0].min() < 8 or uv[:, 0].max() > img_w - 8 or uv[:, 1].min() < 8 or uv[:, 1].max() > img_h - 8:
                continue
            kp = uv / 4.0
            x0, y0, x1, y1 = kp[:, 0].min(), kp[:, 1].min(), kp[:, 0].max(), kp[:, 1].max()
            ct = np.array([(x0 + x1) / 2, (y0 + y1) / 2])
            ci = np.floor(ct).astype(int)
            pix = [tuple(np.floor(k).astype(int)) for k in kp]
            keys = [("c",) + tuple(ci)] + [("k",) + p for p in pix]
            if any((k[0], k[1] + dx, k[2] + dy) in used for k in keys for dx in range(-6, 7) for dy in range(-6, 7)):
                continue
            if len(set(pix)) < 8:
                continue
            used.update(keys)
            g = np.exp(-((xs - ci[0]) ** 2 + (ys - ci[1]) ** 2) / (2 * sigma ** 2)).astype(f32)
            heads["hm"][b, 0] = np.maximum(heads["hm"][b, 0], g * f32(0.95))
            heads["wh"][b, :, ci[1], ci[0]] = [x1 - x0, y1 - y0]
            heads["reg"][b, :, ci[1], ci[0]] = ct - ci
            heads["scale"][b, :, ci[1], ci[0]] = scale / scale[1] * 0.7
            for j in range(8):
                heads["hps"][b, 2 * j:2 * j + 2, ci[1], ci[0]] = kp[j] - ci
                pj = np.array(pix[j])
                gj = np.exp(-((xs - pj[0]) ** 2 + (ys - pj[1]) ** 2) / (2 * sigma ** 2)).astype(f32)
                heads["hm_hp"][b, j] = np.maximum(heads["hm_hp"][b, j], gj * f32(0.9))
                heads["hp_offset"][b, :, pj[1], pj[0]] = kp[j] - pj
            objs.append({"R": R, "t": t, "height": scale[1], "kps_img": uv})
        scenes.append(objs)
    heads["hm"] = np.maximum(heads["hm"], (rng.rand(B, 1, H, W) * 1e-3).astype(f32))
    heads["hm_hp"] = np.maximum(heads["hm_hp"], (rng.rand(B, 8, H, W) * 1e-3).astype(f32))
    return heads, scenes


@pytest.mark.parametrize("rep_mode", [0, 1])
def test_known_poses_recovered_from_a_368x488_grid(device, rep_mode):
    """Objectron-portrait grid (1472 x 1952 image): decode_raw_tiled -> cp_postprocess -> cp_pnp_from_post on the
    device recovers every generating pose to 1 degree / 1 %."""
    B, n_obj, K = 2, 4, 100
    cam = np.array([[1600.0, 0, 736.0], [0, 1600.0, 976.0], [0, 0, 1]])
    heads, scenes = _render_rect(B, n_obj, seed=5, out_h=488, out_w=368, cam=cam)
    g = {k: torch.from_numpy(v).to(device) for k, v in heads.items()}
    det = hip.decode_raw_tiled(g["hm"], g["hps"], g["wh"], g["hm_hp"], None, g["scale"], None, g["reg"], g["hp_offset"],
                               None, None, K=K, rep_mode=rep_mode)
    meta = np.zeros((B, 8))
    meta[:, :6] = [4.0, 0, 0, 0, 4.0, 0]   # output grid -> image: the 4x down-sampling, no crop
    meta[:, 6] = 4.0
    post, cnt = hip.postprocess(det, meta, 0.3, nms=True)
    cam4 = torch.tensor([cam[0, 0], cam[1, 1], cam[0, 2], cam[1, 2]], dtype=torch.float64, device=device).repeat(B, 1)
    poses = hip.pnp_from_post(post, cnt, cam4, rep_mode=rep_mode)
    post, cnt, poses = post.cpu().numpy(), cnt.cpu().numpy(), poses.cpu().numpy()
    n_found = 0
    for b in range(B):
        assert int(cnt[b]) == len(scenes[b]), "image %d: %d detections for %d objects" % (b, cnt[b], len(scenes[b]))
        for k in range(int(cnt[b])):
            row, rec = poses[b, k], post[b, k]
            assert int(row[0]) == 1
            kps = rec[30:46].reshape(8, 2)
            gt = min(scenes[b], key=lambda o: np.linalg.norm(o["kps_img"].mean(0) - kps.mean(0)))
            Rd = opnp.rodrigues_to_matrix(row[1:4])
            ang = np.degrees(np.arccos(np.clip((np.trace(Rd.T @ gt["R"]) - 1) / 2, -1, 1)))
            assert ang < 1.0
            loc = row[4:7] * gt["height"]
            assert np.linalg.norm(loc - gt["t"]) / np.linalg.norm(gt["t"]) < 0.01
            n_found += 1
    assert n_found == sum(len(s) for s in scenes) >= 6
