"""Times the tracking task's targets with the detector in the loop (TrackPoseTargets with a detector,
cp_pose_targets_track_det) at B = 16 and 32, 512 x 512 input (output 128 x 128), 8 joints, S = 1, with
data_generation_mode_ratio 0.3 and 1.0, and writes the table to profiles/track_targets_det_bench.txt (or --out).

The detector is the synthetic dlav1_34 (centerpose_amd.synth), vis_thresh 0.05 so that its random weights leave some
detections; the previous frames are synthetic images, the annotations random, the per-sample mode drawn with the ratio.

  (a) on the device, HIP events around --iters calls on a side stream (the detector's hipGraph replays):
      mode 0     the parent's call: TrackPoseTargets without a detector on the same records
      full       TrackPoseTargets(opt, detector=model)(records, pre_img)
      added      full - mode 0, and its parts, each timed on its own:
      detector   HipModel.detect on the batch (backbone, heads, decode)
      post+PnP   hip.postprocess + hip.pnp_from_post on its output
      match+tgt  the call with the detections handed over (cp_pose_targets_track_det) minus mode 0
  (b) the host route this replaces, wall clock per batch: ObjectPoseDetector.run_batch on the same images (device
      network, one copy to the host, boxes in Python), then the numpy restatement
      tests/pose_targets_track_det_ref.py for the batch, one thread.
Three rounds, the variants alternating within a round; the median of the rounds is reported.

  python tools/track_targets_det_bench.py [--iters 10] [--out profiles/track_targets_det_bench.txt]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from centerpose_amd import hip, synth  # noqa: E402
from centerpose_amd.pose_targets import num_symmetry  # noqa: E402
from centerpose_amd.pose_targets_track import TrackPoseTargets, draw_generation_mode  # noqa: E402
from tests import pose_target_track_det_cases as DC  # noqa: E402
from tests import pose_targets_track_det_ref as DR  # noqa: E402
from tests import pose_targets_track_ref as TR  # noqa: E402


def make_detector(tmp):
    from centerpose_amd.lib.detectors.detector_factory import detector_factory
    from centerpose_amd.lib.models.model import create_model, save_model
    from centerpose_amd.lib.opts import opts

    o = opts().parser.parse_args(["--arch", "dlav1_34", "--c", "camera", "--debug", "5", "--vis_thresh", "0.05"])
    o.obj_scale, o.use_pnp, o.rep_mode = True, True, 1
    o = opts().init(opts().parse(o))
    ck = os.path.join(tmp, "synthetic_dlav1_34.pth")
    m = create_model(o.arch, o.heads, o.head_conv, o)
    m.load_state_dict(synth.make_state_dict("dlav1_34", o.heads), strict=True)
    save_model(ck, 1, m)
    o.load_model = ck
    return detector_factory[o.task](o)


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_targets_det_bench.txt"))
    ap.add_argument("--batches", default="16,32")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    inp, Rr, w, h = 512, 128, 640, 480
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        det = make_detector(tmp)
        over = dict(c="camera", input_res=inp, input_w=inp, input_h=inp, output_res=Rr, render_hm_mode=1,
                    render_hmhp_mode=2, tracking_label_mode=1)
        for B in (int(v) for v in args.batches.split(",")):
            for ratio in (0.3, 1.0):
                opt = DC.make_opt(over, data_generation_mode_ratio=ratio)
                rng = np.random.default_rng(B)
                modes = [draw_generation_mode(rng, ratio) for _ in range(B)]
                per = [DC.random_image(rng, opt, mode=m, n_slots=0, K=100)[0] for m in modes]
                recs = {k: np.stack([p[k] for p in per]) for k in per[0]}
                recs0 = {k: v for k, v in recs.items() if k not in ("ptk_gen", "ptk_det_meta")}
                x = synth.frames(B, seed=B, h=inp, w=inp).to(dev)
                full = TrackPoseTargets(opt, detector=det.model, det_opt=det.opt)
                plain = TrackPoseTargets(DC.make_opt(over, data_generation_mode_ratio=0))
                side = torch.cuda.Stream(dev)
                t = {k: [] for k in ("mode0", "full", "detector", "post", "given", "run_batch", "numpy")}
                fx = 1.1 * max(w, h)
                cam = np.array([[fx, 0, w / 2.0], [0, fx, h / 2.0], [0, 0, 1.0]])
                metas = [{"c": np.array([w / 2.0, h / 2.0], np.float32), "s": float(max(w, h)), "out_height": Rr,
                          "out_width": Rr, "width": w, "height": h, "inp_height": inp, "inp_width": inp,
                          "camera_matrix": cam} for _ in range(B)]
                with torch.cuda.stream(side):
                    dets = full.detect(x, recs["ptk_det_meta"])
                    torch.cuda.synchronize()
                    raw = full.detector.detect(full._det_in, K=100, rep_mode=1, graph=True, **full.decode)[1]
                    meta_d = full._det_meta.to(dev)
                    for _ in range(3):
                        t["mode0"].append(event_ms(lambda: plain(recs0, device=dev), args.iters))
                        t["full"].append(event_ms(lambda: full(recs, pre_img=x), args.iters))
                        t["detector"].append(event_ms(lambda: full.detector.detect(full._det_in, K=100, rep_mode=1, graph=True,
                                                                                   **full.decode), args.iters))
                        t["post"].append(event_ms(lambda: hip.pnp_from_post(
                            *hip.postprocess(raw, meta_d[:, :8].contiguous(), full.det["vis_thresh"], full.det["nms"]),
                            meta_d[:, 8:12].contiguous(), 1), args.iters))
                        t["given"].append(event_ms(lambda: full(recs, detections=dets), args.iters))
                        t0 = time.perf_counter()
                        outs = det.run_batch(x, metas)
                        t["run_batch"].append((time.perf_counter() - t0) * 1e3)
                        boxes = [o["boxes"] for o in outs]
                        t0 = time.perf_counter()
                        DR.batch_targets(recs, boxes, num_symmetry(opt), Rr, TR.options(opt), DR.det_options(opt))
                        t["numpy"].append((time.perf_counter() - t0) * 1e3)
                m = {k: float(np.median(v)) for k, v in t.items()}
                rows.append((B, ratio, sum(modes), int(dets[1].sum()), sum(len(b) for b in boxes), m))
                print(rows[-1], flush=True)
    lines = ["TrackPoseTargets with a detector (cp_pose_targets_track_det) at 512x512 input, 128x128 output, 8 joints, S = 1, "
             "synthetic dlav1_34 detector (f16x3, vis_thresh 0.05, K 100, rep_mode 1); GPU events around %d calls on a side "
             "stream, three alternating rounds, medians" % args.iters,
             "mode 0 = the call without a detector on the same records; full = detector + post-process + PnP + matching + "
             "targets; added = full - mode 0; detector / post+PnP timed alone; match+tgt = the call with the detections "
             "handed over - mode 0; host route = ObjectPoseDetector.run_batch (wall clock) + numpy restatement of the batch",
             "   B  ratio  mode-1  dets  boxes |  mode 0 ms    full ms   added ms | detector ms  post+PnP ms  match+tgt ms |"
             " run_batch ms   numpy ms"]
    for B, ratio, n1, nd, nb, m in rows:
        lines.append("  %2d   %.1f   %5d  %4d  %5d |  %9.4f  %9.4f  %9.4f |   %9.4f    %9.4f     %9.4f |    %9.1f  %9.1f"
                     % (B, ratio, n1, nd, nb, m["mode0"], m["full"], m["full"] - m["mode0"], m["detector"], m["post"],
                        m["given"] - m["mode0"], m["run_batch"], m["numpy"]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
