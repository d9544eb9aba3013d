#!/usr/bin/env python
"""bench.py -- throughput of the CenterPose inference hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

K timed steps after W untimed ones; `ms_per_step` on the result line is the time of one timed step.  --dump-outputs DIR
writes what the last timed step returned (the decoded records; for the default workload also the post-processed records
and the poses) as DIR/<name>.npy; inputs and weights are seeded, so two builds can be compared output for output.

A plain run does only what the headline needs: set-up, warm-up, the timed steps, the dump, and the result line with the
`roofline` read from the timed steps' own launch events.  --full adds every measurement that takes runs of its own: the
batch-1 latencies, the nested `legs` and the `cpu_baseline` (see `extras`); without it those keys are null or a stub.

N > 1: the driver launches this file under `python -m torch.distributed.run --nproc-per-node N ...` (one rank per GPU,
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment); when it is started directly with --gpus N > 1 and no
WORLD_SIZE, it re-executes itself under torch.distributed.run on 127.0.0.1, so `python bench.py --gpus 8` alone is
enough.  One rank per GPU over RCCL (backend "nccl"); images shard by batch (weak scaling), and for N > 1 every step ends
with one all-gather of the detection records over xGMI (BASELINE configs[3]); `n_gpus` is the world size that actually
ran and `rccl_ranks` is read back from the process group after a real all-gather.

Headline workload (top-level line) = BASELINE.json configs[2], the largest single-GPU configuration and the only one
with the whole north-star chain: dla_34 at 512x512, batch 64 per GPU, synthetic Objectron-shaped frames, seeded
random-init weights -> backbone (DLA-34 + DCNv2 up-sampling + fused heads) -> sigmoid -> heat-map decode ->
post-process + soft-NMS -> PnP-input assembly -> batched PnP, everything on the device, no host synchronisation inside
a step.  One "step" = one batch through that chain, inputs resident in HBM before the timed region.

Extra objects on the ONE JSON line rank 0 prints (all but `roofline` with --full only):
  roofline      dominant kernel of the timed region: algorithmic FLOPs of its launches / their HIP-event durations
                (events recorded on the launch stream) vs the dense matrix peak of gfx950, plus the figures
                BASELINE.json's north_star names: roofline.dcn (DCNv2 + offset convolutions vs SURVEY 8(d)'s
                95.36 MB/img and the 8 TB/s HBM peak), roofline.conv1x1 (MFMA rate of the 1x1 convolutions),
                roofline.decode, roofline.pnp
  legs          (N = 1) short driver-timed runs of the other configurations in the same process: configs1 (BASELINE
                configs[1]: dlav1_34, batch 32, backbone + decode, with its own roofline), exact_f32 (the headline
                workload on the exact-f32 MFMA kernels), hourglass / track / track_gru (BASELINE configs[4] in both
                readings), track_e2e (B concurrent videos through the whole CenterPoseTrack loop
                incl. the host tracker: host fraction of a step)
  p50_frame_ms_batch1 / p50_frame_ms_batch1_network_decode
                p50 latency of one frame at batch 1 (frame resident in HBM -> results in HBM, network replayed from its
                hipGraph): the whole chain, and its network + sigmoid + decode share (the rest is the post-process and
                the PnP walk of that frame's detections)
  cpu_baseline  the reference's CPU path for the same workload timed on this host's cores (BASELINE.md section 3:
                3 warm-ups, >= 10 timed images, median): `value` = the reference as shipped (its own scalar
                single-thread deformable im2col, oracle/_ref, + torch CPU convolutions), `fair` = batches of 8 through the
                OpenMP port + torch CPU convolutions, per-stage seconds (the pure-Python PnP restatement apart)
  legs e2e_u8 / rendered_e2e
                the chain from 8-bit HWC frames (cp_preprocess_batch in the timer; PCIe-inclusive variant beside it) and the
                head-to-pose stage (decode + post-process + PnP) on rendered, well-posed Objectron-shaped heads
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from centerpose_amd import distributed as cpd  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md, dense f32 matrix
PEAK_F16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md, dense f16/bf16 matrix
PEAK_HBM_GBPS = 8000.0  # MI355X_MICROARCH.md, HBM3E
# the kernels of the DCN layers' offset / mask convolutions (32-wide N tile): patch-resident (halo16.hip) and row-streamed (strm16.hip)
OFFSET_CONV_KERNELS = ("halo16_f16x3_m128n32", "strm16_f16x3_w32n32")
DCN_MB_PER_IMG = 95.36  # sum over the 16 DCNv2 layers of (Cin + 27 + Cout) * HW * 4 + weights, 512x512
DECODE_MB_PER_IMG = 0.66  # one read of hm + hm_hp, gathers, 47 KB of records
GFLOP_PER_IMG = {"dlav1_34": 106.85, "dla_34": 85.11, "dla_34_track": 109.68,
                 "dlav1_34_track": 138.7, "hourglass": 603.7}  # BASELINE.md section 2, SURVEY 8(a) M9 / 8(f) N4
# hourglass: 739.2 GFLOP/img for the reference module minus the 135.3 of the first stack's seven heads, which do not
# feed model(x)[-1] (object_pose.py:135) and are not computed
DEFAULT_BATCH = {"full": 64, "decode": 32, "track": 16, "track_gru": 16, "hourglass": 8, "track_e2e": 16}
WORKLOAD_TEXT = {
    "full": "BASELINE configs[2]: dla_34 512x512 batch=%d/GPU, uniform-random uint8 frames through the seeded random-init network "
            "(about 26 detections/img above 0.3, mostly ill-posed PnP point sets; rendered-heads PnP figure: leg pnp_rendered), "
            "backbone + sigmoid + heat-map decode + post-process/soft-NMS + batched PnP, all on device",
    "decode": "BASELINE configs[1]: dlav1_34 512x512 batch=%d/GPU, synthetic random frames, backbone + sigmoid + heat-map decode",
    "track": "dla_34 512x512 batch=%d/GPU, two-frame CenterPoseTrack inputs, Gaussian-moment decode + all-gather of records",
    "track_gru": "BASELINE configs[4] as the reference can run it (SURVEY 8(f) N4 ii): dlav1_34 512x512 batch=%d/GPU, two-frame "
                 "inputs + ConvGRU heads, Gaussian-moment decode + all-gather of records",
    "hourglass": "BASELINE configs[4] as the reference defines it (N4 i): 2-stack hourglass 512x512 batch=%d/GPU, single frame, "
                 "backbone + decode",
    "track_e2e": "dla_34 512x512, %d concurrent videos, whole CenterPoseTrack loop per frame (render of the previous tracks, "
                 "two-frame network, decode, post-process, PnP, Gaussian fusion, Tracker.step); `value` = the device tracker, the host tracker beside it",
}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="full", choices=sorted(WORKLOAD_TEXT),
                    help="full (default): BASELINE configs[2]; decode: configs[1]; the others: see the `legs` of a --full run")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default: the configuration's)")
    ap.add_argument("--precision", default="f16x3", choices=["f32", "f16x3"],
                    help="f32: exact float32 MFMA; f16x3: split-binary16 MFMA (float32-class accuracy)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure the batch-1 latencies, the nested legs (other configurations and "
                         "precisions) and the reference's CPU baseline; a plain run skips them")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-legs", action="store_true", help="--full without the nested legs of the default workload")
    ap.add_argument("--no-latency", action="store_true", help="--full without the batch-1 latencies")
    ap.add_argument("--serial-pnp", action="store_true",
                    help="full: run the PnP solve on the network's stream (A/B against the side-stream default)")
    ap.add_argument("--dbg", type=int, default=0, help="cp_set_debug flags (kernel A/B switches, tuning only)")
    ap.add_argument("--dry-run", action="store_true",
                    help="plumbing rehearsal without a device: stub pipeline, real process group / barriers / all-gather "
                         "(tests/test_bench_cpu.py runs it with CP_BENCH_BACKEND=gloo, world size 2)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (float32 / float64, "
                         "at most 64 MB in all), for output-by-output comparison of two builds")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.workload == "track_e2e":
        ap.error("--dump-outputs: the track_e2e workload has no single step output (it times a host-in-the-loop video run)")
    return args


def extras(args, world, dry):
    """Which measurements rank 0 makes after the timed steps: none without --full (a plain run times the headline only)."""
    on = args.full and not dry
    return {"latency": on and not args.no_latency and args.workload in ("full", "decode", "hourglass"),
            "legs": on and world == 1 and args.workload == "full" and not args.no_legs,
            "cpu_baseline": on and world == 1 and not args.no_cpu_baseline}


def respawn_under_torchrun(args):
    """`python bench.py --gpus N` without a launcher: become `python -m torch.distributed.run ... bench.py <same argv>`."""
    port = int(os.environ.get("CP_BENCH_PORT", 29500 + os.getpid() % 2000))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL across processes)
    return subprocess.call(cmd, env=env)


class GatherTimer(object):
    """Time of the per-step detection all-gather on THIS rank (N > 1): HIP events on the stream the collective is issued on
    (device tensors), time.perf_counter around the blocking call otherwise (dry run over gloo).  Reported next to the step as
    the MAX over ranks of the per-rank mean, with the bytes a rank receives."""

    def __init__(self, device):
        self.device, self.pairs, self.host_s, self.bytes_out = device, [], [], 0

    def __call__(self, det):
        if self.device is None:
            t0 = time.perf_counter()
            out = cpd.allgather_detections(det)
            self.host_s.append(time.perf_counter() - t0)
        else:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = cpd.allgather_detections(det)
            e1.record()
            self.pairs.append((e0, e1))
        self.bytes_out = out.numel() * out.element_size()
        return out

    def reset(self):
        self.pairs, self.host_s = [], []

    def mean_ms(self):
        if self.device is not None:
            torch.cuda.synchronize()
            ts = [a.elapsed_time(b) for a, b in self.pairs]
        else:
            ts = [t * 1e3 for t in self.host_s]
        return sum(ts) / len(ts) if ts else None


class Pipeline(object):
    """frames -> heads -> detections [-> poses], all on device."""

    def __init__(self, workload, batch, device, seed, precision="f32", serial_pnp=False, gather=False):
        """``seed``: seed of this rank's FIRST image; image i of the shard is drawn from chunk seed ``seed + 8 * (i // 8)``, so that
        with seed = 317 + shard start (main) global image g is the same frame whatever the number of ranks."""
        from centerpose_amd import hip, synth

        self.hip = hip
        self.serial_pnp = serial_pnp
        self.gather = gather
        self.gather_timer = GatherTimer(device) if gather else None
        self.workload = workload
        self.arch = "dlav1_34" if workload in ("decode", "track_gru") else "hourglass" if workload == "hourglass" else "dla_34"
        self.track = workload in ("track", "track_gru")
        self.heads = synth.HEADS_TRACK if self.track else synth.HEADS_POSE
        self.batch = batch
        self.device = device
        sd = synth.make_state_dict(self.arch, self.heads, self.track)
        self.model = hip.HipModel(self.arch, self.heads, sd, tracking_task=self.track, precision=precision)
        self.extra = {}
        self._stages = {}
        self.last = None
        if self.track:  # previous frame + rendered previous heat-maps (base_detector.py:150-388)
            g = synth._gen(seed, "pre")
            self.extra = dict(
                pre_img=torch.cat([synth.frames(min(8, batch - i), seed=seed + 500 + i) for i in range(0, batch, 8)]).to(device),
                pre_hm=(torch.rand(batch, 1, 512, 512, generator=g) ** 16).to(device),
                pre_hm_hp=(torch.rand(batch, 8, 512, 512, generator=g) ** 16).to(device))
        # distinct frames per batch slot (generated in chunks of 8 to bound host memory)
        xs = [synth.frames(min(8, batch - i), seed=seed + i).to(device) for i in range(0, batch, 8)]
        self.x = torch.cat(xs, 0).contiguous()
        self.cam = torch.tensor([663.0287679036459, 663.0287679036459, 300.2775065104167, 395.00066121419275],
                                dtype=torch.float64, device=device).repeat(batch, 1).contiguous()  # demo.py:143-144
        # 512x512 frames, fix_res: c = (256, 256), s = 512 (base_detector.py:110-114) -> inverse affine grid -> image
        import numpy as np

        from centerpose_amd.lib.utils.image import get_affine_transform

        m = np.zeros((batch, 8))
        m[:, :6] = get_affine_transform(np.array([256.0, 256.0], np.float32), 512.0, 0, (128, 128), inv=1).reshape(-1)
        m[:, 6] = 512.0 / 128
        self.meta = torch.from_numpy(m).to(device)

    def step(self, x=None, graph=False):
        hip = self.hip
        if x is None:
            x, extra = self.x, self.extra
        else:
            extra = {k: v[: x.shape[0]] for k, v in self.extra.items()}
        if self.workload in ("decode", "hourglass"):
            # backbone + sigmoid + decode in one library call (hipGraph replay when graph=True)
            det = self.model.detect(x, K=100, rep_mode=1, fit_gaussian=False, balance=2.0, graph=graph)[1]
            return self.gather_timer(det) if self.gather else det
        if self.workload == "full":
            det = self.model.detect(x, K=100, rep_mode=1, fit_gaussian=False, balance=2.0, graph=graph)[1]
        else:
            z = self.model(x, sigmoid_hm=True, **extra)
            det = hip.decode_raw(z["hm"], z["hps"], z["wh"], z["hm_hp"], z["hps_uncertainty"], z["scale"],
                                 z["scale_uncertainty"], z["reg"], z["hp_offset"], z["tracking"], z["tracking_hp"],
                                 K=100, rep_mode=1, fit_gaussian=True, balance=2.0)
            # the tracker of every video needs all detections: one RCCL all-gather of the fixed-size records
            return self.gather_timer(det) if self.gather else cpd.allgather_detections(det)
        # configs[2]: post-process + soft-NMS (cp_postprocess), PnP input assembly for rep_mode 1 and the batched solve
        # (cp_pnp_from_post) -- library launches only, no torch indexing and no host synchronisation inside the step.
        # The solve (a few dozen latency-bound float64 wavefronts) is queued on hip.PoseStage's side stream and runs under
        # the next batch's network; every solve has finished before the timed region's closing device synchronisation.
        n = det.shape[0]
        if self.serial_pnp:
            post, cnt = hip.postprocess(det, self.meta[:n], 0.3, nms=True)
            poses = hip.pnp_from_post(post, cnt, self.cam[:n], rep_mode=1)
        else:
            stage = self._stages.get(n)
            if stage is None:
                stage = self._stages[n] = hip.PoseStage(n, det.shape[1], self.device, depth=2)
            post, cnt, poses, done = stage.submit(det, self.meta[:n], self.cam[:n], 0.3, nms=True, rep_mode=1)
        self.last = (post, cnt, poses)
        if self.gather:  # BASELINE configs[3]: every rank sees every image's detections
            return self.gather_timer(det), poses
        return det, poses

    def pnp_stats(self):
        """(ms per solve on its stream, detections solved in the last batch) for roofline.pnp."""
        st = self._stages.get(self.batch)
        ms = st.take_solve_ms() if st is not None else None
        n = None
        if self.last is not None:
            torch.cuda.synchronize()
            n = int(self.last[1].sum().item())
        return ms, n


class DryPipeline(object):
    """--dry-run: no device, no library; fixed-size records tagged with the rank (field 0), the device index the rank would bind
    (field 1 = LOCAL_RANK), the GLOBAL image index of the record's image (field 2 = shard start + i, the shard being
    distributed.shard_range of the global batch) and its slot (field 3), so that the gather order (rank, image, slot), the
    rank -> device mapping and the tiling of [0, global batch) by the shards can be checked."""

    def __init__(self, batch, rank, local=0, start=0, workload="full"):
        self.batch, self.rank = batch, rank
        self.arch, self.track, self.workload = "dla_34", workload in ("track", "track_gru"), workload
        self.det = torch.full((batch, 100, 118), float(rank), dtype=torch.float32)
        self.det[:, :, 1] = float(local)
        self.det[:, :, 2] = torch.arange(start, start + batch, dtype=torch.float32).view(batch, 1)
        self.det[:, :, 3] = torch.arange(100, dtype=torch.float32).view(1, 100)
        self.gathered = None
        self.gather_timer = GatherTimer(None)

    def step(self, x=None, graph=False):
        time.sleep(0.002)
        self.gathered = self.gather_timer(self.det)
        return self.gathered


def timed_region(pipe, steps, warmup, barrier, profile=True):
    """W untimed steps, then exactly `steps` timed ones between barriers; per-launch HIP events on every 4th step.  What the
    last timed step returned is left in ``pipe.last_out`` (--dump-outputs)."""
    for _ in range(warmup):
        pipe.step()
    every = 4 if steps >= 8 else 1
    sampled = 0
    barrier()
    if getattr(pipe, "gather_timer", None) is not None:
        pipe.gather_timer.reset()  # the warm-up steps' collectives (communicator bring-up) are not the steady state
    t0 = time.perf_counter()
    for i in range(steps):
        if profile:
            on = i % every == 0
            pipe.model.profile(on)
            sampled += int(on)
        out = pipe.step()
    barrier()
    dt = time.perf_counter() - t0
    pipe.last_out = out
    if not profile:
        return dt, {}, {}, 0
    pipe.model.profile(False)
    prof = pipe.model.profile_read()
    roles = pipe.model.profile_roles()
    return dt, prof, roles, sampled


def north_star_figures(roles, sampled, batch, precision):
    """roofline.dcn / conv1x1 / decode from the per-role event times (cp_model_profile_roles)."""
    out = {}
    per = lambda r: roles[r]["ms"] / sampled if r in roles else 0.0
    t_main, t_off = per("dcn"), per("dcn_offset")
    if t_main > 0:
        t = t_main + t_off
        gbps = DCN_MB_PER_IMG * batch / t  # MB / ms = GB/s
        out["dcn"] = {"bound": "hbm", "ms_per_step": round(t, 3), "main_ms": round(t_main, 3), "offset_conv_ms": round(t_off, 3),
                      "algorithmic_mb_per_img": DCN_MB_PER_IMG, "hbm_gbps": round(gbps, 1), "peak_gbps": PEAK_HBM_GBPS,
                      "frac_hbm": round(gbps / PEAK_HBM_GBPS, 4),
                      "main_only_hbm_gbps": round(DCN_MB_PER_IMG * batch / t_main, 1),
                      "tflops": round((roles["dcn"]["flops"] + roles.get("dcn_offset", {"flops": 0})["flops"]) /
                                      sampled / (t * 1e-3) / 1e12, 1),
                      "main_only_tflops": round(roles["dcn"]["flops"] / sampled / (t_main * 1e-3) / 1e12, 1)}
    peak = PEAK_F16_MFMA_TFLOPS if precision == "f16x3" else PEAK_F32_MFMA_TFLOPS
    names = ("conv1x1", "head_final")
    ms = sum(per(n) for n in names)
    if ms > 0:
        fl = sum(roles[n]["flops"] for n in names if n in roles) / sampled
        by = sum(roles[n]["bytes"] for n in names if n in roles) / sampled
        tf = fl / (ms * 1e-3) / 1e12
        out["conv1x1"] = {"bound": "mfma", "ms_per_step": round(ms, 3), "tflops": round(tf, 1), "peak_tflops": peak,
                          "mfma_utilisation": round(tf / peak, 4),
                          "issued_utilisation": round((3 if precision == "f16x3" else 1) * tf / peak, 4),
                          "algorithmic_gbps": round(by / 1e6 / ms, 1),
                          "launches_per_step": sum(roles[n]["launches"] for n in names if n in roles) // sampled}
    if "decode" in roles:
        us = per("decode") * 1e3
        out["decode"] = {"bound": "hbm", "us_per_step": round(us, 1), "algorithmic_mb_per_img": DECODE_MB_PER_IMG,
                         "hbm_gbps": round(DECODE_MB_PER_IMG * batch / (us * 1e-3), 1),
                         "floor_us_at_hbm_peak": round(DECODE_MB_PER_IMG * batch / PEAK_HBM_GBPS * 1e3, 2)}
    out["ms_per_step_by_role"] = {r: round(v["ms"] / sampled, 3) for r, v in roles.items()}
    return out


def roofline_object(prof, roles, sampled, batch, precision, workload=None):
    """`roofline` of the dominant kernel (largest share of HIP-event time inside the timed region).  `traffic` (HBM-side bytes
    per launch from the PMC passes under profiles/) is attached only when those passes profiled THIS workload at THIS batch
    (pmc_traffic.json: _meta); for every other leg it is null -- the counters of another shape say nothing about this one."""
    if not prof:
        return None
    name, r = max(prof.items(), key=lambda kv: kv[1]["ms"])
    achieved = r["flops"] / (r["ms"] * 1e-3) / 1e12
    total_ms = sum(v["ms"] for v in prof.values())
    is16 = "f16x3" in name
    peak = PEAK_F16_MFMA_TFLOPS if is16 else PEAK_F32_MFMA_TFLOPS
    roof = {"bound": "mfma", "kernel": name, "achieved": round(achieved, 3), "peak": peak,
            "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": None,
            "note": ("algorithmic FLOPs; each is executed as 3 binary16 MFMA products (hi*hi + hi*lo + lo*hi), so "
                     "the matrix pipe does 3x this work: issued rate %.0f TFLOP/s = %.3f of the f16 peak" % (
                         3 * achieved, 3 * achieved / peak)) if is16 else "exact float32 MFMA",
            "launches_per_step": r["launches"] // sampled,
            "timed_steps_sampled": sampled,
            "avg_launch_us": round(r["ms"] * 1e3 / r["launches"], 2),
            "flops_per_launch": r["flops"] / r["launches"],
            "algorithmic_bytes_per_launch": r["bytes"] / r["launches"],
            "share_of_conv_time": round(r["ms"] / total_ms, 4),
            "all_conv_kernels": {k: {"tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2),
                                     "ms_per_step": round(v["ms"] / sampled, 3),
                                     "launches_per_step": v["launches"] // sampled}
                                 for k, v in prof.items()},
            "conv_ms_per_step": round(total_ms / sampled, 3)}
    roof.update(north_star_figures(roles, sampled, batch, precision))
    tr = os.path.join(REPO, "profiles", "pmc_traffic.json")
    if os.path.exists(tr):
        with open(tr) as f:
            pmc = json.load(f)
        meta = pmc.get("_meta", {})
        t = pmc.get(name)
        if t and meta.get("workload") == workload and meta.get("batch") == batch and meta.get("precision", "f16x3") == precision:
            # HBM-side bytes per launch from the rocprofv3 PMC passes of profiles/ (FETCH_SIZE x2 + WRITE_SIZE)
            roof["traffic"] = t["hbm_bytes_per_launch"]
            roof["traffic_source"] = "profiles/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE of `%s`)" % meta.get("command", "bench.py")
            if "dcn" in roof:
                # the DCN pair's counter bytes per step: every DCN main kernel that ran + the offset convolutions (OFFSET_CONV_KERNELS),
                # each kernel's PMC bytes per launch x its launches per step in THIS run
                tot, main, missing = 0.0, 0.0, []
                for k, v in prof.items():
                    if k.startswith(("dcn16", "dcn_igemm16")) or k in OFFSET_CONV_KERNELS:
                        if k in pmc:
                            b = pmc[k]["hbm_bytes_per_launch"] * (v["launches"] / sampled)
                            tot += b
                            main += b if k not in OFFSET_CONV_KERNELS else 0.0
                        else:
                            missing.append(k)
                if tot > 0 and not missing:
                    # (the algorithmic figure counts a layer's input once; the offset convolution is a second kernel over it)
                    roof["dcn"]["traffic"] = round(tot)
                    roof["dcn"]["traffic_over_algorithmic"] = round(tot / (DCN_MB_PER_IMG * 1e6 * batch), 3)
                    roof["dcn"]["traffic_main_kernels"] = round(main)
        else:
            roof["traffic_note"] = "no PMC pass of this workload / batch under profiles/ (pmc_traffic.json profiled %s at batch %s)" % (
                meta.get("workload"), meta.get("batch"))
    return roof


def frame_latency(pipe, n=50):
    """p50 per-frame latency at batch 1: frame already in HBM -> results in HBM, network replayed from a hipGraph."""
    x1 = pipe.x[:1].contiguous()
    for _ in range(3):
        pipe.step(x1, graph=True)
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t1 = time.perf_counter()
        pipe.step(x1, graph=True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t1) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 3)


def detect_latency(pipe, n=30):
    """The same frame through the network + sigmoid + decode only (cp_model_detect from its hipGraph): what is left of
    `frame_latency` is the post-process and the PnP walk, which on random-weight (ill-posed) detections runs its full
    20 Levenberg-Marquardt iterations (profiles/NOTES.md)."""
    x1 = pipe.x[:1].contiguous()
    det = lambda: pipe.model.detect(x1, K=100, rep_mode=1, fit_gaussian=False, balance=2.0, graph=True)
    for _ in range(3):
        det()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t1 = time.perf_counter()
        det()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t1) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 3)


def run_leg(workload, device, precision, steps, warmup, barrier, latency, serial_pnp=False):
    """One nested leg of the default run: a short timed region of another configuration, same harness."""
    batch = DEFAULT_BATCH[workload]
    pipe = Pipeline(workload, batch, device, seed=317, precision=precision, serial_pnp=serial_pnp)
    dt, prof, roles, sampled = timed_region(pipe, steps, warmup, barrier)
    key = pipe.arch + ("_track" if pipe.track else "")
    out = {"workload": WORKLOAD_TEXT[workload] % batch, "precision": precision,
           "value": round(batch * steps / dt, 2), "unit": "images/sec", "steps": steps, "warmup": warmup,
           "ms_per_step": round(dt / steps * 1e3, 3),
           "whole_step_tflops": round(batch * steps / dt * GFLOP_PER_IMG[key] / 1e3, 2),
           "roofline": roofline_object(prof, roles, sampled, batch, precision, workload)}
    if latency and workload in ("full", "decode", "hourglass"):
        out["p50_frame_ms_batch1"] = frame_latency(pipe, 30)
    del pipe
    torch.cuda.empty_cache()
    return out


def _event_ms(fn, n, warm=3, chunks=5):
    """HIP-event milliseconds per call of `fn` on torch's current stream: n calls after `warm`, timed in `chunks` groups, the
    median group's average (these legs are tens of microseconds per call, i.e. bounded by how fast the host issues the
    launches: one 30 ms stall of the host inside 50 calls once turned 43 us into 674)."""
    for _ in range(warm):
        fn()
    per = max(1, n // chunks)
    times = []
    for _ in range(chunks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / per)
    times.sort()
    return times[len(times) // 2]


def decode_only_leg(device, precision, batch=32):
    """BASELINE configs[1] as SURVEY 8(d) defines it: dlav1_34 heads, batch 32, ONLY cp_decode inside the timer, on (i) head
    tensors drawn directly (hm / hm_hp = rand()**8, ...) and (ii) the post-sigmoid heads the dlav1_34 forward produces from
    the random frames.  Roofline: HBM, 0.66 MB/img of algorithmic traffic (one read of hm + hm_hp, the gathers, the records)."""
    from centerpose_amd import hip, synth

    def dec(z):
        return lambda: hip.decode_raw(z["hm"], z["hps"], z["wh"], z["hm_hp"], None, z["scale"], None, z["reg"], z["hp_offset"],
                                      None, None, K=100, rep_mode=1)

    def obj(ms):
        gbps = DECODE_MB_PER_IMG * batch / ms  # MB / ms = GB/s
        return {"us_per_batch": round(ms * 1e3, 2), "images_per_sec": round(batch / (ms * 1e-3), 1),
                "roofline": {"bound": "hbm", "kernel": "peaks_kernel + assoc_kernel", "achieved": round(gbps, 1), "peak": PEAK_HBM_GBPS,
                             "unit": "GB/s", "frac": round(gbps / PEAK_HBM_GBPS, 5), "traffic": None,
                             "algorithmic_mb_per_img": DECODE_MB_PER_IMG,
                             "floor_us_at_hbm_peak": round(DECODE_MB_PER_IMG * batch / PEAK_HBM_GBPS * 1e3, 2)}}

    drawn = {k: v.to(device).contiguous() for k, v in synth.drawn_heads(batch, seed=317).items()}
    out = {"workload": "BASELINE configs[1] (SURVEY 8(d)): dlav1_34 heads 128x128, batch=%d, cp_decode only inside the timer" % batch,
           "drawn_heads": obj(_event_ms(dec(drawn), 50))}
    del drawn
    model = hip.HipModel("dlav1_34", synth.HEADS_POSE, synth.make_state_dict("dlav1_34", synth.HEADS_POSE, False), precision=precision)
    x = torch.cat([synth.frames(8, seed=317 + i).to(device) for i in range(0, batch, 8)])
    z = {k: v.contiguous() for k, v in model(x, sigmoid_hm=True).items()}
    out["network_heads"] = obj(_event_ms(dec(z), 50))
    out["value"], out["unit"] = out["network_heads"]["images_per_sec"], "images/sec (decode only)"
    out["ms_per_step"] = round(out["network_heads"]["us_per_batch"] / 1e3, 5)
    del model, x, z
    torch.cuda.empty_cache()
    return out


def pnp_rendered_leg(device, batch=64):
    """The pose stage on Objectron-shaped heads (1-10 known cuboids per image rendered the way the reference
    builds its ground truth): decode -> post-process + soft-NMS -> PnP-input assembly -> batched solve, the figure to put beside
    the headline's random-weight detections (about 26 per image, mostly ill-posed point sets whose Levenberg-Marquardt walk
    runs its full 20 iterations)."""
    import numpy as np

    from centerpose_amd import hip, synth
    from centerpose_amd.lib.utils.image import get_affine_transform

    heads, counts = synth.rendered_heads(batch, seed=317)
    z = {k: v.to(device).contiguous() for k, v in heads.items()}
    cam = torch.tensor([663.0287679036459, 663.0287679036459, 300.2775065104167, 395.00066121419275], dtype=torch.float64,
                       device=device).repeat(batch, 1).contiguous()
    m = np.zeros((batch, 8))
    m[:, :6] = get_affine_transform(np.array([256.0, 256.0], np.float32), 512.0, 0, (128, 128), inv=1).reshape(-1)
    m[:, 6] = 512.0 / 128
    meta = torch.from_numpy(m).to(device)
    det = hip.decode_raw(z["hm"], z["hps"], z["wh"], z["hm_hp"], None, z["scale"], None, z["reg"], z["hp_offset"], None, None,
                         K=100, rep_mode=1)
    state = {}

    def stage():
        post, cnt = hip.postprocess(det, meta, 0.3, nms=True)
        state["cnt"], state["poses"] = cnt, hip.pnp_from_post(post, cnt, cam, rep_mode=1)

    ms = _event_ms(stage, 20)
    n = int(state["cnt"].sum().item())

    def chain():  # the whole head-to-pose stage on well-posed detections: decode -> post-process + soft-NMS -> assembly -> solve
        d = hip.decode_raw(z["hm"], z["hps"], z["wh"], z["hm_hp"], None, z["scale"], None, z["reg"], z["hp_offset"], None, None,
                           K=100, rep_mode=1)
        post, cnt = hip.postprocess(d, meta, 0.3, nms=True)
        state["cnt2"], state["poses2"] = cnt, hip.pnp_from_post(post, cnt, cam, rep_mode=1)

    ms2 = _event_ms(chain, 20)
    n2 = int(state["cnt2"].sum().item())
    e2e = {"workload": "Objectron-shaped rendered heads (1-10 cuboids per image), batch=%d: cp_decode + post-process + soft-NMS + "
                       "PnP inside the timer (the head-to-pose stage of configs[2] on well-posed detections)" % batch,
           "objects_rendered": int(sum(counts)), "detections_solved": n2, "ms_per_step": round(ms2, 3),
           "value": round(batch / (ms2 * 1e-3), 1), "unit": "images/sec (decode + post-process + PnP)"}
    return {"workload": "Objectron-shaped rendered heads (1-10 cuboids per image), batch=%d: post-process + soft-NMS + PnP" % batch,
            "objects_rendered": int(sum(counts)), "detections_solved": n, "ms_per_batch": round(ms, 3),
            "value": round(n / (ms * 1e-3), 1), "unit": "detections/sec (post-process + PnP)", "ms_per_step": round(ms, 3)}, e2e


def e2e_u8_leg(device, precision, steps, warmup, barrier, batch=64):
    """SURVEY 8(f) N1 inside the timed chain: what BaseDetector.run() starts from (base_detector.py:91-148) -- 8-bit HWC BGR
    frames -> cp_preprocess_batch (warp + normalise on the device) -> the headline chain (network, decode, post-process, PnP).
    Two figures: frames resident in HBM as uint8 (`value`), and frames in pinned HOST memory copied over PCIe every step on a
    copy stream, double-buffered against the previous batch's compute (`pcie_inclusive`)."""
    import numpy as np

    from centerpose_amd import hip, synth
    from centerpose_amd.lib.utils.image import get_affine_transform

    pipe = Pipeline("full", batch, device, seed=317, precision=precision)
    u8_host = torch.cat([synth.frames_u8(min(8, batch - i), seed=317 + i) for i in range(0, batch, 8)]).contiguous().pin_memory()
    trans = get_affine_transform(np.array([256.0, 256.0], np.float32), 512.0, 0, [512, 512])  # fix_res, 512 x 512 frames
    xbuf = torch.empty(batch, 3, 512, 512, device=device, dtype=torch.float32)

    def step(u8):
        hip.preprocess_batch(u8, trans, synth.MEAN, synth.STD, 512, 512, out=xbuf)
        return pipe.step(xbuf)

    u8_dev = u8_host.to(device)
    for _ in range(warmup):
        step(u8_dev)
    # ONE timed pass of `steps`, the protocol of the headline, of every other leg and of pcie_inclusive below (round 5 reported the
    # faster of two passes here, which biased the comparison with them)
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(u8_dev)
    barrier()
    dt = time.perf_counter() - t0
    pre_ms = _event_ms(lambda: hip.preprocess_batch(u8_dev, trans, synth.MEAN, synth.STD, 512, 512, out=xbuf), 20)
    # PCIe-inclusive: batch i + 1 crosses the bus on the copy stream while batch i computes
    cur, cs = torch.cuda.current_stream(), torch.cuda.Stream(device=device)
    bufs = [torch.empty_like(u8_dev), torch.empty_like(u8_dev)]
    copied = [torch.cuda.Event(), torch.cuda.Event()]
    consumed = [None, None]

    def fetch(j):
        with torch.cuda.stream(cs):
            if consumed[j] is not None:
                cs.wait_event(consumed[j])
            bufs[j].copy_(u8_host, non_blocking=True)
            copied[j].record(cs)

    fetch(0)
    dt_pcie = None
    for i in range(warmup + steps):
        if i == warmup:
            barrier()
            t0 = time.perf_counter()
        j = i & 1
        fetch(j ^ 1)
        cur.wait_event(copied[j])
        step(bufs[j])
        consumed[j] = torch.cuda.Event()
        consumed[j].record(cur)
    barrier()
    dt_pcie = time.perf_counter() - t0
    out = {"workload": "uint8 HWC frames (B = %d, 512 x 512) -> cp_preprocess_batch -> the headline chain (network, decode, "
                       "post-process, PnP)" % batch, "precision": precision,
           "value": round(batch * steps / dt, 2), "unit": "images/sec", "steps": steps, "warmup": warmup,
           "timed_passes": 1, "ms_per_step": round(dt / steps * 1e3, 3), "preprocess_ms_per_batch": round(pre_ms, 3),
           "preprocess_gbps": round(batch * (512 * 512 * 3 + 512 * 512 * 12) / 1e6 / pre_ms, 1),
           "pcie_inclusive": {"value": round(batch * steps / dt_pcie, 2), "unit": "images/sec", "ms_per_step": round(dt_pcie / steps * 1e3, 3),
                              "host_mb_per_step": round(u8_host.numel() / 1e6, 1),
                              "note": "pinned host frames, one copy per step on a copy stream, double-buffered"}}
    del pipe, bufs, u8_dev, xbuf
    torch.cuda.empty_cache()
    return out


def track_e2e_leg(device, precision, n_videos, frames, warmup):
    """B concurrent videos through CenterPoseTrack's whole per-frame loop (lib/detectors/batch_tracking.py): what the
    host-side tracker costs next to the batched device stages."""
    import contextlib
    import io
    import tempfile

    import numpy as np

    from centerpose_amd import synth
    from centerpose_amd.lib.detectors.batch_tracking import BatchedTracking
    from centerpose_amd.lib.detectors.detector_factory import detector_factory
    from centerpose_amd.lib.models.model import create_model, save_model
    from centerpose_amd.lib.opts import opts
    from centerpose_amd.lib.utils.image import get_affine_transform

    with contextlib.redirect_stdout(io.StringIO()):
        o = opts().parser.parse_args(["--tracking_task", "--arch", "dla_34", "--c", "cup", "--debug", "0"])
        o.nms, o.obj_scale, o.use_pnp = True, True, True           # src/demo.py:111-149
        o.pre_img = o.pre_hm = o.tracking = o.pre_hm_hp = o.tracking_hp = True
        o.track_thresh = 0.1
        o.obj_scale_uncertainty = o.hps_uncertainty = o.kalman = o.scale_pool = True
        o.vis_thresh = max(o.track_thresh, o.vis_thresh)
        o.pre_thresh = max(o.track_thresh, o.pre_thresh)
        o.new_thresh = max(o.track_thresh, o.new_thresh)
        o.precision = precision
        o = opts().init(opts().parse(o))
        sd = synth.make_state_dict("dla_34", o.heads, True)
        with tempfile.TemporaryDirectory() as td:
            ck = os.path.join(td, "synthetic_dla_34_track.pth")
            m = create_model(o.arch, o.heads, o.head_conv, o)
            m.load_state_dict(sd, strict=True)
            save_model(ck, 1, m)
            o.load_model = ck
            det = detector_factory[o.task](o)
    c, s = np.array([256.0, 256.0], np.float32), 512.0
    K = np.array([[663.0287679036459, 0, 300.2775065104167], [0, 663.0287679036459, 395.00066121419275], [0, 0, 1]])
    meta = {"c": c, "s": s, "height": 512, "width": 512, "out_height": 128, "out_width": 128, "inp_height": 512,
            "inp_width": 512, "trans_input": get_affine_transform(c, s, 0, [512, 512]),
            "trans_output": get_affine_transform(c, s, 0, [128, 128]), "camera_matrix": K}
    vids = [torch.cat([synth.frames(min(8, n_videos - i), seed=4000 + 100 * f + i) for i in range(0, n_videos, 8)]).to(device)
            for f in range(4)]  # four distinct frames per video, cycled
    # Objectron-shaped load: a handful of objects per video (the dataset caps at max_objs = 10).  The random-init network
    # scores ~55 peaks per frame above 0.1, so the thresholds are set to the score that keeps about 4 per video.
    with contextlib.redirect_stdout(io.StringIO()):
        det._skip_host_dets = True
        det.process(vids[0], vids[0], torch.zeros(n_videos, 1, 512, 512, device=device),
                    torch.zeros(n_videos, 8, 512, 512, device=device), None)
        det._skip_host_dets = False
    scores = det.raw_dets[..., 4].flatten().sort(descending=True).values
    thr = float(scores[min(4 * n_videos, scores.numel() - 1)])
    o.vis_thresh = o.pre_thresh = o.new_thresh = o.track_thresh = thr
    metas = lambda f: [dict(meta, id=f) for _ in range(n_videos)]
    res = {}
    for mode in ("host", "device"):
        bt = BatchedTracking(det, n_videos, device_tracker=(mode == "device"))
        n_tracks = 0
        with contextlib.redirect_stdout(io.StringIO()):
            for f in range(warmup + frames):
                if f == warmup:
                    torch.cuda.synchronize()
                    bt.times = {k: 0 if k == "steps" else 0.0 for k in bt.times}
                    t0 = time.perf_counter()
                outs = bt.step(vids[f % 4], metas(f), read=(mode == "host"))
                if outs is not None:
                    n_tracks = sum(len(x["results"]) for x in outs)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        t = bt.times
        tot = t["host_records"] + t["device"] + t["host_tracks"]
        res[mode] = {"frames_per_sec": round(n_videos * frames / dt, 2), "ms_per_step": round(dt / frames * 1e3, 3),
                     "ms_device_stages": round(t["device"] / frames * 1e3, 3),
                     "ms_host_records": round(t["host_records"] / frames * 1e3, 3),
                     "ms_host_tracker": round(t["host_tracks"] / frames * 1e3, 3),
                     "host_fraction": round((t["host_records"] + t["host_tracks"]) / tot, 4)}
        if mode == "host":
            res[mode]["tracks_alive_last_frame"] = n_tracks
        else:
            res[mode]["tracks_alive_last_frame"] = sum(len(a) for a in bt.dev.read())
        del bt
    out = {"workload": WORKLOAD_TEXT["track_e2e"] % n_videos, "precision": precision,
           "value": res["device"]["frames_per_sec"], "unit": "frames/sec (all videos)", "steps": frames, "warmup": warmup,
           "ms_per_step": res["device"]["ms_per_step"], "host_fraction": res["device"]["host_fraction"],
           "detection_threshold": round(thr, 4),
           "device_tracker": res["device"], "host_tracker": res["host"],
           "note": "device_tracker: render of the previous tracks + two-frame network + decode + post-process + PnP + "
                   "cp_track_step (fusion, association, Kalman filter, scale pool, filtered PnP, next frame's Gaussian "
                   "records) as one launch sequence, no host work inside a step (the tracks stay in HBM); host_tracker: the "
                   "same loop with the reference-shaped Python Tracker per video (Gaussian-record building, detection "
                   "dicts, fusion, pnp_shell packaging, Tracker.step with one cp_pnp_solve round trip per track)"}
    del det
    torch.cuda.empty_cache()
    return out


def cpu_baseline(workload, arch, budget_s=45.0, n_timed=10, n_warm=3):
    """The reference's CPU path on a bounded sample of the same workload (3 warm-ups, >= 10 timed
    images, median).  Both legs run the oracle's restatement of the reference graph (torch CPU convolutions on all
    cores) + numpy decode (+ for configs[2] the host post-process and the float64 PnP restatement per detection); they
    differ in the deformable im2col: `value` = the reference's own scalar single-thread source as shipped
    (oracle/_ref, kind "reference"; this repo's C port pinned to one thread where that binary is absent), `fair` = the C
    port with OpenMP over all cores."""
    if workload not in ("full", "decode"):
        return None
    import statistics

    import numpy as np

    from centerpose_amd import synth
    from oracle import backbone as ob
    from oracle import dcn as odcn
    from oracle import decode as odec
    from oracle import pnp as opnp

    heads = synth.HEADS_POSE
    sd = synth.make_state_dict(arch, heads, False)
    cores = torch.get_num_threads()
    Kmat = np.array([[663.0287679036459, 0, 300.2775065104167], [0, 663.0287679036459, 395.00066121419275], [0, 0, 1]])
    n_pnp = []

    def one(i, kind):
        x = synth.frames(1, seed=1000 + i)
        t1 = time.perf_counter()
        z = ob.dlaseg_forward(sd, x, heads, arch=arch.split("_")[0], dcn_kind=kind)
        hm = torch.sigmoid(z["hm"]).numpy()
        hm_hp = torch.sigmoid(z["hm_hp"]).numpy()
        d = odec.object_pose_decode(hm, z["hps"].numpy(), wh=z["wh"].numpy(), obj_scale=z["scale"].numpy(),
                                    reg=z["reg"].numpy(), hm_hp=hm_hp, hp_offset=z["hp_offset"].numpy(), K=100,
                                    rep_mode=1)
        if workload == "full":  # the PnP of every detection above vis_thresh (x4: 128-grid -> 512 image, fix_res)
            keep = np.nonzero(d["scores"][0, :, 0] > 0.3)[0]
            for k in keep:
                pts = np.hstack((d["kps_displacement_mean"][0, k].reshape(8, 2), d["kps_heatmap_mean"][0, k].reshape(8, 2)))
                pts = np.where(pts < -5000, pts, pts * 4.0).reshape(-1, 2)
                opnp.solve_cuboid_pnp(pts, d["obj_scale"][0, k].astype(np.float64), Kmat)
            n_pnp.append(len(keep))
        return time.perf_counter() - t1

    def leg(kind, budget):
        for w in range(n_warm):  # warm-ups: page-in, thread pools, im2col scratch
            one(w, kind)
        ts, t0 = [], time.perf_counter()
        while len(ts) < n_timed or (time.perf_counter() - t0 < budget and len(ts) < 2 * n_timed):
            ts.append(one(n_warm + len(ts), kind))
            if time.perf_counter() - t0 > 4 * budget:
                break  # stated budget: a slow host stops after 4x the budget even below n_timed images
        ts.sort()
        return ts

    def describe(ts, what):
        med = statistics.median(ts)
        return med, ("%d timed images after %d warm-ups, %s; median %.3f s/img (p50), p95 %.3f, min %.3f" % (
            len(ts), n_warm, what, med, ts[min(len(ts) - 1, int(0.95 * len(ts)))], ts[0]))

    kind = "reference" if odcn.have_reference() else "port"
    omp = None
    if kind == "port":
        try:
            import ctypes

            omp = ctypes.CDLL("libgomp.so.1")
            omp.omp_set_num_threads(1)
        except OSError:
            omp = None
    shipped = leg(kind, budget_s)
    med, text = describe(shipped, "scalar single-thread deformable im2col (%s) + torch CPU convolutions on %d threads + numpy "
                                  "decode%s" % ("the reference's own dcn_v2_im2col_cpu.cpp, oracle/_ref" if kind == "reference"
                                                else "this repo's C port pinned to 1 thread", cores,
                                                " + float64 PnP restatement" if workload == "full" else ""))
    out = {"value": round(1.0 / med, 4), "unit": "images/sec", "cores": cores, "kind": kind, "sample": text,
           "protocol": "BASELINE.md section 3: %d warm-ups, >= %d timed images (budget %.0f s), median" % (n_warm, n_timed, budget_s)}
    if omp is not None:
        omp.omp_set_num_threads(cores)
    if n_pnp:
        out["pnp_detections_per_image"] = round(sum(n_pnp) / len(n_pnp), 2)
    # `fair`: what the same host does when it is used the way a CPU deployment would use it -- batches of 8 through the torch CPU
    # convolutions (all cores inside every operator) with the OpenMP port of the im2col, stage by stage, so that the pure-Python
    # float64 PnP restatement (a cost of the ORACLE, not of the reference's cv2.solvePnP) is reported separately
    FB = 8

    def one_batch(i):
        x = torch.cat([synth.frames(1, seed=2000 + FB * i + k) for k in range(FB)])
        t1 = time.perf_counter()
        z = ob.dlaseg_forward(sd, x, heads, arch=arch.split("_")[0], dcn_kind="port")
        t2 = time.perf_counter()
        hm, hm_hp = torch.sigmoid(z["hm"]).numpy(), torch.sigmoid(z["hm_hp"]).numpy()
        d = odec.object_pose_decode(hm, z["hps"].numpy(), wh=z["wh"].numpy(), obj_scale=z["scale"].numpy(), reg=z["reg"].numpy(),
                                    hm_hp=hm_hp, hp_offset=z["hp_offset"].numpy(), K=100, rep_mode=1)
        t3 = time.perf_counter()
        if workload == "full":
            for b in range(FB):
                for k in np.nonzero(d["scores"][b, :, 0] > 0.3)[0]:
                    pts = np.hstack((d["kps_displacement_mean"][b, k].reshape(8, 2), d["kps_heatmap_mean"][b, k].reshape(8, 2)))
                    pts = np.where(pts < -5000, pts, pts * 4.0).reshape(-1, 2)
                    opnp.solve_cuboid_pnp(pts, d["obj_scale"][b, k].astype(np.float64), Kmat)
        t4 = time.perf_counter()
        return t2 - t1, t3 - t2, t4 - t3

    one_batch(0)  # warm-up
    rows, t0 = [], time.perf_counter()
    while len(rows) < 2 or (time.perf_counter() - t0 < budget_s / 2 and len(rows) < 6):
        rows.append(one_batch(1 + len(rows)))
    med = lambda c: statistics.median(r[c] for r in rows) / FB
    net, dec, pnp = med(0), med(1), med(2)
    out["fair"] = {"value": round(1.0 / (net + dec + pnp), 4), "unit": "images/sec", "kind": "port", "cores": cores, "batch": FB,
                   "value_network_decode_only": round(1.0 / (net + dec), 4),
                   "stages_s_per_image": {"network (torch CPU convolutions + OpenMP im2col)": round(net, 4), "decode (numpy)": round(dec, 4),
                                          "pnp (pure-Python float64 restatement)": round(pnp, 4)},
                   "sample": "%d timed batches of %d images after 1 warm-up batch, median per stage" % (len(rows), FB)}
    return out


def compact_line(d):
    """The ONE JSON line: every leg and every north-star figure, without the per-kernel tables and the long notes (those go to
    the detail file written beside it) -- the driver keeps an 8 KB tail of stdout, and the round-3 line (> 8 KB) lost four legs."""
    def roof(r, full):
        if not r:
            return None
        keep = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic")
        if full:
            keep += ("avg_launch_us", "launches_per_step", "flops_per_launch", "algorithmic_bytes_per_launch", "share_of_conv_time",
                     "conv_ms_per_step", "timed_steps_sampled")
        o = {k: r[k] for k in keep if k in r}
        sub = {"dcn": ("ms_per_step", "main_ms", "offset_conv_ms", "hbm_gbps", "frac_hbm", "tflops", "traffic", "traffic_over_algorithmic", "traffic_main_kernels"),
               "conv1x1": ("tflops", "mfma_utilisation", "algorithmic_gbps"), "decode": ("us_per_step", "hbm_gbps"),
               "pnp": ("ms_per_batch_on_side_stream", "detections_last_batch")}
        for name, ks in sub.items():
            if name in r and (full or name == "dcn"):
                o[name] = {k: r[name][k] for k in (ks if full else ("ms_per_step", "frac_hbm")) if k in r[name]}
        return o

    def leg(v):
        if v is None or "error" in v:
            return v
        o = {k: v[k] for k in ("value", "unit", "ms_per_step", "steps", "p50_frame_ms_batch1", "host_fraction") if k in v}
        if v.get("roofline"):
            o["roofline"] = roof(v["roofline"], False)
        for k in ("drawn_heads", "network_heads"):  # decode_only
            if k in v:
                o[k] = {"us_per_batch": v[k]["us_per_batch"], "roofline": roof(v[k]["roofline"], False)}
        for k in ("detections_solved", "objects_rendered", "preprocess_ms_per_batch"):  # pnp_rendered / rendered_e2e / e2e_u8
            if k in v:
                o[k] = v[k]
        if "pcie_inclusive" in v:  # e2e_u8
            o["pcie_inclusive"] = {k: v["pcie_inclusive"][k] for k in ("value", "ms_per_step")}
        if "host_tracker" in v:  # track_e2e
            o["host_tracker_frames_per_sec"] = v["host_tracker"]["frames_per_sec"]
        return o

    out = {k: v for k, v in d.items() if k not in ("roofline", "legs", "cpu_baseline")}
    out["roofline"] = roof(d.get("roofline"), True)
    out["legs"] = {k: leg(v) for k, v in d["legs"].items()} if d.get("legs") else None
    c = d.get("cpu_baseline")
    if c and "value" in c:
        out["cpu_baseline"] = {k: c[k] for k in ("value", "unit", "cores", "kind") if k in c}
        out["cpu_baseline"]["sample"] = c["sample"][:160]
        if "fair" in c:
            out["cpu_baseline"]["fair_value"] = c["fair"]["value"]
            out["cpu_baseline"]["fair_network_decode_only"] = c["fair"].get("value_network_decode_only")
        if "pnp_detections_per_image" in c:
            out["cpu_baseline"]["pnp_detections_per_image"] = c["pnp_detections_per_image"]
    else:
        out["cpu_baseline"] = c
    return out


def write_detail(d):
    """The full record of the run (per-kernel tables, notes, every leg's roofline object) beside the compact line."""
    path = os.environ.get("CP_BENCH_DETAIL")
    if not path:
        # never a committed file: profiles/ holds the recorded runs, build/ is git-ignored
        scratch = os.path.join(REPO, "gpurun_out")
        path = os.path.join(scratch if os.path.isdir(scratch) else os.path.join(REPO, "build"), "bench_detail_last.json")
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(d, f, indent=1)
        return os.path.relpath(path, REPO)
    except OSError:
        return None


DUMP_BYTES_MAX = 64 << 20


def dump_outputs(pipe, path):
    """--dump-outputs DIR: what the last timed step handed its caller, as DIR/<name>.npy.  Every workload: `detections`, the
    decoded records [B, 100, 118] (all ranks' after the per-step all-gather when N > 1).  full: also the pose stage's results,
    `counts` [B] and the first counts[b] rows of `post` [B, 100, 120] and `poses` [B, 100, 40]; the rows past the count are
    not part of the result (reused buffers) and are written as zeros.  Integers are written as float64.  Should the whole
    exceed DUMP_BYTES_MAX, every array keeps the same fixed, seeded sample of its leading-axis rows (`sample_rows.npy`)."""
    import numpy as np

    out = pipe.last_out
    det = out[0] if isinstance(out, tuple) else out
    arrays = {"detections": det}
    last = getattr(pipe, "last", None)
    if pipe.workload == "full" and last is not None:
        post, cnt, poses = last
        valid = torch.arange(post.shape[1], device=cnt.device).view(1, -1) < cnt.view(-1, 1).long()
        arrays["counts"] = cnt
        arrays["post"] = torch.where(valid.unsqueeze(-1), post, torch.zeros((), dtype=post.dtype, device=post.device))
        arrays["poses"] = torch.where(valid.unsqueeze(-1), poses, torch.zeros((), dtype=poses.dtype, device=poses.device))
    if torch.cuda.is_available() and det.is_cuda:
        torch.cuda.synchronize()
    arrays = {k: v.detach().cpu().numpy() for k, v in arrays.items()}
    arrays = {k: v if v.dtype in (np.float32, np.float64) else v.astype(np.float64) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_BYTES_MAX:
        n = det.shape[0]
        keep = max(1, int(n * DUMP_BYTES_MAX // total))
        rows = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        arrays = {k: v[rows] for k, v in arrays.items()}
        arrays["sample_rows"] = rows.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(v))
    return sorted(arrays)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(respawn_under_torchrun(args))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dry = args.dry_run
    backend = os.environ.get("CP_BENCH_BACKEND", "nccl")
    if not dry and not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (there is no CPU path)")
    device = None
    if not dry:
        # one GPU per rank; ($CP_BENCH_BACKEND=gloo with fewer GPUs than ranks is a plumbing rehearsal on a 1-GPU box)
        ndev = torch.cuda.device_count()
        if world > ndev and backend == "nccl":
            raise SystemExit("bench.py: %d ranks but %d visible GPUs (RCCL needs one GPU per rank)" % (world, ndev))
        local = local % ndev
        torch.cuda.set_device(local)
        device = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist

        cpd.init_from_env(backend)
    if rank == 0 and args.gpus != world:
        print("bench.py: --gpus %d but the launcher started %d rank(s); n_gpus reports %d" % (args.gpus, world, world),
              file=sys.stderr)
    if args.dbg and not dry:
        from centerpose_amd import hip

        hip.lib().cp_set_debug(args.dbg)
    batch = args.batch or DEFAULT_BATCH[args.workload]

    def barrier():
        if dist is not None:
            if backend == "nccl" and not dry:
                dist.barrier(device_ids=[local])
            else:
                dist.barrier()
        if not dry:
            torch.cuda.synchronize()

    if args.workload == "track_e2e":  # host-in-the-loop measurement, single GPU
        if world != 1:
            raise SystemExit("track_e2e is a single-process measurement")
        leg = track_e2e_leg(device, args.precision, batch, args.steps, max(args.warmup, 2))
        leg.update({"metric": "frames/sec over %d concurrent videos (CenterPoseTrack loop incl. host tracker)" % batch,
                    "n_gpus": 1, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "data": "synthetic",
                    "dtype": "f32", "config": {"workload": leg["workload"]}})
        print(json.dumps(leg), flush=True)
        return

    # this rank's contiguous shard of the global batch (BASELINE configs[3]: 512 = 8 x 64); frames are seeded by GLOBAL image
    # index, so image g is the same frame at every N
    g0, g1 = cpd.shard_range(world * batch, rank, world)
    assert g1 - g0 == batch
    if dry:
        pipe = DryPipeline(batch, rank, local, start=g0, workload=args.workload)
    else:
        pipe = Pipeline(args.workload, batch, device, seed=317 + g0, precision=args.precision,
                        serial_pnp=args.serial_pnp, gather=world > 1)
        side = torch.cuda.Stream(device=device)  # a non-default stream (hipGraph capture needs one)
        torch.cuda.set_stream(side)
    dt, prof, roles, sampled = timed_region(pipe, args.steps, args.warmup, barrier, profile=not dry)
    dumped = None
    if args.dump_outputs and rank == 0:  # before anything else runs on the pipeline's buffers
        dumped = dump_outputs(pipe, args.dump_outputs)
    rccl_ranks = 1
    allgather = None
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=device if (device is not None and backend == "nccl") else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        # the collective really ran: gather one tagged record per rank and read the world size back from the group
        tag = torch.full((1, 1, 4), float(rank), dtype=torch.float32,
                         device=device if (device is not None and backend == "nccl") else "cpu")
        got = cpd.allgather_detections(tag).flatten()[::4].tolist()
        if got != [float(r) for r in range(world)]:
            raise SystemExit("bench.py: all-gather returned %r, expected ranks 0..%d in order" % (got, world - 1))
        rccl_ranks = dist.get_world_size()
        # the per-step collective next to the step: MAX over ranks of each rank's mean (HIP events on its launch stream)
        gm = pipe.gather_timer.mean_ms() if getattr(pipe, "gather_timer", None) is not None else None
        tg = torch.tensor([gm if gm is not None else -1.0], dtype=torch.float64, device=t.device)
        dist.all_reduce(tg, op=dist.ReduceOp.MAX)
        if float(tg.item()) >= 0:
            nbytes = pipe.gather_timer.bytes_out
            allgather = {"ms_per_step_max_over_ranks": round(float(tg.item()), 4), "ms_per_step_rank0": round(gm, 4),
                         "bytes_received_per_rank": nbytes, "gbps_per_rank": round(nbytes / 1e9 / (float(tg.item()) * 1e-3), 2)
                         if float(tg.item()) > 0 else None,
                         "timer": "HIP events on the launch stream" if not dry else "perf_counter around the blocking gloo call"}
        if dry and pipe.gathered is not None:
            # the shards tile [0, global batch) exactly, and the records arrive in (rank, image, slot) order
            gi = pipe.gathered[:, 0, 2].to(torch.int64).tolist()
            if gi != list(range(world * batch)):
                raise SystemExit("bench.py: shards do not tile [0, %d): %r ..." % (world * batch, gi[:8]))
            rk = pipe.gathered[:, 0, 0].to(torch.int64).tolist()
            if rk != [g // batch for g in range(world * batch)] or \
               not bool((pipe.gathered[:, :, 3] == torch.arange(100, dtype=torch.float32).view(1, 100)).all()):
                raise SystemExit("bench.py: gathered records are not in (rank, image, slot) order")
    ms_per_step = dt / args.steps * 1e3
    value = world * batch * args.steps / dt

    if rank == 0:
        more = extras(args, world, dry)
        roof = None if dry else roofline_object(prof, roles, sampled, batch, args.precision, args.workload)
        if roof is not None and args.workload == "full":
            ms, n = pipe.pnp_stats()
            if ms:
                roof["pnp"] = {"bound": "latency", "ms_per_batch_on_side_stream": round(ms, 3),
                               "detections_last_batch": n,
                               "detections_per_s_while_solving": round(n / (ms * 1e-3), 1) if n else None,
                               "note": "PnP-input assembly + batched solve of one batch, HIP events on hip.PoseStage's side "
                                       "stream; runs under the next batch's network (DESIGN 3.6)"}
        lat = lat_det = None
        if more["latency"]:
            pipe.gather = False  # rank 0 alone: no collective inside the batch-1 latency loop
            lat = frame_latency(pipe)
            if args.workload == "full":
                lat_det = detect_latency(pipe)
        legs = None
        if more["legs"]:
            # the other configurations, driver-timed in the same run (short legs; each has its own roofline object)
            del pipe.model
            pipe._stages.clear()
            torch.cuda.empty_cache()
            legs = {}
            k = max(4, min(args.steps, 10))   # (6 steps after 2 warm-ups gave one 35 % outlier in a dozen runs: a leg is a few
            w = max(1, min(args.warmup, 3))   # hundred milliseconds either way)
            legs["configs1"] = run_leg("decode", device, args.precision, max(4, min(args.steps, 12)), w, barrier,
                                       not args.no_latency)
            try:
                legs["decode_only"] = decode_only_leg(device, args.precision)
            except Exception as e:
                legs["decode_only"] = {"error": "%s: %s" % (type(e).__name__, e)}
            try:
                legs["pnp_rendered"], legs["rendered_e2e"] = pnp_rendered_leg(device)
            except Exception as e:
                legs["pnp_rendered"] = legs["rendered_e2e"] = {"error": "%s: %s" % (type(e).__name__, e)}
            try:
                legs["e2e_u8"] = e2e_u8_leg(device, args.precision, k, w, barrier)
            except Exception as e:
                legs["e2e_u8"] = {"error": "%s: %s" % (type(e).__name__, e)}
            legs["exact_f32"] = run_leg("full", device, "f32", 4, 1, barrier, False)
            for name in ("hourglass", "track", "track_gru"):
                legs[name] = run_leg(name, device, args.precision, k, w, barrier, False)
            try:
                legs["track_e2e"] = track_e2e_leg(device, args.precision, DEFAULT_BATCH["track_e2e"], 6, 2)
            except Exception as e:  # the host-in-the-loop leg must not take the headline line down with it
                legs["track_e2e"] = {"error": "%s: %s" % (type(e).__name__, e)}
        cpu = None
        if more["cpu_baseline"]:
            cpu = cpu_baseline(args.workload, pipe.arch)
        elif world > 1:
            cpu = {"skipped": "N > 1: the reference's CPU path is timed on rank 0 of the N = 1 run only"}
        elif not dry and not args.full:
            cpu = {"skipped": "the reference's CPU path is timed by --full runs only"}
        key = pipe.arch + ("_track" if pipe.track else "")
        gf = GFLOP_PER_IMG[key]
        tail = {"full": " + post-process + PnP", "decode": "", "hourglass": ""}.get(args.workload, " + detection all-gather")
        out = {
            "metric": "images/sec at 512x512 %s (backbone + heat-map decode%s)" % (
                "2-stack hourglass" if pipe.arch == "hourglass" else "DLA-34", tail),
            "value": round(value, 2), "unit": "images/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if args.precision == "f32" else "f32 via split-f16 (f16x3) MFMA, f32 accumulate",
            "data": "dry-run (stub pipeline, no device work)" if dry else "synthetic",
            "rccl_ranks": rccl_ranks,
            **({"allgather": allgather} if allgather is not None else {}),
            **({"dry_run_global_images": [int(pipe.gathered[0, 0, 2]), int(pipe.gathered[-1, 0, 2]), int(pipe.gathered.shape[0])]}
               if dry and pipe.gathered is not None else {}),
            **({"dry_run_devices": [int(v) for v in pipe.gathered[::batch, 0, 1].tolist()]} if dry and pipe.gathered is not None else {}),
            "config": {"workload": WORKLOAD_TEXT[args.workload] % batch, "global_batch": world * batch,
                       "per_gpu_batch": batch, "input": "512x512",
                       "parallelism": "batch-shard x%d (%s)" % (
                           world, "all-gather of detection records over %s" % ("RCCL" if backend == "nccl" else backend)
                           if world > 1 else "single rank, no collective"),
                       "gflop_per_image": gf,
                       **({"gflop_note": "603.7 = BASELINE.md's 739.2 GFLOP/img for the reference module minus the 135.3 of "
                                         "the first stack's seven heads, which do not feed model(x)[-1] (object_pose.py:135) "
                                         "and are not computed"} if pipe.arch == "hourglass" else {})},
            "p50_frame_ms_batch1": lat,
            **({"p50_frame_ms_batch1_network_decode": lat_det} if lat_det is not None else {}),
            "whole_step_tflops": round(value * gf / 1e3 / world, 2),
            "roofline": roof, "legs": legs, "cpu_baseline": cpu,
        }
        line = compact_line(out)
        line["detail"] = write_detail(out)
        if dumped is not None:
            line["dumped_outputs"] = dumped
        print(json.dumps(line), flush=True)
    if dist is not None:
        barrier()  # rank 0 may still be measuring the batch-1 latency; leave together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
