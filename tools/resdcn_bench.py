"""resdcn throughput and the dense deconv kernel against the composite the other kernels can do (GPU).

    python tools/resdcn_bench.py [--batch 64] [--res 512] [--iters 10]

Prints JSON lines:
* per arch (resdcn_18, resdcn_101) and precision: img/s of network + decode + post-process + PnP at B = --batch
  (ObjectPoseDetector.run_batch on pre-processed frames), p50 batch-1 latency of the same chain, and the per-kernel
  times of one profiled network forward (HipModel.profile_read);
* per resdcn_18 deconv layer at B = --batch: the stand-alone deconv call vs a 3x3 / stride-1 cp_conv2d_nhwc with
  4*Cout zero-embedded taps followed by a pixel shuffle (the same values computed by existing kernels), and the largest
  difference between the two results.  Both stand-alone calls pack their weights on every call, so these wall times
  include packing; for kernel-against-kernel times run this part under
  `rocprofv3 --kernel-trace --stats -- python tools/resdcn_bench.py --skip-network --layer L`
  (deconv_kernel against igemm16 / igemm + the shuffle's copy kernel);
* per deconv launch inside the profiled network (pre-packed weights): time, TFLOP/s and GB/s, with their shares of
  the f16x3 (833 TFLOP/s = 2.5 PFLOP/s / 3) or f32 (157.3 TFLOP/s) matrix ceiling and of 8 TB/s HBM.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from centerpose_amd import hip, synth  # noqa: E402


PEAK_TFLOPS = {"f16x3": 2500.0 / 3, "f32": 157.3}
HBM_GBPS = 8000.0


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def composite_weight(w):
    """ConvTranspose2d(k=4, s=2, p=1) weight [Cin, Cout, 4, 4] -> 3x3 / stride-1 / pad-1 conv weight [4*Cout, Cin, 3, 3]
    whose channel (2*py + px)*Cout + co is output parity class (py, px): tap (dy, dx) of the 3x3 window reads input row
    i + dy - 1, which class py reaches through ky = py + 3 - 2*dy (when 0 <= ky < 4)."""
    Cin, Cout = w.shape[:2]
    out = torch.zeros(4 * Cout, Cin, 3, 3, dtype=w.dtype, device=w.device)
    for py in range(2):
        for px in range(2):
            c = 2 * py + px
            for dy in range(3):
                ky = py + 3 - 2 * dy
                if not 0 <= ky < 4:
                    continue
                for dx in range(3):
                    kx = px + 3 - 2 * dx
                    if 0 <= kx < 4:
                        out[c * Cout:(c + 1) * Cout, :, dy, dx] = w[:, :, ky, kx].t()
    return out


def composite(x, wc, scale4, shift4, Cout):
    y = hip.conv2d_nhwc(x, wc, scale4, shift4, None, 1, 1, 1)  # [B,H,W,4*Cout], class-major channels
    B, H, W, _ = y.shape
    return y.view(B, H, W, 2, 2, Cout).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, Cout)


def deconv_layers(batch, res, iters, dev, only=None):
    sd = synth.make_state_dict("resdcn_18", synth.HEADS_POSE)
    rows = []
    for i, (c, hw) in enumerate(((256, res // 32), (128, res // 16), (64, res // 8))):
        if only is not None and i != only:
            continue
        w = sd["deconv_layers.%d.weight" % (6 * i + 3)].to(dev)
        g = torch.Generator().manual_seed(i)
        x = torch.relu(torch.randn(batch, hw, hw, c, generator=g)).to(dev)
        scale = (torch.rand(c, generator=g) + 0.5).to(dev)
        shift = (torch.randn(c, generator=g) * 0.1).to(dev)
        wc = composite_weight(w)
        scale4, shift4 = scale.repeat(4), shift.repeat(4)
        for prec in ("f16x3", "f32"):
            hip.set_default_precision(prec)
            ours = hip.conv_transpose2d(x, w, scale, shift, act=1)
            comp = composite(x, wc, scale4, shift4, c)
            t_ours = _time(lambda: hip.conv_transpose2d(x, w, scale, shift, act=1), iters)
            t_comp = _time(lambda: composite(x, wc, scale4, shift4, c), iters)
            flops = 2.0 * batch * (2 * hw) ** 2 * c * 4 * c
            nbytes = 4.0 * (batch * hw * hw * c + batch * 4 * hw * hw * c + 16 * c * c)
            rows.append(dict(layer="deconv_layers.%d" % (6 * i + 3), precision=prec, B=batch, Cin=c, Cout=c, H=hw, W=hw,
                             ms=t_ours, composite_ms=t_comp, speedup=t_comp / t_ours, tflops=flops / t_ours / 1e9,
                             gbps=nbytes / t_ours / 1e6, max_abs_diff=float((ours - comp).abs().max()),
                             note="includes per-call weight packing of both paths"))
            print(json.dumps(rows[-1]), flush=True)
    hip.set_default_precision("f32")
    return rows


def network(arch, batch, res, iters, dev):
    from centerpose_amd.lib.detectors.detector_factory import detector_factory
    from centerpose_amd.lib.models.model import create_model, save_model
    from centerpose_amd.lib.opts import opts

    out = []
    for prec in ("f16x3", "f32"):
        o = opts().parser.parse_args(["--arch", arch, "--c", "cup", "--debug", "0"])
        o.nms = True
        o.obj_scale = True
        o.use_pnp = True
        opt = opts().init(opts().parse(o))
        opt.precision = prec
        sd = synth.make_state_dict(arch, opt.heads)
        ck = os.path.join(tempfile.gettempdir(), "resdcn_bench_%s.pth" % arch)
        m = create_model(opt.arch, opt.heads, opt.head_conv, opt)
        m.load_state_dict(sd, strict=True)
        save_model(ck, 1, m)
        opt.load_model = ck
        det = detector_factory[opt.task](opt)
        rng = np.random.RandomState(0)
        img = rng.randint(0, 255, (res, res, 3)).astype(np.uint8)
        images, meta = det.pre_process(img, 1.0, {})
        xb = images.repeat(batch, 1, 1, 1)
        metas = [meta] * batch
        det.run_batch(xb, metas)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            det.run_batch(xb, metas)
        torch.cuda.synchronize()
        ips = batch * iters / (time.perf_counter() - t0)
        lat = []
        for _ in range(max(iters, 20)):
            t = time.perf_counter()
            det.run_batch(images, [meta])
            torch.cuda.synchronize()
            lat.append((time.perf_counter() - t) * 1e3)
        hm = hip.HipModel(arch, opt.heads, sd, head_conv=opt.head_conv, precision=prec)
        x = synth.frames(batch, seed=1, h=res, w=res).to(dev)
        hm(x)
        hm.profile(True)
        hm(x)
        torch.cuda.synchronize()
        dump = os.path.join(tempfile.gettempdir(), "resdcn_bench_launches_%d.csv" % os.getpid())
        if os.path.exists(dump):
            os.remove(dump)
        os.environ["CP_PROFILE_DUMP"] = dump  # per-launch rows: name, M, N, K, kh, stride, ms, TFLOP/s, role
        kernels = hm.profile_read()
        del os.environ["CP_PROFILE_DUMP"]
        deconvs = []
        with open(dump) as f:
            for line in f:
                name, M, N, K, kh, stride, ms, tf, role = line.strip().split(",")
                if role != "deconv":
                    continue
                M, N, K, ms = int(M), int(N), int(K), float(ms)
                flops = 2.0 * M * N * K
                nbytes = 4.0 * (M // 4 * (K // 4) + M * N + 4 * K * N)  # input once, output once, weights
                deconvs.append(dict(kernel=name, Cin=K // 4, Cout=N, out_pixels=M, ms=ms, tflops=flops / ms / 1e9,
                                    gbps=nbytes / ms / 1e6, share_of_matrix_peak=flops / ms / 1e9 / PEAK_TFLOPS[prec],
                                    share_of_hbm=nbytes / ms / 1e6 / HBM_GBPS))
        os.remove(dump)
        roles = hm.profile_roles()
        hm.profile(False)
        out.append(dict(arch=arch, precision=prec, B=batch, res=res, img_per_s=ips, p50_batch1_ms=float(np.median(lat)),
                        kernels={k: dict(v, tflops=v["flops"] / v["ms"] / 1e9) for k, v in kernels.items()},
                        roles=roles, deconv_launches=deconvs))
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--skip-network", action="store_true")
    ap.add_argument("--layer", type=int, default=None, help="only this deconv layer (0: 256 ch, 1: 128, 2: 64)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    deconv_layers(a.batch, a.res, a.iters, dev, a.layer)
    if not a.skip_network:
        for arch in ("resdcn_18", "resdcn_101"):
            network(arch, a.batch, a.res, a.iters, dev)


if __name__ == "__main__":
    main()
