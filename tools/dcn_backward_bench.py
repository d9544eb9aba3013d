"""DCNv2 backward (cp_dcnv2_backward) per fast-path layer shape, next to the forward of the same shape (GPU).

    python tools/dcn_backward_bench.py [--batches 16 64] [--iters 10] [--std 1.0] [--layers TEXT] [--deterministic]
                                       [--precision f32|both]

One JSON line per (shape, batch): ms per call of cp_dcnv2_backward and of cp_dcnv2_forward (HIP events around `iters`
back-to-back calls with pre-allocated outputs and workspace), the backward's TFLOP/s against the f32 matrix peak
(157.3 TFLOP/s; FLOPs = the two contractions, 4 * B * H * W * 9C * Co), a model of its HBM bytes against 8 TB/s, and its
global float-atomic bytes against the chip-wide atomic rate (1.3 TB/s).  The atomic bytes are counted on the host from the
actual offsets: the halo kernel's flush (at most one add per in-image halo cell and channel per 16 x 4 patch) plus every
corner add that falls outside its patch's halo.  Per-kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/dcn_backward_bench.py --batches 16 --iters 3`.
--deterministic also times cp_dcnv2_backward_det on the same tensors: the two calls alternate in three rounds of `iters`
calls each and the median round is reported for both (bwd_ms, bwd_det_ms), with the deterministic call's workspace and the
bytes of its sorted index (16 per (pixel, tap, corner) of a grad_col chunk).
--precision both times cp_dcnv2_backward_prec in CP_PREC_F32 (the two calls above, bit for bit) and in CP_PREC_F16X3 on both
paths: the four calls alternate in three rounds after a warm-up of each, and the median round is reported (f32_ms, f16x3_ms,
f32_det_ms, f16x3_det_ms and the two ratios), with the f16x3 workspaces and the mask of what ran in f16x3.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from centerpose_amd import hip  # noqa: E402

SHAPES = [  # (name, C, Co, H = W): CenterPose (dla) and resdcn DCN layers
    ("dla 64->64 @128", 64, 64, 128), ("dla 128->128 @64", 128, 128, 64), ("dla 256->256 @32", 256, 256, 32),
    ("dla 256->128 @32", 256, 128, 32), ("dla 512->256 @16", 512, 256, 16),
    ("resdcn 128->64 @64", 128, 64, 64),  # resdcn's other two stages are the 512->256 @16 and 256->128 @32 rows
]
PEAK_TF, HBM_GBPS, ATOMIC_GBPS = 157.3, 8000.0, 1300.0
PT_X, PT_Y, R = 16, 4, 4  # dcn_bwd.hip's patch and halo margin


def atomic_bytes(off, B, C, H, W):
    """Global float-atomic bytes of the halo kernel for these offsets (host model of dcn_bwd.hip)."""
    hy, hx = PT_Y + 2 * R + 1, PT_X + 2 * R + 1
    ys = torch.arange(H, device=off.device).view(1, H, 1)
    xs = torch.arange(W, device=off.device).view(1, 1, W)
    outside = 0
    for t in range(9):
        i, j = divmod(t, 3)
        sy = (ys - 1 + i).float() + off[:, 2 * t]
        sx = (xs - 1 + j).float() + off[:, 2 * t + 1]
        live = (sy > -1) & (sx > -1) & (sy < H) & (sx < W)
        y0, x0 = torch.floor(sy).long(), torch.floor(sx).long()
        hy0 = (ys // PT_Y) * PT_Y - R
        hx0 = (xs // PT_X) * PT_X - R
        for dy in (0, 1):
            for dx in (0, 1):
                y, x = y0 + dy, x0 + dx
                inimg = live & (y >= 0) & (y < H) & (x >= 0) & (x < W)
                inhalo = (y >= hy0) & (y < hy0 + hy) & (x >= hx0) & (x < hx0 + hx)
                outside += int((inimg & ~inhalo).sum())
    cells = 0
    for py in range(0, H, PT_Y):
        for px in range(0, W, PT_X):
            ny = min(H, py - R + hy) - max(0, py - R)
            nx = min(W, px - R + hx) - max(0, px - R)
            cells += ny * nx
    return 4 * C * (outside + B * cells)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--std", type=float, default=1.0)
    ap.add_argument("--layers", default="", help="only the layer shapes whose name contains this text")
    ap.add_argument("--deterministic", action="store_true", help="also time cp_dcnv2_backward_det, alternating with the default")
    ap.add_argument("--precision", default="f32", choices=["f32", "both"],
                    help="both: also time cp_dcnv2_backward_prec in f32 and f16x3 on both paths, alternating")
    a = ap.parse_args()
    L = hip.lib()
    dev = torch.device("cuda:0")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for B in a.batches:
        for name, C, Co, H in SHAPES:
            if a.layers not in name:
                continue
            W = H
            g = torch.Generator(device=dev).manual_seed(0)
            x = torch.randn(B, C, H, W, device=dev, generator=g)
            w = torch.randn(Co, C, 3, 3, device=dev, generator=g) / (9 * C) ** 0.5
            b = torch.randn(Co, device=dev, generator=g)
            off = a.std * torch.randn(B, 18, H, W, device=dev, generator=g)
            mask = torch.rand(B, 9, H, W, device=dev, generator=g)
            go = torch.randn(B, Co, H, W, device=dev, generator=g)
            y = torch.empty(B, Co, H, W, device=dev)
            grads = [torch.empty_like(t) for t in (x, off, mask, w, b)]
            nf = L.cp_dcnv2_workspace_bytes(B, C, H, W, Co)
            nb = L.cp_dcnv2_backward_workspace_bytes(B, C, H, W, Co, 3, 3, 1, 1, 1, 1, 1, 1, 1)
            wsf = torch.empty(nf, dtype=torch.uint8, device=dev)
            wsb = torch.empty(nb, dtype=torch.uint8, device=dev)
            geo = (B, C, H, W, Co, 3, 3, 1, 1, 1, 1, 1, 1, 1)

            def fwd():
                return L.cp_dcnv2_forward(s, P(x), P(w), P(b), P(off), P(mask), P(y), *geo, P(wsf), nf)

            def bwd():
                return L.cp_dcnv2_backward(s, P(x), P(w), P(off), P(mask), P(go), *[P(t) for t in grads], *geo, P(wsb), nb)

            order = [("fwd", fwd), ("bwd", bwd)]
            if a.deterministic:
                nd = L.cp_dcnv2_backward_det_workspace_bytes(*geo)
                wsd = torch.empty(nd, dtype=torch.uint8, device=dev)

                def det():
                    return L.cp_dcnv2_backward_det(s, P(x), P(w), P(off), P(mask), P(go), *[P(t) for t in grads], *geo, P(wsd),
                                                   nd)

                order = [("fwd", fwd)] + [("bwd", bwd), ("bwd_det", det)] * 3
            prec_ws = {}
            if a.precision == "both":
                def prec_call(det, prec):
                    n = L.cp_dcnv2_backward_prec_workspace_bytes(*geo, det, prec)
                    buf = torch.empty(n, dtype=torch.uint8, device=dev)
                    prec_ws[(det, prec)] = n
                    return lambda: L.cp_dcnv2_backward_prec(s, P(x), P(w), P(off), P(mask), P(go), *[P(t) for t in grads], *geo,
                                                            det, prec, P(buf), n)

                four = [("f32", prec_call(0, 0)), ("f16x3", prec_call(0, 1)), ("f32_det", prec_call(1, 0)), ("f16x3_det", prec_call(1, 1))]
                for _, fn in four:   # the warm-up of each, before the first timed round of any
                    assert fn() == 0, L.cp_last_error()
                order = order + four * 3
            rounds = {}
            for key, fn in order:
                assert fn() == 0, L.cp_last_error()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                rounds.setdefault(key, []).append(e0.elapsed_time(e1) / a.iters)
            res = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
            px = B * H * W
            flops = 4.0 * px * 9 * C * Co
            # HBM model: inputs and outputs once; NHWC input stage written + read, grad_output transposed written + read,
            # grad_col written + read, the NHWC input gradient read + written by the NCHW copy-out
            hbm = 4.0 * (2 * px * C + px * 27 * 2 + 2 * px * Co + 2 * 9 * C * Co) + 4.0 * (
                2 * px * C + 2 * px * Co + 2 * px * 9 * C + 2 * px * C)
            atom = atomic_bytes(off, B, C, H, W)
            ms = res["bwd"]
            extra = {}
            if a.deterministic:
                chunk = min(B, max(1, (256 << 20) // (9 * C * H * W * 4)))  # dcn_bwd.hip: plan
                extra = {"bwd_det_ms": round(res["bwd_det"], 4), "det_over_default": round(res["bwd_det"] / ms, 2),
                         "det_workspace_mb": round(nd / 2 ** 20, 1), "index_entries_m": round(chunk * H * W * 36 / 1e6, 2),
                         "index_mb": round(16 * chunk * H * W * 36 / 2 ** 20, 1), "chunks": -(-B // chunk)}
                del wsd
            if a.precision == "both":
                extra.update({k + "_ms": round(res[k], 4) for k in ("f32", "f16x3", "f32_det", "f16x3_det")})
                extra.update({"f16x3_over_f32": round(res["f16x3"] / res["f32"], 3),
                              "f16x3_det_over_f32_det": round(res["f16x3_det"] / res["f32_det"], 3),
                              "f16x3_mask": L.cp_dcnv2_backward_prec_mask(*geo, 0, 1),
                              "f16x3_workspace_mb": round(prec_ws[(0, 1)] / 2 ** 20, 1),
                              "f16x3_det_workspace_mb": round(prec_ws[(1, 1)] / 2 ** 20, 1)})
            print(json.dumps({
                "layer": name, "B": B, "offset_std": a.std, "bwd_ms": round(ms, 4), "fwd_ms": round(res["fwd"], 4),
                "bwd_over_fwd": round(ms / res["fwd"], 2), "tflops": round(flops / ms / 1e9, 2),
                "frac_f32_peak": round(flops / ms / 1e9 / PEAK_TF, 3), "hbm_model_gb": round(hbm / 1e9, 3),
                "frac_hbm_peak": round(hbm / ms / 1e6 / HBM_GBPS, 3), "atomic_gb": round(atom / 1e9, 3),
                "atomic_floor_ms": round(atom / ATOMIC_GBPS / 1e6, 4),
                "naive_atomic_gb": round(4.0 * px * 9 * 4 * C / 1e9, 3), "workspace_mb": round(nb / 2 ** 20, 1), **extra}),
                flush=True)
            del x, w, b, off, mask, go, y, grads, wsf, wsb
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
