"""Times the overlay (cp_draw_detections + cp_draw_primitives) at B = 64 frames of 720 x 1280 and writes the table to
profiles/draw_bench.txt (or --out).

  loads      (a) 1 - 10 detections per image, every one with a solved cuboid: the occupancy of the rendered_e2e scenes;
             (b) K = 100 detections per image, all visible; (c) an empty list (count 0: 4400 cleared slots per image)
  overlay    GPU events around list builder + rasteriser, the median of --iters calls after a warm-up; the three loads take
             turns (a, b, c, a, b, c, ...) and the figure of a load is the median of its three rounds.  `raster` is the
             rasteriser alone on the same list
  covered    pixels any primitive covers (counted by drawing the list in white on black frames), the bytes the tile kernel
             stores (3 per covered pixel: it stores nothing else) and the time 6.29 TB/s, the measured HBM copy rate, would take
             for them; `list MB` is what the tile pass reads of the compact lists (16 bytes per surviving primitive and tile)
  detect     the same run's time of one detect step (dla_34, f16x3, B = 64 frames of 512 x 512, cp_model_detect)
  PIL        the same list of image 0 drawn with PIL.ImageDraw on the host, times B: another rasteriser (its own line and
             circle rules, no glyphs), for context only

  python tools/draw_bench.py [--iters 20] [--out profiles/draw_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from centerpose_amd import hip, synth  # noqa: E402
from centerpose_amd.hip import draw as hd  # noqa: E402

COPY_RATE = 6.29e12  # bytes/s
B, H, W, K = 64, 720, 1280, 100
S = hip._structs.DRAW_SLOTS


def median_ms(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def records(counts, seed):
    """post [B, K, 120], pnp [B, K, 40]: boxes of 80 - 320 pixels somewhere in the frame, the 8 vertices inside the box."""
    rs = np.random.RandomState(seed)
    post, pnp = np.zeros((B, K, 120)), np.zeros((B, K, 40))
    post[..., 0] = rs.uniform(0.4, 0.95, (B, K))
    post[..., 2:5] = rs.uniform(0.5, 1.5, (B, K, 3))
    bw, bh = rs.uniform(80, 320, (B, K)), rs.uniform(80, 320, (B, K))
    x0, y0 = rs.uniform(0, W - bw), rs.uniform(0, H - bh)
    post[..., 24], post[..., 25], post[..., 26], post[..., 27] = x0, y0, x0 + bw, y0 + bh
    u = rs.uniform(0, 1, (B, K, 8, 2))
    pnp[..., 8:24] = (np.stack([x0, y0], -1)[:, :, None] + u * np.stack([bw, bh], -1)[:, :, None]).reshape(B, K, 16)
    pnp[..., 0] = 1
    q = rs.normal(size=(B, K, 4))
    pnp[..., 24:28] = pnp[..., 31:35] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    pnp[..., 4:7] = pnp[..., 28:31] = rs.uniform(-0.3, 0.3, (B, K, 3)) + (0, 0, 3.0)
    return post, pnp, np.asarray(counts, np.int32)


def pil_ms(prims, frame):
    from PIL import Image, ImageDraw

    img = Image.fromarray(frame)
    d = ImageDraw.Draw(img)
    t0 = time.perf_counter()
    for kind, x0, y0, x1, y1, size, c, _ in prims:
        col = (c >> 16 & 255, c >> 8 & 255, c & 255)
        if kind == 1:
            d.line([(x0, y0), (x1, y1)], fill=col, width=size)
        elif kind == 2:
            d.ellipse([x0 - size, y0 - size, x0 + size, y0 + size], fill=col)
        elif kind == 3:
            d.rectangle([min(x0, x1), min(y0, y1), max(x0, x1), max(y0, y1)], outline=col, width=size)
        elif kind == 4:
            d.rectangle([min(x0, x1), min(y0, y1), max(x0, x1), max(y0, y1)], fill=col)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "draw_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("draw_bench: no HIP device (there is no CPU timing of a device call)")
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(1)
    frames = torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(dev)
    cam = torch.tensor([[1000.0, 1000.0, W / 2.0, H / 2.0]] * B, dtype=torch.float64, device=dev)
    params = hd.draw_params(None, width=W, height=H, vis_thresh=0.3, show_axes=1)
    loads = [("a: 1-10 per image", records(rs.randint(1, 11, B), 2)), ("b: K = 100 visible", records([K] * B, 3)),
             ("c: empty list", records([0] * B, 4))]
    state = []
    for name, (post, pnp, count) in loads:
        t = [torch.from_numpy(a).to(dev) for a in (post, count, pnp)]
        prims = torch.empty(B, K * S, 8, dtype=torch.int32, device=dev)
        ws = torch.empty(hd.workspace_bytes(B, K * S), dtype=torch.uint8, device=dev)
        state.append((name, t, prims, ws))

    def overlay(i):
        _, (post, count, pnp), prims, ws = state[i]
        hd.draw_detections(post, count, pnp, cam, params, out=prims)
        hd.draw_primitives(frames, prims, ws=ws)

    def raster(i):
        hd.draw_primitives(frames, state[i][2], ws=state[i][3])

    rounds = {i: ([], []) for i in range(3)}
    for _ in range(3):          # alternating rounds
        for i in range(3):
            rounds[i][0].append(median_ms(lambda: overlay(i), args.iters))
            rounds[i][1].append(median_ms(lambda: raster(i), args.iters))

    # the same run's detect step
    model = hip.HipModel("dla_34", synth.HEADS_POSE, synth.make_state_dict("dla_34", synth.HEADS_POSE), precision="f16x3")
    x = torch.cat([synth.frames(8, seed=317 + i) for i in range(0, B, 8)]).to(dev)
    detect = [median_ms(lambda: model.detect(x, K=100, rep_mode=1, fit_gaussian=False, balance=2.0, graph=False), max(5, args.iters // 2))
              for _ in range(3)]
    detect_ms = float(np.median(detect))

    tiles = ((W + 63) // 64) * ((H + 15) // 16)
    lines = ["Overlay (cp_draw_detections + cp_draw_primitives) at B = %d frames of %d x %d, K = %d x %d slots; median of three "
             "alternating rounds of %d calls (HIP events)" % (B, H, W, K, S, args.iters),
             "covered = pixels any primitive covers; stored MB = 3 bytes per covered pixel (all the tile kernel stores); floor = "
             "those bytes at 6.29 TB/s; list MB = 16 bytes per surviving primitive and tile, read by the tile pass",
             "detect step of the same run (dla_34, f16x3, B = %d x 512 x 512): %.3f ms   (rounds %s)"
             % (B, detect_ms, ", ".join("%.3f" % v for v in detect)),
             " load               | prims/img | overlay ms  raster ms | covered Mpx  stored MB   floor ms | list MB | share of detect | PIL host ms (x B)"]
    for i, (name, _, prims, ws) in enumerate(state):
        ov, ra = float(np.median(rounds[i][0])), float(np.median(rounds[i][1]))
        hd.draw_detections(*state[i][1][:2], state[i][1][2], cam, params, out=prims)
        white = prims.clone()
        white[..., 6] = 0xFFFFFF
        black = torch.zeros_like(frames)
        hd.draw_primitives(black, white)
        covered = int((black[..., 0] != 0).sum())
        host = prims.cpu().numpy()
        n_prims = float((host[..., 0] != 0).sum()) / B
        pil = pil_ms([tuple(int(v) for v in p) for p in host[0] if p[0] != 0], np.zeros((H, W, 3), np.uint8)) * B
        lines.append(" %-18s | %9.1f | %10.4f %10.4f | %11.3f %10.2f %10.5f | %7.1f | %14.2f%% | %10.1f"
                     % (name, n_prims, ov, ra, covered / 1e6, 3 * covered / 1e6, 3 * covered / COPY_RATE * 1e3,
                        n_prims * B * tiles * 16 / 1e6, 100.0 * ov / detect_ms, pil))
        lines.append("   rounds: overlay %s | raster %s" % (", ".join("%.4f" % v for v in rounds[i][0]),
                                                           ", ".join("%.4f" % v for v in rounds[i][1])))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
