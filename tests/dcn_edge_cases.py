"""Case constructors for the DCNv2 edge tests (test helper, not a test module).

The patch-resident forward kernels (dcn16p / dcn16t: halo 3, dcn16s: halo 4) give every 8 x 16 block of output pixels a
staged input halo.  A *valid* sample whose 2 x 2 corner block leaves that halo is an "exception": the block files it in a
list of ECAP entries (184 for p / t, 64 for s) and, past that capacity, switches as a whole to buffer loads.  Which mode a
block runs in therefore depends on the offsets only.  ``exception_field`` builds offsets that give every block a chosen
exception count; ``count_exceptions`` restates the kernels' predicate (float32, dcn16p.hip / dcn16t.hip / dcn16s.hip set-up)
so that a test can assert the counts it relies on.  Every offset is a multiple of 1/4 (or of 2^-8 in ``exact_positions``), so
the kernels' float32 sums ``(y - 1 + kh) + off`` are exact and every sample lands where the case says."""
import numpy as np
import torch

TH, TW = 8, 16                         # output pixels per block (patch16_common.h: PATCH_TH, PATCH_TW)
GEOM = {"p": (3, 184), "t": (3, 184), "s": (4, 64)}   # kernel -> (HALO, ECAP)


def blocks(H, W):
    assert H % TH == 0 and W % TW == 0, "the patch kernels need whole 8 x 16 blocks"
    return H // TH, W // TW


def _positions(off, H, W):
    """float32 sample positions h_im, w_im [B, 9, H, W] as the kernels form them: (y - 1 + kh) + off."""
    off = np.asarray(off, dtype=np.float32)
    B = off.shape[0]
    t = np.arange(9)
    ys = (np.arange(H)[None, :, None] - 1 + t[:, None, None] // 3).astype(np.float32)
    xs = (np.arange(W)[None, None, :] - 1 + t[:, None, None] % 3).astype(np.float32)
    h = ys[None] + off[:, 0::2]
    w = xs[None] + off[:, 1::2]
    return h.reshape(B, 9, H, W), w.reshape(B, 9, H, W)


def exception_mask(off, H, W, halo):
    """[B, 9, H, W] bool: the sample is valid and its corner block leaves the halo of its own block."""
    h, w = _positions(off, H, W)
    valid = (h > -1) & (w > -1) & (h < H) & (w < W)
    hf = np.where(valid, h, np.float32(0))
    wf = np.where(valid, w, np.float32(0))
    ph, pw = TH + 2 * halo, TW + 2 * halo
    ty0 = (np.arange(H) // TH * TH)[None, None, :, None]
    tx0 = (np.arange(W) // TW * TW)[None, None, None, :]
    qy = np.floor(hf).astype(np.int64) - (ty0 - halo)
    qx = np.floor(wf).astype(np.int64) - (tx0 - halo)
    inside = (qy >= 0) & (qy <= ph - 2) & (qx >= 0) & (qx <= pw - 2)
    return valid & ~inside


def count_exceptions(off, H, W, halo):
    """Exception samples per block: int array [B, H / 8, W / 16]."""
    e = exception_mask(off, H, W, halo)
    B = e.shape[0]
    tys, txs = blocks(H, W)
    return e.reshape(B, 9, tys, TH, txs, TW).sum(axis=(1, 3, 5))


def exception_field(B, H, W, counts, seed=0, border_images=()):
    """Offsets [B, 18, H, W] (float32 tensor) giving block (b, by, bx) exactly ``counts[b, by, bx]`` exception samples for
    either halo (3 or 4).  Every other sample moves by at most one pixel (multiples of 1/4 in [-1, 1]), which keeps it inside
    the halo or makes it invalid.  An exception sample is sent, still valid, to a column of another block at least four
    columns beyond the halo of either width.  In the images listed in ``border_images`` the exception samples of the top
    (bottom) border blocks land in rows (-1, 0) (resp. (H - 1, H)): one corner row outside the image, the neighbouring image's
    border row in memory."""
    tys, txs = blocks(H, W)
    assert txs >= 2, "exception samples need another block column to go to"
    counts = np.broadcast_to(np.asarray(counts), (B, tys, txs))
    assert counts.max() <= 9 * TH * TW
    rng = np.random.default_rng(seed)
    off = (rng.integers(-4, 5, size=(B, 18, H, W)) / 4.0).astype(np.float32)
    q = np.array([0.0, 0.25, 0.5, 0.75])
    for b in range(B):
        for by in range(tys):
            for bx in range(txs):
                n = int(counts[b, by, bx])
                if n == 0:
                    continue
                ty0, tx0 = by * TH, bx * TW
                cols = np.array([c for c in range(W) if c <= tx0 - 5 or c >= tx0 + TW + 4])
                pick = rng.choice(9 * TH * TW, size=n, replace=False)
                t, r = pick // (TH * TW), pick % (TH * TW)
                y, x = ty0 + r // TW, tx0 + r % TW
                wt = rng.choice(cols, size=n) + rng.choice(q, size=n)
                if b in border_images and (by == 0 or by == tys - 1):
                    top = by == 0 if tys > 1 else (np.arange(n) % 2 == 0)
                    frac = rng.choice(q[1:], size=n)
                    ht = np.where(top, -frac, H - frac)
                else:
                    ht = rng.integers(0, H, size=n) + rng.choice(q, size=n)
                off[b, 2 * t, y, x] = ht - (y - 1 + t // 3)
                off[b, 2 * t + 1, y, x] = wt - (x - 1 + t % 3)
    return torch.from_numpy(off)


def capacity_counts(B, H, W, cap):
    """Per-block counts with blocks at cap - 1, cap and cap + 1 (the last block of the last image at cap + 1), the others
    spread below and above the capacity."""
    tys, txs = blocks(H, W)
    n = B * tys * txs
    assert n >= 3
    ladder = [0, cap - 1, cap, cap + 1, cap // 2, 2 * cap]
    c = np.array([ladder[i % len(ladder)] for i in range(n)])
    c[-3:] = (cap - 1, cap, cap + 1)
    return c.reshape(B, tys, txs)


def loud_border_input(B, C, H, W, mid, seed=0, loud=64.0):
    """Input [B, C, H, W] whose images next to image ``mid`` carry their border rows facing it (row H - 1 of image mid - 1,
    row 0 of image mid + 1) ``loud`` times louder: a corner read across the image boundary cannot hide."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    x[mid - 1, :, H - 1] *= loud
    x[mid + 1, :, 0] *= loud
    return x


def exact_positions(B, H, W, seed=0):
    """Offsets [B, 18, H, W] whose samples land exactly on image edges and integer points or far away, and masks
    [B, 9, H, W] with zeros among them.  Per axis a sample takes one of: -1, -1 + 2^-8, -2^-8, 0, 2^-8, H - 1 - 2^-8, H - 1,
    H - 1 + 2^-8, H - 2^-8, H (resp. W), an integer inside, or a plain sample near its pixel; or the whole offset is one of
    +-1e4, +-1e10.  All these sums are exact in float32."""
    rng = np.random.default_rng(seed)
    e = 2.0 ** -8

    def targets(n, size):
        return np.array([-1.0, -1 + e, -e, 0.0, e, n - 1 - e, n - 1.0, n - 1 + e, n - e, float(n)] +
                        [float(v) for v in rng.integers(1, n - 1, size=size)])

    t = np.arange(9)
    ys = (np.arange(H)[None, :, None] - 1 + t[:, None, None] // 3).astype(np.float64)
    xs = (np.arange(W)[None, None, :] - 1 + t[:, None, None] % 3).astype(np.float64)
    shape = (B, 9, H, W)
    th, tw = targets(H, 6), targets(W, 6)
    h = np.where(rng.random(shape) < 0.8, rng.choice(th, size=shape), ys + rng.integers(-4, 5, size=shape) / 4.0)
    w = np.where(rng.random(shape) < 0.8, rng.choice(tw, size=shape), xs + rng.integers(-4, 5, size=shape) / 4.0)
    off = np.empty((B, 18, H, W))
    off[:, 0::2] = h - ys
    off[:, 1::2] = w - xs
    far = np.array([1e4, -1e4, 1e10, -1e10])
    sel = rng.random((B, 18, H, W)) < 0.05
    off = np.where(sel, rng.choice(far, size=off.shape), off)
    mask = rng.uniform(0.0, 1.0, size=shape)
    mask = np.where(rng.random(shape) < 0.1, 0.0, mask)
    return torch.from_numpy(off.astype(np.float32)), torch.from_numpy(mask.astype(np.float32))


def bwd_chunk_images(B, C, H, W, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1):
    """Images per grad_col chunk of the backward, as dcn_bwd.hip's plan() computes it (256 MiB cap, at least one)."""
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    per_img = C * kh * kw * Ho * Wo * 4
    return max(1, min(B, (256 << 20) // per_img))
