"""The DCN edge-case constructors (tests/dcn_edge_cases.py) against independent brute-force counts, on the CPU: the GPU edge
tests (test_dcn_edges_gpu.py) assert the per-block exception counts and chunk counts these helpers promise."""
import math

import numpy as np
import pytest

from tests import dcn_edge_cases as E


def _brute_force_counts(off, H, W, halo):
    """One sample at a time, in float32, the kernels' predicate written out again (dcn16p.hip / dcn16s.hip set-up)."""
    off = off.numpy()
    B = off.shape[0]
    ph, pw = E.TH + 2 * halo, E.TW + 2 * halo
    out = np.zeros((B, H // E.TH, W // E.TW), dtype=np.int64)
    f32 = np.float32
    for b in range(B):
        for y in range(H):
            for x in range(W):
                ty0, tx0 = y // E.TH * E.TH, x // E.TW * E.TW
                for t in range(9):
                    h_im = f32(y - 1 + t // 3) + off[b, 2 * t, y, x]
                    w_im = f32(x - 1 + t % 3) + off[b, 2 * t + 1, y, x]
                    if not (h_im > -1 and w_im > -1 and h_im < H and w_im < W):
                        continue
                    qy = math.floor(h_im) - (ty0 - halo)
                    qx = math.floor(w_im) - (tx0 - halo)
                    if not (0 <= qy <= ph - 2 and 0 <= qx <= pw - 2):
                        out[b, y // E.TH, x // E.TW] += 1
    return out


@pytest.mark.parametrize("kernel", ["p", "s"])
def test_exception_field_gives_the_requested_counts(kernel):
    halo, cap = E.GEOM[kernel]
    B, H, W = 3, 16, 32
    counts = E.capacity_counts(B, H, W, cap)
    off = E.exception_field(B, H, W, counts, seed=3, border_images=(1,))
    assert off.dtype.is_floating_point and off.dtype.itemsize == 4
    assert np.all(off.numpy() * 4 == np.round(off.numpy() * 4))   # multiples of 1/4: exact float32 sums
    bf = _brute_force_counts(off, H, W, halo)
    assert np.array_equal(bf, counts)
    assert np.array_equal(E.count_exceptions(off, H, W, halo), counts)
    assert counts[-1, -1, -1] == cap + 1
    assert {cap - 1, cap, cap + 1} <= set(counts.ravel().tolist())


def test_exception_field_counts_hold_for_the_other_halo():
    """A field built for one kernel family is valid for the other: the exiled samples clear both halos, the jittered ones
    stay inside both."""
    B, H, W = 2, 8, 48
    counts = np.arange(B * 3).reshape(B, 1, 3) * 37
    off = E.exception_field(B, H, W, counts, seed=5)
    for halo in (3, 4):
        assert np.array_equal(_brute_force_counts(off, H, W, halo), counts)


def test_border_images_put_their_border_exceptions_in_the_outer_row():
    B, H, W = 3, 16, 32
    counts = np.full((B, 2, 2), 70)
    off = E.exception_field(B, H, W, counts, seed=1, border_images=(1,))
    h, _ = E._positions(off.numpy(), H, W)
    ex = E.exception_mask(off.numpy(), H, W, 3)
    top, bot = h[1, :, :E.TH][ex[1, :, :E.TH]], h[1, :, E.TH:][ex[1, :, E.TH:]]
    assert top.size == 140 and bot.size == 140
    assert np.all((top > -1) & (top < 0)) and np.all((bot > H - 1) & (bot < H))
    for b in (0, 2):   # the other images' exceptions are anywhere in the picture
        hb = h[b][ex[b]]
        assert np.all((hb >= 0) & (hb < H))


def test_exact_positions_land_where_they_say():
    B, H, W = 2, 8, 32
    off, mask = E.exact_positions(B, H, W, seed=2)
    h32, w32 = E._positions(off.numpy(), H, W)
    t = np.arange(9)
    ys = np.arange(H)[None, :, None] - 1 + t[:, None, None] // 3
    xs = np.arange(W)[None, None, :] - 1 + t[:, None, None] % 3
    h64 = ys[None] + off.numpy()[:, 0::2].astype(np.float64)
    w64 = xs[None] + off.numpy()[:, 1::2].astype(np.float64)
    near = (np.abs(off.numpy()[:, 0::2]) < 1e3) & (np.abs(off.numpy()[:, 1::2]) < 1e3)
    assert np.array_equal(h32[near], h64[near]) and np.array_equal(w32[near], w64[near])  # no rounding in the kernels' sum
    e = 2.0 ** -8
    for v in (-1.0, -1 + e, 0.0, e, H - 1.0, H - e, float(H)):
        assert np.any(h32[near] == v), v
    for v in (-1.0, 0.0, W - 1.0, W - e, float(W)):
        assert np.any(w32[near] == v), v
    for v in (1e4, -1e4, 1e10, -1e10):
        assert np.any(off.numpy() == np.float32(v)), v
    assert np.any(mask.numpy() == 0) and np.any(mask.numpy() > 0)


def test_backward_chunk_planning_matches_the_worked_example():
    # dcn_bwd.hip plan(): grad_col holds at most 256 MiB; 64 channels at 128 x 128 are 36 MiB an image -> 7 per chunk
    assert E.bwd_chunk_images(16, 64, 128, 128) == 7
    assert E.bwd_chunk_images(2, 64, 128, 128) == 2
    assert E.bwd_chunk_images(1, 512, 512, 512) == 1
