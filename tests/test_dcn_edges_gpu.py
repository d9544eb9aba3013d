"""DCNv2 kernels at their data-dependent mode switches and edges (pytest -m gpu).

Offsets from tests/dcn_edge_cases.py put each block of the patch-resident forward kernels at a chosen exception count (below,
at and above the capacity at which a block switches to buffer loads), put samples exactly on image edges, integer points and
far outside, and the backward runs over several grad_col chunks.  Errors are measured per image, relative to that image's own
max |reference|, so that a read across an image boundary cannot hide behind a louder neighbour: 2e-5 for the forward, 1e-4
per gradient for the backward (the tolerances of test_gpu_parity.py and test_dcn_backward_gpu.py)."""
import numpy as np
import pytest
import torch

from centerpose_amd import hip
from oracle import dcn as odcn
from tests import dcn_backward_ref as R
from tests import dcn_edge_cases as E

pytestmark = pytest.mark.gpu
S = hip.KernelSel
CP = (3, 3, 1, 1, 1, 1, 1, 1, 1)
GRAD_NAMES = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")

# f16x3 kernels that stage a halo per 8 x 16 block: name -> (exception geometry, selection)
PATCH = {
    "dcn16p": ("p", S.DCN16P_ALWAYS | S.DCN16P_NOT_WIDE | S.DCN16S_NEVER | S.DCN16T_NEVER),
    "dcn16p_wide": ("p", S.DCN16P_ALWAYS | S.DCN16S_NEVER | S.DCN16T_NEVER),   # 128-wide N tile (Co % 128 == 0)
    "dcn16t": ("t", S.DCN16P_ALWAYS | S.DCN16T_ALWAYS),
    "dcn16s": ("s", S.DCN16P_ALWAYS | S.DCN16S_ALWAYS | S.DCN16T_NEVER),
    "dcn16s_grid8": ("s", S.DCN16P_ALWAYS | S.DCN16S_ALWAYS | S.DCN16T_NEVER | S.DCN16S_GRID8),
}
# every forward kernel: (precision, selection)
FORWARD = dict({k: ("f16x3", sel) for k, (_, sel) in PATCH.items()},
               dcn16=("f16x3", S.DCN16P_NEVER), generic_f16x3=("f16x3", S.DCN_GENERIC),
               exact_f32=("f32", 0), generic_f32=("f32", S.DCN_GENERIC))


def _layer(C, Co, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Co, C, 3, 3, generator=g) / (C * 9) ** 0.5
    b = torch.randn(Co, generator=g)
    return w, b


def _forward(device, precision, sel, x, w, b, off, mask):
    hip.set_default_precision(precision)
    try:
        with hip.select_kernels(sel):
            return hip.dcn_v2_forward(*(t.to(device) for t in (x, w, b, off, mask)), *CP).cpu()
    finally:
        hip.set_default_precision("f32")


def _assert_per_image(out, ref, tol, what=""):
    for i in range(ref.shape[0]):
        scale = float(ref[i].abs().max())
        err = float((out[i].double() - ref[i]).abs().max())
        assert err <= tol * scale, "%s image %d: max err %.3g vs max |ref| %.3g" % (what, i, err, scale)


# ---------------------------------------------------------------- B: exception capacity and cross-image reads (f16x3)

@pytest.mark.parametrize("kernel", list(PATCH))
def test_forward_blocks_at_the_exception_capacity(device, kernel):
    """Blocks at ECAP - 1, ECAP (the last exceptions still filed, fast mode) and ECAP + 1 (buffer-load mode) in one launch,
    the last block of the last image at ECAP + 1."""
    geo, sel = PATCH[kernel]
    halo, cap = E.GEOM[geo]
    B, C, Co, H, W = 2, 64, 128, 16, 32
    counts = E.capacity_counts(B, H, W, cap)
    off = E.exception_field(B, H, W, counts, seed=11)
    assert np.array_equal(E.count_exceptions(off, H, W, halo), counts)
    assert counts[-1, -1, -1] == cap + 1 and {cap - 1, cap}.issubset(counts.ravel().tolist())
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, C, H, W, generator=g)
    mask = torch.rand(B, 9, H, W, generator=g)
    w, b = _layer(C, Co, 13)
    out = _forward(device, "f16x3", sel, x, w, b, off, mask)
    _assert_per_image(out, odcn.dcn_v2_forward_f64(x, w, b, off, mask), 2e-5, kernel)


@pytest.mark.parametrize("kernel", list(PATCH))
def test_forward_border_exceptions_do_not_read_the_neighbouring_image(device, kernel):
    """B = 3: the middle image's border blocks file their exceptions in rows (-1, 0) and (H - 1, H) -- one corner row outside
    the picture, in memory the neighbouring image's border row, which is 2^6 times louder.  One block of each border row
    is over the capacity (buffer loads with corner-validity bits), the other at the capacity (exceptions staged per chunk)."""
    geo, sel = PATCH[kernel]
    halo, cap = E.GEOM[geo]
    B, C, Co, H, W = 3, 32, 128, 16, 32
    counts = np.zeros((B, 2, 2), dtype=np.int64)
    counts[0] = counts[2] = cap // 2
    counts[1] = [[cap + 1, cap], [cap, cap + 1]]
    off = E.exception_field(B, H, W, counts, seed=21, border_images=(1,))
    assert np.array_equal(E.count_exceptions(off, H, W, halo), counts)
    x = E.loud_border_input(B, C, H, W, mid=1, seed=22)
    mask = torch.rand(B, 9, H, W, generator=torch.Generator().manual_seed(23))
    w, b = _layer(C, Co, 24)
    out = _forward(device, "f16x3", sel, x, w, b, off, mask)
    _assert_per_image(out, odcn.dcn_v2_forward_f64(x, w, b, off, mask), 2e-5, kernel)


def test_dcn16t_equals_dcn16s_where_their_modes_differ(device):
    """dcn16t and dcn16s sum the same products in the same order.  With 65 .. 184 exceptions a block is in fast mode in
    dcn16t (capacity 184) and in buffer-load mode in dcn16s (capacity 64): the outputs must still agree bit for bit."""
    B, C, Co, H, W = 3, 64, 64, 16, 32
    counts = np.array([0, 63, 64, 65, 100, 183, 184, 185, 64, 65, 120, 40]).reshape(B, 2, 2)
    off = E.exception_field(B, H, W, counts, seed=31, border_images=(1,))
    ct, cs = E.count_exceptions(off, H, W, 3), E.count_exceptions(off, H, W, 4)
    assert np.array_equal(ct, counts) and np.array_equal(cs, counts)
    assert np.sum((counts > 64) & (counts <= 184)) >= 4   # blocks where the two kernels sit in different modes
    x = E.loud_border_input(B, C, H, W, mid=1, seed=32)
    mask = torch.rand(B, 9, H, W, generator=torch.Generator().manual_seed(33))
    w, b = _layer(C, Co, 34)
    outs = {k: _forward(device, "f16x3", PATCH[k][1], x, w, b, off, mask) for k in ("dcn16t", "dcn16s", "dcn16s_grid8")}
    assert torch.equal(outs["dcn16t"], outs["dcn16s"])
    assert torch.equal(outs["dcn16s"], outs["dcn16s_grid8"])
    _assert_per_image(outs["dcn16t"], odcn.dcn_v2_forward_f64(x, w, b, off, mask), 2e-5)


def test_dcn16s_workgroups_alternate_between_modes(device):
    """dcn16s on 8 workgroups (one per XCD): XCD x walks a contiguous range of items (dcn16s.hip: it_lo .. it_end), and
    consecutive items alternate 0 / 64 / 65 exceptions, so every workgroup hands over fast -> fast, fast -> slow and
    slow -> fast, with the two parity counters of the exception list in every combination."""
    B, C, Co, H, W = 3, 64, 64, 32, 64
    tys, txs = E.blocks(H, W)
    items = B * tys * txs                                   # Co = 64: one N tile, item = block in (b, ty, tx) order
    counts = np.array([(0, 64, 65)[i % 3] for i in range(items)]).reshape(B, tys, txs)
    off = E.exception_field(B, H, W, counts, seed=41, border_images=(1,))
    assert np.array_equal(E.count_exceptions(off, H, W, 4), counts)
    iq, ir = items // 8, items % 8
    flat = counts.ravel()
    for xcd in range(8):
        lo = xcd * (iq + 1) if xcd < ir else ir * (iq + 1) + (xcd - ir) * iq
        walk = flat[lo:lo + iq + (1 if xcd < ir else 0)]
        slow = walk > 64
        assert len(walk) >= 3 and np.any(slow[1:] & ~slow[:-1]) and np.any(~slow[1:] & slow[:-1]), walk
    x = E.loud_border_input(B, C, H, W, mid=1, seed=42)
    mask = torch.rand(B, 9, H, W, generator=torch.Generator().manual_seed(43))
    w, b = _layer(C, Co, 44)
    out8 = _forward(device, "f16x3", PATCH["dcn16s_grid8"][1], x, w, b, off, mask)
    full = _forward(device, "f16x3", PATCH["dcn16s"][1], x, w, b, off, mask)
    assert torch.equal(out8, full)
    _assert_per_image(out8, odcn.dcn_v2_forward_f64(x, w, b, off, mask), 2e-5)


# ---------------------------------------------------------------- C: exact sample positions

@pytest.mark.parametrize("kernel", list(FORWARD))
def test_forward_exact_positions(device, kernel):
    """Samples exactly at -1, 0, H - 1, H (and W), 2^-8 inside each edge, on integer points, offsets of +-1e4 / +-1e10 (a
    zero sample), masks of 0: the validity test and the corner selection at their boundaries."""
    precision, sel = FORWARD[kernel]
    B, C, Co, H, W = 2, 64, 128, 16, 32
    off, mask = E.exact_positions(B, H, W, seed=51)
    g = torch.Generator().manual_seed(52)
    x = torch.randn(B, C, H, W, generator=g)
    w, b = _layer(C, Co, 53)
    out = _forward(device, precision, sel, x, w, b, off, mask)
    assert torch.isfinite(out).all()
    _assert_per_image(out, odcn.dcn_v2_forward_f64(x, w, b, off, mask), 2e-5, kernel)


def _expected_bwd(*args):
    return R.backward_ref(*args) if odcn.have_reference() else R.backward_f64(*args)


def _backward(device, x, w, b, off, mask, go):
    return [t.cpu() for t in hip.dcn_v2_backward(*(t.to(device) for t in (x, w, b, off, mask, go)), *CP)]


def _assert_grads(got, exp, tol=1e-4, what=""):
    """Per image for grad_input / grad_offset / grad_mask, whole tensor for grad_weight / grad_bias."""
    for k, (name, a, e) in enumerate(zip(GRAD_NAMES, got, exp)):
        assert a.shape == e.shape, name
        parts = range(a.shape[0]) if k < 3 else [None]
        for i in parts:
            ai, ei = (a[i], e[i]) if i is not None else (a, e)
            scale = float(ei.abs().max())
            err = float((ai.double() - ei.double()).abs().max())
            assert err <= tol * scale + 1e-30, "%s %s image %s: max err %.3g vs max |ref| %.3g" % (what, name, i, err, scale)


@pytest.mark.parametrize("C,path", [(32, "halo_kernel<32>"), (16, "halo_kernel<16>"), (24, "generic")])
def test_backward_exact_positions(device, C, path):
    """The backward's validity test and its one-sided coordinate gradient (get_coordinate_weight) at integer positions and
    edges, far samples and zero masks: the fast path's two halo-kernel instantiations and the generic path (C % 16 != 0)."""
    B, Co, H, W = 2, 24, 12, 20
    off, mask = E.exact_positions(B, H, W, seed=61 + C)
    g = torch.Generator().manual_seed(62)
    x = torch.randn(B, C, H, W, generator=g)
    w, b = _layer(C, Co, 63)
    go = torch.randn(B, Co, H, W, generator=g)
    got = _backward(device, x, w, b, off, mask, go)
    assert all(torch.isfinite(t).all() for t in got)
    _assert_grads(got, _expected_bwd(x, w, b, off, mask, go, *CP), what=path)


# ---------------------------------------------------------------- D: masks outside [-1, 1] (f16x3)

@pytest.mark.parametrize("kernel", ["dcn16p", "dcn16p_wide", "dcn16t", "dcn16s", "dcn16"])
def test_forward_masks_beyond_one(device, kernel):
    """cp_dcnv2_forward takes any mask.  The f16x3 kernels fold the mask into the corner weights of a pre-scaled activation;
    with |mask| up to 8 and samples landing (integer offsets: weights 1, 0, 0, 0) on the input's max pixel, the blended value
    reaches 8 x the activation bound.  The output must stay within the f16x3 budget."""
    precision, sel = FORWARD[kernel]
    B, C, Co, H, W = 2, 64, 128, 16, 32
    g = torch.Generator().manual_seed(71)
    x = torch.randn(B, C, H, W, generator=g)
    x[:, :, 5, 7] = 8.0                                     # the tensor's max |x|, in every channel of both images
    off = torch.randint(-2, 3, (B, 18, H, W), generator=g).float()
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    near = (ys < 8) & (xs < 16)                             # block (0, 0): a third of its samples on the max pixel
    for t in range(9):
        hit = near & (torch.rand(H, W, generator=g) < 0.34)
        off[:, 2 * t][:, hit] = (5 - (ys - 1 + t // 3)[hit]).float()
        off[:, 2 * t + 1][:, hit] = (7 - (xs - 1 + t % 3)[hit]).float()
    mask = torch.rand(B, 9, H, W, generator=g) * 16 - 8
    mask[0, :, :4, :4] = 8.0
    mask[1, :, :4, :4] = -8.0
    w, b = _layer(C, Co, 72)
    out = _forward(device, precision, sel, x, w, b, off, mask)
    assert torch.isfinite(out).all()
    _assert_per_image(out, odcn.dcn_v2_forward_f64(x, w, b, off, mask), 2e-5, kernel)


def test_forward_masks_within_one_keep_the_scale(device):
    """The mask's |max| enters the activation bound only above 1: a mask in [0, 1] and the same mask with one entry at
    exactly 1 give the same bits (the bound is max |x| either way)."""
    B, C, Co, H, W = 2, 64, 64, 16, 32
    g = torch.Generator().manual_seed(81)
    x = torch.randn(B, C, H, W, generator=g)
    off = torch.randn(B, 18, H, W, generator=g) * 1.5
    mask = torch.rand(B, 9, H, W, generator=g) * 0.999
    mask1 = mask.clone()
    mask1[0, 0, 0, 0] = 1.0
    w, b = _layer(C, Co, 82)
    sel = PATCH["dcn16t"][1]
    a = _forward(device, "f16x3", sel, x, w, b, off, mask)
    a1 = _forward(device, "f16x3", sel, x, w, b, off, mask1)
    assert torch.equal(a[1], a1[1])


# ---------------------------------------------------------------- E: backward grad_col chunks, halo_kernel<16>

BWD_CHUNKS = [
    # B, C, Co, H, W: the halo kernel's instantiation; nb images per grad_col chunk (256 MiB cap) < B, not dividing it
    (16, 64, 64, 128, 128),   # halo_kernel<32>: the 64 -> 64 layer at 128^2, chunks of 7, 7, 2
    (6, 16, 16, 301, 301),    # halo_kernel<16> (C % 32 == 16), ragged in x (301 % 16) and y (301 % 4): chunks of 5, 1
    (4, 48, 32, 203, 203),    # halo_kernel<16>, C = 48, ragged: chunks of 3, 1
]


@pytest.mark.parametrize("B,C,Co,H,W", BWD_CHUNKS)
def test_backward_over_several_grad_col_chunks(device, B, C, Co, H, W):
    nb = E.bwd_chunk_images(B, C, H, W)
    assert nb < B and B % nb != 0 and -(-B // nb) >= 2, (B, nb)
    g = torch.Generator().manual_seed(B + C + H)
    x = torch.randn(B, C, H, W, generator=g)
    w, b = _layer(C, Co, C + 1)
    off = torch.randn(B, 18, H, W, generator=g) * 2.0
    mask = torch.rand(B, 9, H, W, generator=g) * 2 - 0.5    # nonzero, some negative, some above 1
    go = torch.randn(B, Co, H, W, generator=g)
    full = _backward(device, x, w, b, off, mask, go)
    singles = [_backward(device, x[i:i + 1], w, b, off[i:i + 1], mask[i:i + 1], go[i:i + 1]) for i in range(B)]
    for i, s in enumerate(singles):
        # grad_offset / grad_mask are reproducible (no atomics): chunk position must not change a bit
        assert torch.equal(full[1][i], s[1][0]), "grad_offset image %d" % i
        assert torch.equal(full[2][i], s[2][0]), "grad_mask image %d" % i
        scale = float(s[0].abs().max())
        assert float((full[0][i] - s[0][0]).abs().max()) <= 1e-4 * scale, "grad_input image %d" % i
    for k in (3, 4):   # weight and bias gradients: the chunked batch is the sum of its images
        total = sum(s[k].double() for s in singles)
        assert float((full[k].double() - total).abs().max()) <= 1e-4 * float(total.abs().max()), GRAD_NAMES[k]
    for i in (0, B - 1):   # first and last image (the ragged last chunk) against the reference
        sl = [t[i:i + 1] for t in (x, off, mask, go)]
        exp = _expected_bwd(sl[0], w, b, sl[1], sl[2], sl[3], *CP)
        got = [full[0][i:i + 1], full[1][i:i + 1], full[2][i:i + 1], singles[i][3], singles[i][4]]
        _assert_grads(got, exp, what="image %d" % i)
