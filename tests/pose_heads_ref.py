"""Float64 reference of the prediction-head block (n heads Conv2d(Cin, hid, 3, padding=1) -> ReLU -> Conv2d(hid, classes, 1)
on one feature map) as torch CPU ops under autograd, a hand-written float64 backward that guards it, the input generators of
the GPU tests and the computed allowance for hidden units at the ReLU kink.  No test lives here."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

DLA_CLASSES = (1, 2, 16, 2, 8, 2, 3)  # hm, wh, hps, reg, hm_hp, hp_offset, scale (opts.py:394-426, 8 keypoints)
AMBIGUOUS_REL = 2e-5                  # |h64| <= this * max|h64|: float32 may gate the unit differently
AMBIGUOUS_CAP = 1e-3                  # largest share of such units a realistic case may have


def _f64(t):
    return t.detach().cpu().double()


def forward64(feat, params):
    """feat [B,Cin,H,W], params [(w0, b0, w1, b1)] -> (outs, hiddens) in float64; hidden is the pre-activation."""
    feat = _f64(feat)
    outs, hids = [], []
    for w0, b0, w1, b1 in params:
        h = F.conv2d(feat, _f64(w0), _f64(b0), padding=1)
        hids.append(h)
        outs.append(F.conv2d(F.relu(h), _f64(w1), _f64(b1)))
    return outs, hids


def reference(feat, params, grad_outs):
    """Autograd in float64.  grad_outs[i] None = the head is left out.  -> dict(outs, hidden, gfeat, grads[i] = (gw0, gb0, gw1, gb1))."""
    x = _f64(feat).requires_grad_(True)
    ps = [[_f64(t).requires_grad_(True) for t in p] for p in params]
    outs, hids, total = [], [], None
    for (w0, b0, w1, b1), go in zip(ps, grad_outs):
        h = F.conv2d(x, w0, b0, padding=1)
        o = F.conv2d(F.relu(h), w1, b1)
        hids.append(h.detach())
        outs.append(o.detach())
        if go is not None:
            term = (o * _f64(go)).sum()
            total = term if total is None else total + term
    if total is not None:
        total.backward()
    grads = [tuple(t.grad if t.grad is not None else torch.zeros_like(t) for t in p) for p in ps]
    gfeat = x.grad if x.grad is not None else torch.zeros_like(x)
    return dict(outs=outs, hidden=hids, gfeat=gfeat, grads=grads)


def _wgrad3x3(x, g):
    """sum over images and pixels of g[b,h,y,x] * x[b,c,y+i-1,x+j-1] -> [hid, Cin, 3, 3]"""
    B, C, H, W = x.shape
    cols = F.unfold(x, 3, padding=1).reshape(B, C, 9, H * W)
    return torch.einsum("bhp,bctp->hct", g.reshape(B, g.shape[1], H * W), cols).reshape(g.shape[1], C, 3, 3)


def manual_backward64(feat, params, grad_outs):
    """The same gradients written out by hand (no autograd): the formulas of centerpose_amd/csrc/heads_bwd.hip."""
    x = _f64(feat)
    gfeat = torch.zeros_like(x)
    grads = []
    for (w0, b0, w1, b1), go in zip(params, grad_outs):
        w0, b0, w1, b1 = map(_f64, (w0, b0, w1, b1))
        if go is None:
            grads.append(tuple(torch.zeros_like(t) for t in (w0, b0, w1, b1)))
            continue
        go = _f64(go)
        h = F.conv2d(x, w0, b0, padding=1)
        gw1 = torch.einsum("bcyx,bhyx->ch", go, F.relu(h)).reshape(w1.shape)
        gb1 = go.sum(dim=(0, 2, 3))
        gh = torch.einsum("bcyx,ch->bhyx", go, w1[:, :, 0, 0])
        gh = torch.where(h <= 0, torch.zeros_like(gh), gh)   # torch's threshold_backward: a NaN h passes the gradient
        gb0 = gh.sum(dim=(0, 2, 3))
        gw0 = _wgrad3x3(x, gh)
        gfeat += F.conv_transpose2d(gh, w0, padding=1)
        grads.append((gw0, gb0, gw1, gb1))
    return dict(gfeat=gfeat, grads=grads)


def allowance(feat, params, grad_outs, hidden):
    """The largest change the ambiguous hidden units (|h64| <= AMBIGUOUS_REL * max|h64| per head) can cause: every gradient
    is linear in the gate, so it is the same backward on absolute values restricted to those units.  grad_w1 reads relu(h),
    which is continuous: there the change is at most |h| * |grad_out| of those units.
    -> dict(share, gfeat, grads[i] = (gw0, gb0, gw1, gb1)) of non-negative float64 arrays."""
    x = _f64(feat).abs()
    gfeat = torch.zeros_like(x)
    grads, amb_n, n = [], 0, 0
    for (w0, b0, w1, b1), go, h in zip(params, grad_outs, hidden):
        w0, w1 = _f64(w0).abs(), _f64(w1).abs()
        if go is None:
            grads.append(tuple(torch.zeros(tuple(t.shape), dtype=torch.float64) for t in (w0, b0, w1, b1)))
            continue
        go = _f64(go).abs()
        amb = h.abs() <= AMBIGUOUS_REL * float(h.abs().max())
        amb_n += int(amb.sum())
        n += amb.numel()
        gh = torch.einsum("bcyx,ch->bhyx", go, w1[:, :, 0, 0]) * amb
        gw1 = torch.einsum("bcyx,bhyx->ch", go, h.abs() * amb).reshape(w1.shape)
        gfeat += F.conv_transpose2d(gh, w0, padding=1)
        grads.append((_wgrad3x3(x, gh), gh.sum(dim=(0, 2, 3)), gw1, torch.zeros(w1.shape[0], dtype=torch.float64)))
    return dict(share=amb_n / max(n, 1), gfeat=gfeat, grads=grads)


def dyadic_case(seed, B, Cin, hid, H, W, classes, go_scale=1.0):
    """The strict inputs: feat and w0 multiples of 1/4 in [-2, 2], b0 an odd multiple of 1/32, so every hidden value is an odd
    multiple of 1/32 computed exactly in float32 (and in f16x3): never zero, gated alike in float32 and float64.  w1, b1 and
    grad_out are Gaussian.  -> SimpleNamespace(feat, params, grad_outs) of float32 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.randint(-8, 9, (B, Cin, H, W), generator=g).float() / 4
    params, gos = [], []
    for c in classes:
        w0 = torch.randint(-8, 9, (hid, Cin, 3, 3), generator=g).float() / 4
        b0 = (2 * torch.randint(-16, 16, (hid,), generator=g) + 1).float() / 32
        w1 = torch.randn(c, hid, 1, 1, generator=g) * 0.05
        b1 = torch.randn(c, generator=g)
        params.append((w0, b0, w1, b1))
        gos.append(torch.randn(B, c, H, W, generator=g) * go_scale)
    assert 9 * Cin * 4 + float(max(p[1].abs().max() for p in params)) < 2 ** 24 / 32
    case = SimpleNamespace(feat=feat, params=params, grad_outs=gos)
    check_dyadic(case)
    return case


def check_dyadic(case):
    """The generator's promises, checked on the CPU: float32 hidden values equal the float64 ones, are odd multiples of 1/32,
    and 30-70 % of the units are active."""
    for w0, b0, _, _ in case.params:
        h32 = F.conv2d(case.feat, w0, b0, padding=1)
        h64 = F.conv2d(case.feat.double(), w0.double(), b0.double(), padding=1)
        assert torch.equal(h32.double(), h64)
        k = h64 * 32
        assert torch.equal(k, k.round()) and bool((k.abs() % 2 == 1).all())
        active = float((h64 > 0).double().mean())
        assert 0.3 <= active <= 0.7, active


def gaussian_grad_outs(seed, B, classes, H, W):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, c, H, W, generator=g) for c in classes]


def head_params(state_dict, heads):
    """[(w0, b0, w1, b1)] of a reference-format state dict, in the order of ``heads``."""
    return [tuple(state_dict["%s.%s" % (h, k)].float() for k in ("0.weight", "0.bias", "2.weight", "2.bias")) for h in heads]


# ---- the shapes of the GPU tests' strict cases (tests/test_pose_heads_gpu.py), so the CPU suite can check the generator on all of them
DYADIC_SHAPES = {
    # name: (B, Cin, hid, H, W, classes)
    "dla_128": (2, 64, 256, 128, 128, DLA_CLASSES),
    "dla_32": (1, 64, 256, 32, 32, DLA_CLASSES),
    "resdcn": (2, 64, 64, 32, 32, DLA_CLASSES),
    "c128_h96": (1, 128, 96, 24, 24, (3, 5)),
    "ragged_13x19": (2, 64, 64, 13, 19, (2, 16)),
    "ragged_1x1": (3, 32, 32, 1, 1, (1, 4)),
    "ragged_130x66": (1, 64, 64, 130, 66, (8,)),
    "classes_1": (1, 64, 64, 16, 16, (1,)),
    "classes_64": (1, 64, 64, 16, 16, (64,)),
}

# ---- single-head cases on which cp_pose_heads_backward and cp_conv2d_backward_nhwc must agree bit for bit: the heads' 3x3 layer
# runs conv_bwd.hip's weight and data gradient, so the same grad_hidden gives the same bits.  The smallest shapes that reach each
# accumulator count of the weight-gradient kernel (hid 96 / 64 / 256: NH = 1 / 2 / 4), with ragged rows and a slab that spans images
SHARED_CONV_CASES = {
    # name: (seed, B, Cin, hid, H, W, classes)
    "nh2_two_images_13x19": (101, 2, 64, 64, 13, 19, (1,)),
    "nh1_9x7": (102, 1, 128, 96, 9, 7, (1,)),
    "nh4_8x10": (103, 1, 64, 256, 8, 10, (1,)),
}
