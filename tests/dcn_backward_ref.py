"""References for the DCNv2 backward (test helper, not a test module).

``backward_ref`` restates the reference's CPU orchestration ``dcn_v2_cpu_backward`` (DCNv2/src/cpu/dcn_v2_cpu.cpp:109-238):
per image, ``columns = W^T grad_out`` (float64, rounded to float32: the stand-in for THFloatBlas_gemm), then the
reference's COMPILED ``modulated_deformable_col2im_coord_cpu`` / ``modulated_deformable_col2im_cpu`` /
``modulated_deformable_im2col_cpu`` from oracle/_ref/libdcn_im2col_ref.so, and the weight / bias gradients in float64.

``backward_f64`` is an independent float64 restatement: torch autograd through a vectorised forward whose sample
positions are the float32 positions the reference computes (so both sides sit on the same side of every integer), with the
reference's quirk for the input gradient (pad_h on both axes, dcn_v2_im2col_cpu.cpp:364) unless ``quirk=False``."""
import ctypes

import torch

from oracle import dcn as odcn

_P, _I = ctypes.c_void_p, ctypes.c_int
_fns = {}


def have_reference():
    return odcn.have_reference()


def _ref(name):
    if name not in _fns:
        lib = ctypes.CDLL(odcn._REF)
        fn = getattr(lib, name)
        if name == "modulated_deformable_col2im_coord_cpu":  # dcn_v2_im2col_cpu.h:83-90
            fn.argtypes = [_P] * 4 + [_I] * 15 + [_P] * 2
        else:  # modulated_deformable_col2im_cpu, dcn_v2_im2col_cpu.h:76-81
            fn.argtypes = [_P] * 3 + [_I] * 15 + [_P]
        fn.restype = None
        _fns[name] = fn
    return _fns[name]


def out_size(H, W, kh, kw, sh, sw, ph, pw, dh, dw):
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def backward_ref(x, w, b, off, mask, go, kh, kw, sh, sw, ph, pw, dh, dw, dg):
    """[grad_input, grad_offset, grad_mask, grad_weight, grad_bias] as the reference's CPU op computes them (CPU float32)."""
    x, w, off, mask, go = (t.detach().cpu().contiguous().float() for t in (x, w, off, mask, go))
    B, C, H, W = x.shape
    Co = w.shape[0]
    Ho, Wo = out_size(H, W, kh, kw, sh, sw, ph, pw, dh, dw)
    gin, goff, gmask = torch.zeros_like(x), torch.zeros_like(off), torch.zeros_like(mask)
    gw = torch.zeros(Co, C * kh * kw, dtype=torch.float64)
    gb = torch.zeros(Co, dtype=torch.float64)
    w2 = w.reshape(Co, -1).double()
    coord, col2im = _ref("modulated_deformable_col2im_coord_cpu"), _ref("modulated_deformable_col2im_cpu")
    geo = (1, C, H, W, Ho, Wo, kh, kw, ph, pw, sh, sw, dh, dw, dg)
    for n in range(B):
        g2 = go[n].reshape(Co, -1).double()
        columns = (w2.t() @ g2).float().contiguous()  # dcn_v2_cpu.cpp:175-178
        xn, on, mn = x[n].contiguous(), off[n].contiguous(), mask[n].contiguous()
        coord(columns.data_ptr(), xn.data_ptr(), on.data_ptr(), mn.data_ptr(), *geo, goff[n].data_ptr(), gmask[n].data_ptr())
        gi = torch.zeros_like(xn)
        col2im(columns.data_ptr(), on.data_ptr(), mn.data_ptr(), *geo, gi.data_ptr())
        gin[n] = gi
        col, _, _ = odcn.im2col(x[n:n + 1], off[n:n + 1], mask[n:n + 1], kh, kw, ph, pw, sh, sw, dh, dw, dg, kind="reference")
        gw += g2 @ col[0].double().t()  # dcn_v2_cpu.cpp:218-221
        gb += g2.sum(1)                  # :226-229
    return [gin, goff, gmask, gw.float().view(Co, C, kh, kw), gb.float()]


def _forward_f64(x, w, b, off, mask, kh, kw, sh, sw, ph, pw_pos, dh, dw, dg, Ho, Wo):
    """Vectorised float64 DCNv2 forward with the output grid (Ho, Wo) given and pw_pos the horizontal pad used for the
    sample positions.  Positions are the reference's float32 values; gradients flow through the offsets at slope 1."""
    B, C, H, W = x.shape
    Co, T, cpg = w.shape[0], kh * kw, C // dg
    ys = torch.arange(Ho).view(Ho, 1)
    xs = torch.arange(Wo).view(1, Wo)
    bi = torch.arange(B).view(B, 1, 1)
    cols = []
    for g in range(dg):
        per_tap = []
        for t in range(T):
            i, j = divmod(t, kw)
            oh, ow = off[:, g * 2 * T + 2 * t], off[:, g * 2 * T + 2 * t + 1]
            m = mask[:, g * T + t]
            py32 = (ys * sh - ph + i * dh).float() + oh.detach().float()
            px32 = (xs * sw - pw_pos + j * dw).float() + ow.detach().float()
            py = py32.double() + (oh - oh.detach())
            px = px32.double() + (ow - ow.detach())
            valid = (py32 > -1) & (px32 > -1) & (py32 < H) & (px32 < W)
            y0, x0 = torch.floor(py32).long(), torch.floor(px32).long()
            lh, lw = py - y0.double(), px - x0.double()
            val = 0
            for yy, xx, wt in ((y0, x0, (1 - lh) * (1 - lw)), (y0, x0 + 1, (1 - lh) * lw),
                               (y0 + 1, x0, lh * (1 - lw)), (y0 + 1, x0 + 1, lh * lw)):
                ok = valid & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
                v = x[bi, g * cpg:(g + 1) * cpg, yy.clamp(0, H - 1), xx.clamp(0, W - 1)]  # [B,Ho,Wo,cpg]
                val = val + v * (wt * ok.double()).unsqueeze(-1)
            per_tap.append(val * m.unsqueeze(-1))
        cols.append(torch.stack(per_tap, -1))  # [B,Ho,Wo,cpg,T]
    col = torch.cat(cols, 3)                    # [B,Ho,Wo,C,T]
    return torch.einsum("oct,bhwct->bohw", w.view(Co, C, T), col) + b.view(1, Co, 1, 1)


def backward_f64(x, w, b, off, mask, go, kh, kw, sh, sw, ph, pw, dh, dw, dg, quirk=True):
    """Float64 gradients of the forward (CPU float64 tensors)."""
    B, C, H, W = x.shape
    Ho, Wo = out_size(H, W, kh, kw, sh, sw, ph, pw, dh, dw)
    leaves = [t.detach().cpu().double().requires_grad_(True) for t in (x, w, b, off, mask)]
    g = go.detach().cpu().double()
    y = _forward_f64(*leaves, kh, kw, sh, sw, ph, pw, dh, dw, dg, Ho, Wo)
    gx, gw, gb, goff, gmask = torch.autograd.grad(y, leaves, g)
    if quirk and ph != pw:
        xi = x.detach().cpu().double().requires_grad_(True)
        yq = _forward_f64(xi, *(t.detach() for t in leaves[1:]), kh, kw, sh, sw, ph, ph, dh, dw, dg, Ho, Wo)
        gx, = torch.autograd.grad(yq, [xi], g)
    return [gx, goff, gmask, gw, gb]
