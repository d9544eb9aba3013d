"""dcn16t's up-sample + add epilogue with its taps of t read from LDS (dcn16t.hip, UPADD): a workgroup stages the rectangle of t
behind its 8 x 16 patch once -- rows ty0 / f - 1 .. (ty0 + 8) / f, columns likewise, zeros where t has no pixel -- and every lane
reads its 2 x 2 taps from there.  The shapes aim at that rectangle's logic; all four fused sites are compared: dla_up.ida_2
iterations 2 and 3 (f = 2), ida_up iteration 1, stored by dla_up.ida_2's last node (f = 2), and ida_up iteration 2 (f = 4).

The pair compared with torch.equal is test_upadd_epilogue_gpu.py's (the reasons are given there):
    fused:    DCN16P_ALWAYS | DCN16T_ALWAYS
    unfused:  DCN16P_ALWAYS | DCN16S_ALWAYS | DCN16T_NEVER

Shapes (B, H, W; the sites work on maps of H/4 x W/4).  The engine fuses only whole launches, and a DCN launch of fewer than 128
patches is a split-K launch; so each shape below is the nearest one with at least 128 patches to the shape that was asked for,
with the batch raised and the map left as it was:
  * (128, 32, 64) for (1, 32, 64): ONE patch per image -- all four borders of t fall in one workgroup, with the taps outside t
    on both sides (row and column -1, and (ty0 + 8) / f = t's height, likewise its width) and another image next in memory;
  * (64, 64, 64) for (3, 64, 64): two patches per image, one above the other: the lower patch's first staged row is the upper
    patch's, the upper patch's row -1 and the lower patch's last row must not come from the neighbouring images;
  * (15, 96, 192) for (2, 96, 192): maps of 24 x 48 (3 x 3 patches, no power of two): interior patches, whose whole rectangle
    exists, next to border patches.

float64 bound of u = o + sum of four products (as test_upadd_epilogue_gpu.py): five float32 roundings, each at most 2^-24 of a
partial result of magnitude at most S = |o| + sum |t w|: |u - ref| <= 6 * 2^-24 * S per element."""
import pytest
import torch
import torch.nn.functional as F

from centerpose_amd import hip, synth

pytestmark = pytest.mark.gpu
S = hip.KernelSel
FUSED = S.DCN16P_ALWAYS | S.DCN16T_ALWAYS
UNFUSED = S.DCN16P_ALWAYS | S.DCN16S_ALWAYS | S.DCN16T_NEVER
DCN16T = "dcn16t_f16x3_p128n64"
# (u, also the name of the ConvTranspose2d whose weight it uses; the node whose epilogue stores it; the up-sampled t; f)
SITES = [("dla_up.ida_2.up_2", "dla_up.ida_2.node_1", "dla_up.ida_2.proj_2", 2),
         ("dla_up.ida_2.up_3", "dla_up.ida_2.node_2", "dla_up.ida_2.proj_3", 2),
         ("ida_up.up_1", "dla_up.ida_2.node_3", "ida_up.proj_1", 2),
         ("ida_up.up_2", "ida_up.node_1", "ida_up.proj_2", 4)]
SHAPES = [(128, 32, 64), (64, 64, 64), (15, 96, 192)]


def _tap(model, x, name, sel):
    with hip.select_kernels(sel):
        _, t = model.forward(x, tap=name)
        return t.clone()


def _dcn16t_bytes(model, x, sel, tap=None):
    with hip.select_kernels(sel):
        model.profile(True)
        if tap is None:
            model.forward(x)
        else:
            model.forward(x, tap=tap)
        torch.cuda.synchronize()
        ran = model.profile_read()
        model.profile(False)
    assert DCN16T in ran, sorted(ran)
    return ran[DCN16T]["bytes"], ran[DCN16T]["launches"]


def _check_f64(sd, name, f, u, t, o):
    w = sd[name + ".weight"].double().to(u.device)
    ref = F.conv_transpose2d(t.double(), w, None, stride=f, padding=f // 2, groups=w.shape[0]) + o.double()
    mag = F.conv_transpose2d(t.double().abs(), w.abs(), None, stride=f, padding=f // 2, groups=w.shape[0]) + o.double().abs()
    err = (u.double() - ref).abs()
    excess = float((err - 6.0 * 2.0 ** -24 * mag).max())
    print("%s f=%d: max |u - f64| = %.3e, max |u| = %.3e, max (err - bound) = %.3e" % (
        name, f, float(err.max()), float(ref.abs().max()), excess))
    assert u.shape == ref.shape and float(ref.abs().max()) > 0
    assert excess <= 0.0, (name, excess)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_lds_taps_fused_equals_unfused_bit_for_bit(device, B, H, W):
    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("dla_34", heads)
    model = hip.HipModel("dla_34", heads, sd, precision="f16x3")
    x = synth.frames(B, seed=71, h=H, w=W).to(device)
    hf, wf = H // 4, W // 4
    # all four sites really take the fused form at this shape: their dcn16t launches are charged for t, and a tap on the
    # boundary node takes that away
    by_f, n_f = _dcn16t_bytes(model, x, FUSED)
    by_u, n_u = _dcn16t_bytes(model, x, FUSED, tap="dla_up.ida_2.node_3")
    t_bytes = 4.0 * B * 64 * (3 * (hf // 2) * (wf // 2) + (hf // 4) * (wf // 4))
    print("dcn16t launches %d / %d, bytes fused - unfused = %.0f (t: %.0f)" % (n_f, n_u, by_f - by_u, t_bytes))
    assert n_f == n_u and abs((by_f - by_u) - t_bytes) < 1.0
    with hip.select_kernels(UNFUSED):
        z_u = {k: v.clone() for k, v in model.forward(x).items()}
    ref = {}
    for rep in range(2):  # every case twice: both passes against the one unfused reference, so bit for bit against each other
        for name, node, proj, f in SITES:
            u_f = _tap(model, x, name, FUSED)
            assert u_f.shape == (B, 64, hf, wf)
            if rep == 0:
                ref[name] = _tap(model, x, name, UNFUSED)
                o = _tap(model, x, node, UNFUSED)
                t = _tap(model, x, proj, UNFUSED)
                assert t.shape == (B, 64, hf // f, wf // f)
                _check_f64(sd, name, f, u_f, t, o)
            assert torch.equal(u_f, ref[name]), (rep, name, float((u_f - ref[name]).abs().max()))
        with hip.select_kernels(FUSED):
            z_f = model.forward(x)
            for k in z_u:
                assert torch.equal(z_f[k], z_u[k]), (rep, k)
