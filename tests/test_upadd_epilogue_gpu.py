"""IDAUp's up-sample + add inside the epilogue of the DCN node that produces `add` (dcn16t.hip UPADD, engine_forward.hip ida()).

Three sites of dla_34 take the fused form when their node runs on dcn16t in f16x3: dla_up.ida_2 iterations 2 and 3 (f = 2) and
ida_up iteration 2 (f = 4).  node_{k-1} then stores u_k = relu(bn(dcn)) + up_k(t_k) and its own output does not exist.

The unfused reference.  A tap on any `.node_` tensor, CP_SEL_DCN16T_NEVER, float32 and small (split-K) launches all select the
plain sequence.  For a bit-for-bit comparison the two forms must not differ in anything else, and plain DCN16T_NEVER does: at every
batch some 64-output DCN layer moves from dcn16t to dcn16p (another summation order; e.g. at B = 8 .. 31 the nodes, from B = 32 the
128 -> 64 projections), on the parent commit as well.  So the pair compared with torch.equal is
    fused:    DCN16P_ALWAYS | DCN16T_ALWAYS                   (every eligible DCN on dcn16t)
    unfused:  DCN16P_ALWAYS | DCN16S_ALWAYS | DCN16T_NEVER    (the same layers on dcn16s, documented and tested bit-identical
                                                               to dcn16t: test_dcn16t_equals_dcn16s_where_their_modes_differ)
at a batch where the nodes are dcn16t launches by default too (B = 8 at 512 x 512: 1024 workgroups) and at small shapes.  The
default selection itself (no switch) is checked at B = 8 bit for bit on the heads' input (`feat` against the same tensor tapped as
`ida_up.node_2`, which runs the unfused sequence on the same kernels), against float64 and through the launch profile; its distance
to plain DCN16T_NEVER is printed, not asserted (see above).

float64 bound of u = o + sum of four products: five float32 roundings (four FMAs, one add), each at most 2^-24 of a partial
result that is at most S = |o| + sum |t w| in magnitude: |u - ref| <= 6 * 2^-24 * S per element (one rounding of slack)."""
import pytest
import torch
import torch.nn.functional as F

from centerpose_amd import hip, synth

pytestmark = pytest.mark.gpu
S = hip.KernelSel
FUSED = S.DCN16P_ALWAYS | S.DCN16T_ALWAYS
UNFUSED = S.DCN16P_ALWAYS | S.DCN16S_ALWAYS | S.DCN16T_NEVER
# (ida, iteration k, f): u_k = up_k(proj_k) + node_{k-1}
SITES = [("dla_up.ida_2", 2, 2), ("dla_up.ida_2", 3, 2), ("ida_up", 2, 4)]
DCN16T = "dcn16t_f16x3_p128n64"
# B, H, W: feature maps of H/4 x W/4 in 8 x 16 patches; >= 128 patches, else the nodes are split-K launches (never fused)
SHAPES = [(8, 512, 512), (2, 256, 512), (4, 320, 256)]


def _model():
    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("dla_34", heads)
    return hip.HipModel("dla_34", heads, sd, precision="f16x3"), sd


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


def _t_bytes(B, H, W):
    hf, wf = H // 4, W // 4
    return 4.0 * B * 64 * (2 * (hf // 2) * (wf // 2) + (hf // 4) * (wf // 4))


def _check_f64(sd, ida, k, f, u, t, o):
    w = sd["%s.up_%d.weight" % (ida, k)].double().to(u.device)
    ref = F.conv_transpose2d(t.double(), w, None, stride=f, padding=f // 2, groups=w.shape[0]) + o.double()
    mag = F.conv_transpose2d(t.double().abs(), w.abs(), None, stride=f, padding=f // 2, groups=w.shape[0]) + o.double().abs()
    err = (u.double() - ref).abs()
    excess = float((err - 6.0 * 2.0 ** -24 * mag).max())
    print("%s.up_%d f=%d: max |u - f64| = %.3e, max |u| = %.3e, max (err - bound) = %.3e" % (
        ida, k, f, float(err.max()), float(ref.abs().max()), excess))
    assert u.shape == ref.shape and float(ref.abs().max()) > 0
    assert excess <= 0.0, (ida, k, excess)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_fused_equals_unfused_bit_for_bit(device, B, H, W):
    model, sd = _model()
    x = synth.frames(B, seed=41, h=H, w=W).to(device)
    # the fused form really runs: the three node launches are charged for t, and a tap on a node takes that away
    by_f, n_f = _dcn16t_bytes(model, x, FUSED)
    by_u, n_u = _dcn16t_bytes(model, x, FUSED, tap="ida_up.node_1")
    print("dcn16t launches %d / %d, bytes fused - unfused = %.0f (t: %.0f)" % (n_f, n_u, by_f - by_u, _t_bytes(B, H, W)))
    assert n_f == n_u and abs((by_f - by_u) - _t_bytes(B, H, W)) < 1.0
    for ida, k, f in SITES:
        name = "%s.up_%d" % (ida, k)
        u_f = _tap(model, x, name, FUSED)
        u_u = _tap(model, x, name, UNFUSED)
        assert u_f.shape == (B, 64, H // 4, W // 4)
        assert torch.equal(u_f, u_u), (name, float((u_f - u_u).abs().max()))
        # the elided node: tapping it returns what the unfused sequence computes, and u is that + up(t) (float64)
        node = "%s.node_%d" % (ida, k - 1)
        o_f = _tap(model, x, node, FUSED)
        o_u = _tap(model, x, node, UNFUSED)
        assert torch.equal(o_f, o_u), node
        t = _tap(model, x, "%s.proj_%d" % (ida, k), FUSED)
        assert t.shape == (B, 64, H // 4 // f, W // 4 // f)
        _check_f64(sd, ida, k, f, u_f, t, o_f)
    # all heads, 20 forwards each way (launch-to-launch differences: the |max| slot is an atomic max, order-independent)
    with hip.select_kernels(UNFUSED):
        z_u = {k: v.clone() for k, v in model.forward(x).items()}
    for it in range(20):
        with hip.select_kernels(FUSED):
            z_f = model.forward(x)
            for k in z_u:
                assert torch.equal(z_f[k], z_u[k]), (it, k)
        with hip.select_kernels(UNFUSED):
            z = model.forward(x)
            for k in z_u:
                assert torch.equal(z[k], z_u[k]), (it, k)


def test_default_selection_fuses_and_matches_float64(device):
    """No switch, B = 8 at 512 x 512: the 64 -> 64 @128^2 nodes are dcn16t launches (1024 workgroups) and take the fused form."""
    B, H, W = 8, 512, 512
    model, sd = _model()
    x = synth.frames(B, seed=43, h=H, w=W).to(device)
    by_f, n_f = _dcn16t_bytes(model, x, 0)
    by_u, n_u = _dcn16t_bytes(model, x, 0, tap="dla_up.ida_2.node_1")
    print("default: dcn16t launches %d / %d, bytes fused - unfused = %.0f (t: %.0f)" % (n_f, n_u, by_f - by_u, _t_bytes(B, H, W)))
    assert n_f == n_u and abs((by_f - by_u) - _t_bytes(B, H, W)) < 1.0
    for ida, k, f in SITES:
        u = _tap(model, x, "%s.up_%d" % (ida, k), 0)
        o = _tap(model, x, "%s.node_%d" % (ida, k - 1), 0)   # (the tap selects the unfused sequence, same kernels)
        t = _tap(model, x, "%s.proj_%d" % (ida, k), 0)
        _check_f64(sd, ida, k, f, u, t, o)
        # plain DCN16T_NEVER moves the nodes to dcn16p at this batch (another summation order): reported only
        u_n = _tap(model, x, "%s.up_%d" % (ida, k), S.DCN16T_NEVER)
        print("%s.up_%d: max |default - DCN16T_NEVER| = %.3e (max |u| %.3e)" % (
            ida, k, float((u - u_n).abs().max()), float(u.abs().max())))
    # bit for bit against the unfused sequence on the SAME kernels: the heads' input is ida_up.node_2 -- tapped under that name the
    # pass runs unfused (a tap on a node), under the name `feat` it runs fused
    feat_f = _tap(model, x, "feat", 0)
    feat_u = _tap(model, x, "ida_up.node_2", 0)
    assert feat_f.shape == (B, 64, H // 4, W // 4) and float(feat_f.abs().max()) > 0
    assert torch.equal(feat_f, feat_u), float((feat_f - feat_u).abs().max())
    z0 = {k: v.clone() for k, v in model.forward(x).items()}
    for it in range(20):
        z = model.forward(x)
        for k in z0:
            assert torch.equal(z[k], z0[k]), (it, k)


def test_float32_and_split_k_launches_keep_the_plain_sequence(device):
    """Where the node's launch is not dcn16t's -- exact-f32 mode, or a launch small enough for split-K -- nothing is fused and the up
    tap is still there."""
    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("dla_34", heads)
    x = synth.frames(1, seed=47, h=128, w=128).to(device)
    for prec in ("f32", "f16x3"):
        model = hip.HipModel("dla_34", heads, sd, precision=prec)
        with hip.select_kernels(FUSED if prec == "f16x3" else 0):
            for ida, k, f in SITES:
                _, u = model.forward(x, tap="%s.up_%d" % (ida, k))
                u = u.clone()
                _, o = model.forward(x, tap="%s.node_%d" % (ida, k - 1))
                o = o.clone()
                _, t = model.forward(x, tap="%s.proj_%d" % (ida, k))
                _check_f64(sd, ida, k, f, u, t.clone(), o)
