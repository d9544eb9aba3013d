"""The level entries' 1x1 projection inside the epilogue of the block's conv2 (halo16.hip PJ, engine_forward.hip tree1()).

dla_34 has four level entries with cin != cout (base.level2, base.level3.tree1, base.level4.tree1, base.level5).  Each computes
proj = bn_p(W_p . maxpool(x)) with a 1x1 launch (pw16.hip) and conv2 of its first block reads proj back as the residual.  Where
that conv2 is a whole (not split-K) halo16 launch on the 64- or 128-wide tile in f16x3, the workgroup computes the projection of
its own 8 x 16 pixels after its K loop -- pw16.hip's operands, K order and term order -- and adds it where `res` was added: the
projected tensor and its launch do not exist.

The unfused reference.  There is no free CP_SEL_* bit for a switch of its own (31 usable bits, bit 11 retired), so the engine
keeps the plain sequence wherever the projection's kernel is asked for by name: CP_SEL_PW16_FRAG_A runs every 1x1 layer on
pw16_kernel, documented and tested bit-identical to the default pw16s_kernel, and the projection as a launch of its own.  A tap
on any `<entry>.project` does the same (for every entry, so that the launch sequence has two forms).  Both are used below.

Decisions and work space.  The engine decides from shapes and switches alone, and every sequence a real pass can take -- entries
fused or not, IDAUp sites all fused / none / the boundary one only, stem fused or not, tap or not -- is one of the forms the
work-space query runs dry.  test_decisions_and_work_space checks the decision (through the launch profile) and that the peak a
real pass reached (cp_model_workspace_used) is within the query's answer, form by form.

Which entries fuse is decided by the same split-K plan as every other launch (fewer than 128 output tiles: split-K, never
fused), so at the small shapes only level 2 is a whole halo16 launch; B = 16 at 512 x 512 is the smallest batch at which
level 5's conv2 (two patches per image, four N tiles) is one, and there all four fuse.

float64 bound.  y = relu(bn2(conv2(t)) + bn_p(W_p . bottom)), K = 9 cout + cin products in all.  f16x3 keeps hi*hi + hi*lo +
lo*hi of operands split into two binary16 halves: the dropped lo*lo term is at most 2^-22 |a w|, and each operand's split leaves
at most 2^-22 of it behind, so a product is off by at most 3 * 2^-22 |a w|.  Every float32 accumulation, the two scale / shift
FMAs and the final add round once, each by at most 2^-24 of a partial result bounded by S = sum |a w| |scale| + |shift| over both
branches: |y - ref| <= (3 * 2^-22 + (K + 4) * 2^-24) * S."""
import pytest
import torch
import torch.nn.functional as F

from centerpose_amd import hip, synth
from oracle.backbone import BN_EPS

pytestmark = pytest.mark.gpu
S = hip.KernelSel
FUSED = 0
UNFUSED = S.PW16_FRAG_A
# entry prefix, cin, cout, the tensor the entry reads
ENTRIES = [("base.level2", 32, 64, "base.level1"), ("base.level3.tree1", 64, 128, "base.level2"),
           ("base.level4.tree1", 128, 256, "base.level3"), ("base.level5", 256, 512, "base.level4")]
PW16 = ("pw16_f16x3_m128n64", "pw16_f16x3_m128n128")
# (B, H, W) -> entries that fuse (see above)
SHAPES = [(2, 256, 512, 1), (4, 320, 256, 1), (3, 256, 512, 1), (16, 512, 512, 4)]

_cache = {}


def _model():
    if "m" not in _cache:
        heads = synth.HEADS_POSE
        sd = synth.make_state_dict("dla_34", heads)
        _cache["m"] = (hip.HipModel("dla_34", heads, sd, precision="f16x3"), sd)
    return _cache["m"]


def _tap(model, x, name, sel=0):
    with hip.select_kernels(sel):
        _, t = model.forward(x, tap=name)
        return t.clone()


def _profile(model, x, sel):
    with hip.select_kernels(sel):
        model.profile(True)
        model.forward(x)
        torch.cuda.synchronize()
        ran = model.profile_read()
        roles = model.profile_roles()
        model.profile(False)
    return ran, roles


def _bn(sd, name, dev):
    g = sd[name + ".weight"].double() / torch.sqrt(sd[name + ".running_var"].double() + BN_EPS)
    return g.to(dev), (sd[name + ".bias"].double() - sd[name + ".running_mean"].double() * g).to(dev)


def _check_f64(sd, p, cin, cout, y, t, x_in):
    dev = y.device
    bottom = F.max_pool2d(x_in, 2, 2).double()
    w2 = sd[p + ".tree1.conv2.weight"].double().to(dev)
    wp = sd[p + ".project.0.weight"].double().to(dev)
    g2, b2 = _bn(sd, p + ".tree1.bn2", dev)
    gp, bp = _bn(sd, p + ".project.1", dev)
    v = lambda a: a.view(1, -1, 1, 1)
    ref = F.relu(F.conv2d(t.double(), w2, None, 1, 1) * v(g2) + v(b2) + F.conv2d(bottom, wp) * v(gp) + v(bp))
    mag = (F.conv2d(t.double().abs(), w2.abs(), None, 1, 1) * v(g2.abs()) + v(b2.abs()) +
           F.conv2d(bottom.abs(), wp.abs()) * v(gp.abs()) + v(bp.abs()))
    K = 9 * cout + cin
    err = (y.double() - ref).abs()
    excess = float((err - (3 * 2.0 ** -22 + (K + 4) * 2.0 ** -24) * mag).max())
    print("%s: max |y - f64| = %.3e, max |y| = %.3e, max (err - bound) = %.3e" % (p, float(err.max()), float(ref.abs().max()), excess))
    assert y.shape == ref.shape and float(ref.abs().max()) > 0
    assert excess <= 0.0, (p, excess)


@pytest.mark.parametrize("B,H,W,nfused", SHAPES)
def test_fused_equals_unfused_bit_for_bit(device, B, H, W, nfused):
    model, sd = _model()
    x = synth.frames(B, seed=53, h=H, w=W).to(device)
    # the fused form really runs: that many 1x1 launches fewer, their work charged to the 3x3 launches
    ran_f, roles_f = _profile(model, x, FUSED)
    ran_u, roles_u = _profile(model, x, UNFUSED)
    n_f = sum(ran_f[k]["launches"] for k in PW16 if k in ran_f)
    n_u = sum(ran_u[k]["launches"] for k in PW16 if k in ran_u)
    print("pw16 launches fused %d, unfused %d; conv1x1 role %d / %d" % (n_f, n_u, roles_f["conv1x1"]["launches"],
                                                                        roles_u["conv1x1"]["launches"]))
    assert n_u - n_f == nfused
    assert roles_u["conv1x1"]["launches"] - roles_f["conv1x1"]["launches"] == nfused
    assert roles_u["conv"]["launches"] == roles_f["conv"]["launches"]
    flops_f = sum(r["flops"] for r in roles_f.values())
    flops_u = sum(r["flops"] for r in roles_u.values())
    assert abs(flops_f - flops_u) <= 1e-9 * flops_u, (flops_f, flops_u)
    # first block of every entry
    for p, cin, cout, _ in ENTRIES:
        y_f = _tap(model, x, p + ".tree1", FUSED)
        y_u = _tap(model, x, p + ".tree1", UNFUSED)
        assert y_f.shape[1] == cout and float(y_f.abs().max()) > 0
        assert torch.equal(y_f, y_u), (p, float((y_f - y_u).abs().max()))
    # all heads, 20 forwards each way, odd ones with the batch reversed
    with hip.select_kernels(UNFUSED):
        z_u = {k: v.clone() for k, v in model.forward(x).items()}
    xr = x.flip(0).contiguous()
    for it in range(20):
        for sel in (FUSED, UNFUSED):
            with hip.select_kernels(sel):
                z = model.forward(xr if it & 1 else x)
                for k in z_u:
                    zk = z[k].flip(0) if it & 1 else z[k]
                    assert torch.equal(zk, z_u[k]), (it, int(sel), k)


@pytest.mark.parametrize("B,H,W,idx", [(3, 256, 512, 0), (16, 512, 512, 3)])
def test_fused_entry_matches_float64(device, B, H, W, idx):
    """Level 2 (64-wide tile, K = 32) and level 5 (128-wide tile, K = 256) against float64; a tap on the entry's projection runs
    that entry unfused and returns the tensor the fused form never writes, checked against float64 as well."""
    model, sd = _model()
    x = synth.frames(B, seed=59, h=H, w=W).to(device)
    p, cin, cout, src = ENTRIES[idx]
    y = _tap(model, x, p + ".tree1")
    t = _tap(model, x, p + ".tree1.conv1")
    x_in = _tap(model, x, src)
    _check_f64(sd, p, cin, cout, y, t, x_in)
    proj = _tap(model, x, p + ".project")
    assert proj.shape == (B, cout, y.shape[2], y.shape[3]) and float(proj.abs().max()) > 0
    gp, bp = _bn(sd, p + ".project.1", x.device)
    wp = sd[p + ".project.0.weight"].double().to(x.device)
    ref_p = F.conv2d(F.max_pool2d(x_in, 2, 2).double(), wp) * gp.view(1, -1, 1, 1) + bp.view(1, -1, 1, 1)
    mag_p = F.conv2d(F.max_pool2d(x_in, 2, 2).double().abs(), wp.abs()) * gp.abs().view(1, -1, 1, 1) + bp.abs().view(1, -1, 1, 1)
    assert float(((proj.double() - ref_p).abs() - (3 * 2.0 ** -22 + (cin + 2) * 2.0 ** -24) * mag_p).max()) <= 0.0


def test_float32_and_switches_keep_the_plain_sequence(device):
    """Exact-f32 mode and the switches that take conv2 off halo16 or the projection off pw16s run the projection as a launch."""
    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("dla_34", heads)
    x = synth.frames(2, seed=61, h=256, w=512).to(device)
    m32 = hip.HipModel("dla_34", heads, sd, precision="f32")
    _, proj = m32.forward(x, tap="base.level2.project")
    assert proj.shape == (2, 64, 64, 128)
    model, _ = _model()
    ran0, roles0 = _profile(model, x, 0)
    for sel in (S.PW16_FRAG_A, S.PW16_NEVER, S.HALO_NEVER, S.HALO_LDS_WEIGHTS):
        ran, roles = _profile(model, x, sel)
        assert roles["conv1x1"]["launches"] == roles0["conv1x1"]["launches"] + 1, sel


def _conv1x1(model, x, sel, tap):
    """conv1x1-role launches and the work-space peak of one real pass with that tap under those switches."""
    with hip.select_kernels(sel):
        need = model.workspace_bytes(*((x.shape[0],) + tuple(x.shape[2:])))
        model.profile(True)
        model.forward(x, tap=tap) if tap else model.forward(x)
        torch.cuda.synchronize()
        used = model.workspace_used()
        model.profile_read()
        n = model.profile_roles()["conv1x1"]["launches"]
        model.profile(False)
    return n, used, need


# (B, H, W) -> entries that fuse: the three shapes above, one where every launch is split-K, one where all four fuse
@pytest.mark.parametrize("B,H,W,nfused", [(2, 256, 512, 1), (4, 320, 256, 1), (3, 256, 512, 1), (1, 128, 128, 0), (16, 512, 512, 4)])
def test_decisions_and_work_space(device, B, H, W, nfused):
    model, sd = _model()
    x = synth.frames(B, seed=71, h=H, w=W).to(device)
    DCN = S.DCN16P_ALWAYS | S.DCN16T_ALWAYS  # (the IDAUp sites fuse at the small shapes as well)
    # a neutral tap (fused heads off, nothing else) is the reference count of the tapped forms
    n_plain, _, _ = _conv1x1(model, x, 0, None)
    n_tap, _, _ = _conv1x1(model, x, 0, "base.level1")
    forms = [("default", 0, None, n_plain), ("PW16_FRAG_A", S.PW16_FRAG_A, None, n_plain + nfused),
             ("HALO_NEVER", S.HALO_NEVER, None, n_plain + nfused), ("neutral tap", 0, "base.level1", n_tap),
             ("tap on a projection", 0, "base.level3.tree1.project", n_tap + nfused),
             ("tap on an entry block", 0, "base.level2.tree1", n_tap),
             ("IDAUp fused", DCN, None, n_plain), ("IDAUp: tap on an inner node", DCN, "ida_up.node_1", n_tap),
             ("IDAUp: tap on the boundary node", DCN, "dla_up.ida_2.node_3", n_tap),
             ("IDAUp unfused", DCN | S.DCN16S_ALWAYS | S.DCN16T_NEVER, None, n_plain),
             ("stem unfused", S.STEM_LEVEL0_UNFUSED, None, n_plain)]
    for name, sel, tap, want in forms:
        n, used, need = _conv1x1(model, x, sel, tap)
        print("%-32s conv1x1 launches %2d (want %2d)  work space used %10d of %10d" % (name, n, want, used, need))
        assert n == want, name
        assert 0 < used <= need, (name, used, need)
    m32 = hip.HipModel("dla_34", synth.HEADS_POSE, sd, precision="f32")
    n32, used, need = _conv1x1(m32, x, 0, None)
    n32p, used_p, need_p = _conv1x1(m32, x, 0, "base.level2.project")
    n32t, _, _ = _conv1x1(m32, x, 0, "base.level1")
    print("float32: conv1x1 launches %d / %d with a tap on a projection / %d neutral tap, work space %d of %d" % (n32, n32p, n32t, used, need))
    assert n32p == n32t and 0 < used <= need and 0 < used_p <= need_p  # nothing to unfuse in float32
