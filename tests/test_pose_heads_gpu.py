"""GPU tests of the prediction-head block (cp_pose_heads_forward / _backward, cp_model_features, PoseHeads) against the
float64 reference of tests/pose_heads_ref.py.  Tolerances are the project's own: forward 2e-5 * max(1, max|ref|) (the
convolution tests of tests/test_gpu_parity.py), each gradient 1e-4 * max|ref| (the DCN backward tests).  The strict cases
use dyadic inputs, whose hidden values are exact and never at the ReLU kink; the realistic cases add the computed allowance
for the hidden units float32 and float64 may gate differently."""
import numpy as np
import pytest
import torch

from centerpose_amd import hip, synth
from centerpose_amd.lib.models.model import create_model
from centerpose_amd.pose_heads import PoseHeads
from tests import pose_heads_ref as R

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL = 2e-5, 1e-4
NAMES = ("grad_w0", "grad_b0", "grad_w1", "grad_b1")


def _to(dev, case):
    feat = case.feat.to(dev).contiguous(memory_format=torch.channels_last)
    params = [tuple(t.to(dev) for t in p) for p in case.params]
    gos = [g.to(dev) if g is not None else None for g in case.grad_outs]
    return feat, params, gos


def _check_forward(outs, ref, where):
    for i, (o, r) in enumerate(zip(outs, ref["outs"])):
        err, tol = float((o.cpu().double() - r).abs().max()), FWD_TOL * max(1.0, float(r.abs().max()))
        print("%s head %d: forward err %.3e (tol %.3e)" % (where, i, err, tol))
        assert o.shape == r.shape and err <= tol, (where, i, err, tol)


def _check_grads(gfeat, grads, ref, where, allow=None, tol=GRAD_TOL):
    """Every gradient within tol * max|ref| (+ the element-wise allowance of a realistic case)."""
    def one(name, dev, r, al):
        d = (dev.cpu().double() - r).abs()
        bound = tol * float(r.abs().max())
        extra = al if al is not None else torch.zeros(())
        print("%s %s: err %.3e (tol %.3e, max|ref| %.3e, allowance up to %.3e)"
              % (where, name, float(d.max()), bound, float(r.abs().max()), float(extra.max())))
        assert dev.shape == r.shape and bool((d <= bound + extra).all()), (where, name, float(d.max()), bound)

    if gfeat is not None:
        one("grad_feat", gfeat, ref["gfeat"], allow["gfeat"] if allow else None)
    for i, (gd, gr) in enumerate(zip(grads, ref["grads"])):
        for k in range(4):
            one("head %d %s" % (i, NAMES[k]), gd[k], gr[k], allow["grads"][i][k] if allow else None)


def _dyadic(name, go_scale=1.0):
    return R.dyadic_case(sum(map(ord, name)), *R.DYADIC_SHAPES[name], go_scale=go_scale)


@pytest.mark.parametrize("name", sorted(R.DYADIC_SHAPES))
def test_forward_and_gradients_dyadic(device, name):
    case = _dyadic(name)
    feat, params, gos = _to(device, case)
    ref = R.reference(case.feat, case.params, case.grad_outs)
    try:
        for prec in ("f32", "f16x3"):
            hip.set_default_precision(prec)
            _check_forward(hip.pose_heads_forward(feat, params), ref, "%s %s" % (name, prec))
    finally:
        hip.set_default_precision("f32")
    gfeat, grads = hip.pose_heads_backward(feat, params, gos)
    assert gfeat.is_contiguous(memory_format=torch.channels_last)
    _check_grads(gfeat, grads, ref, name)
    # an NCHW-contiguous feature map is the same call
    g2, grads2 = hip.pose_heads_backward(case.feat.to(device), params, gos)
    assert torch.equal(g2, gfeat) and all(torch.equal(a, b) for x, y in zip(grads, grads2) for a, b in zip(x, y))


def test_backward_is_exact_float32_under_f16x3(device):
    case = _dyadic("resdcn")
    feat, params, gos = _to(device, case)
    a = hip.pose_heads_backward(feat, params, gos)
    try:
        hip.set_default_precision("f16x3")
        b = hip.pose_heads_backward(feat, params, gos)
    finally:
        hip.set_default_precision("f32")
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for p, q in zip(a[1], b[1]) for x, y in zip(p, q))


def test_heads_without_a_gradient(device):
    case = _dyadic("resdcn")
    feat, params, gos = _to(device, case)
    for drop in ((1, 4), (0, 2, 3, 5, 6), tuple(range(7))):
        cpu_gos = [None if i in drop else g for i, g in enumerate(case.grad_outs)]
        dev_gos = [None if i in drop else g for i, g in enumerate(gos)]
        ref = R.reference(case.feat, case.params, cpu_gos)
        gfeat, grads = hip.pose_heads_backward(feat, params, dev_gos)
        for i in drop:
            assert all(not bool(g.any()) for g in grads[i]), (drop, i)
        if len(drop) == 7:
            assert not bool(gfeat.any())
            continue
        _check_grads(gfeat, grads, ref, "dropped %s" % (drop,))


def test_frozen_backbone_leaves_grad_feat_alone(device):
    case = _dyadic("resdcn")
    feat, params, gos = _to(device, case)
    poison = torch.full_like(feat, 1234.5)
    gfeat, grads = hip.pose_heads_backward(feat, params, gos, grad_feat=poison.clone(memory_format=torch.channels_last))
    buf = poison.clone(memory_format=torch.channels_last)
    none, grads2 = hip.pose_heads_backward(feat, params, gos, need_feat_grad=False, grad_feat=buf)
    torch.cuda.synchronize()
    assert none is None and torch.equal(buf, poison)
    assert all(torch.equal(a, b) for x, y in zip(grads, grads2) for a, b in zip(x, y))
    assert not torch.equal(gfeat, poison)


@pytest.mark.parametrize("scale", [1e-6, 1e3])
def test_gradient_range(device, scale):
    case = _dyadic("ragged_13x19", go_scale=scale)
    feat, params, gos = _to(device, case)
    ref = R.reference(case.feat, case.params, case.grad_outs)
    gfeat, grads = hip.pose_heads_backward(feat, params, gos)
    _check_grads(gfeat, grads, ref, "scale %g" % scale)


def test_reproducible_bit_for_bit(device):
    case = _dyadic("dla_32")
    feat, params, gos = _to(device, case)
    runs = [hip.pose_heads_backward(feat, params, gos) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0])   # the header declares no atomics: grad_feat too
        assert all(torch.equal(a, b) for x, y in zip(r[1], runs[0][1]) for a, b in zip(x, y))


def test_chunk_boundary_inside_the_batch(device):
    """One 64 -> 256 head at 128 x 128 with a partial last chunk: equals the reference, and grad_feat of image b equals the
    B = 1 call on image b alone."""
    H = W = 128
    chunk = hip.pose_heads_chunk_images(64, H, W, 256)
    B = chunk + 1 if chunk >= 1 else 17
    assert hip.pose_heads_chunk_images(B, H, W, 256) == chunk < B
    case = R.dyadic_case(77, B, 64, 256, H, W, (3,))
    feat, params, gos = _to(device, case)
    ref = R.reference(case.feat, case.params, case.grad_outs)
    _check_forward(hip.pose_heads_forward(feat, params), ref, "chunked B=%d" % B)
    gfeat, grads = hip.pose_heads_backward(feat, params, gos)
    _check_grads(gfeat, grads, ref, "chunked B=%d" % B)
    for b in (0, chunk - 1, chunk):
        one, _ = hip.pose_heads_backward(feat[b:b + 1], params, [gos[0][b:b + 1]])
        assert torch.equal(one[0], gfeat[b]), b


@pytest.mark.parametrize("name", sorted(R.SHARED_CONV_CASES))
def test_heads_and_conv2d_backward_share_one_implementation(device, name):
    """The heads' 3x3 layer goes through conv_bwd.hip: with one class, grad_hidden is one rounded float32 product gated by an
    exactly known hidden value, so torch reproduces it bit for bit, and cp_conv2d_backward_nhwc on it must return the bits of
    grad_w0 and grad_feat (same kernels, same plan, same order)."""
    seed, *shape = R.SHARED_CONV_CASES[name]
    case = R.dyadic_case(seed, *shape)
    feat, params, gos = _to(device, case)
    w0, b0, w1, _ = case.params[0]
    h = torch.nn.functional.conv2d(case.feat, w0, b0, padding=1)   # exact (check_dyadic)
    gh = torch.where(h > 0, case.grad_outs[0] * w1.view(1, -1, 1, 1), torch.zeros(()))
    gfeat, grads = hip.pose_heads_backward(feat, params, gos)
    gx, gw, _ = hip.conv2d_backward(feat.permute(0, 2, 3, 1), params[0][0], gh.to(device).permute(0, 2, 3, 1).contiguous(),
                                    stride=1, pad=1, need_bias_grad=False)
    ref = R.reference(case.feat, case.params, case.grad_outs)["grads"][0][0]
    err, tol = float((grads[0][0].cpu().double() - ref).abs().max()), GRAD_TOL * float(ref.abs().max())
    print("%s: grad_w0 err %.3e (tol %.3e); differing elements: grad_w0 %d, grad_feat %d"
          % (name, err, tol, int((grads[0][0] != gw).sum()), int((gfeat.permute(0, 2, 3, 1) != gx).sum())))
    assert err <= tol   # the equality below cannot be met by two equally wrong results
    assert torch.equal(grads[0][0], gw)
    assert torch.equal(gfeat.permute(0, 2, 3, 1), gx)


def _model(arch, device, tracking=False):
    heads = synth.HEADS_POSE
    opt = None
    if tracking:
        from types import SimpleNamespace
        opt = SimpleNamespace(pre_img=True, pre_hm=True, pre_hm_hp=True, tracking_task=False)
    head_conv = 64 if arch.startswith("resdcn") else 256
    model = create_model(arch, heads, head_conv, opt).to(device)
    model.load_state_dict(synth.make_state_dict(arch, heads, tracking=tracking))
    return model, heads


@pytest.mark.parametrize("arch", ["dla_34", "resdcn_18"])
def test_realistic_case_with_ambiguous_unit_allowance(device, arch):
    model, heads = _model(arch, device)
    x = synth.frames(1, seed=3, h=256, w=256).to(device)
    feat = model.features(x)
    params = R.head_params(model.state_dict(), heads)
    B, _, H, W = feat.shape
    gos = R.gaussian_grad_outs(5, B, list(heads.values()), H, W)
    ref = R.reference(feat, params, gos)
    allow = R.allowance(feat, params, gos, ref["hidden"])
    print("%s: ambiguous share %.3e of the hidden units (cap %.0e)" % (arch, allow["share"], R.AMBIGUOUS_CAP))
    assert allow["share"] <= R.AMBIGUOUS_CAP
    dparams = [tuple(t.to(device) for t in p) for p in params]
    _check_forward(hip.pose_heads_forward(feat, dparams), ref, arch)
    gfeat, grads = hip.pose_heads_backward(feat, dparams, [g.to(device) for g in gos])
    _check_grads(gfeat, grads, ref, arch, allow)


@pytest.mark.parametrize("arch, tracking, tap", [("dla_34", False, "feat"), ("dla_34", True, "feat"),
                                                 ("resdcn_18", False, "deconv_layers.17")])
def test_model_features(device, arch, tracking, tap):
    model, heads = _model(arch, device, tracking)
    B, H, W = 2, 128, 128
    x = synth.frames(B, seed=9, h=H, w=W).to(device)
    pre = {}
    if tracking:
        g = torch.Generator().manual_seed(4)
        pre = dict(pre_img=synth.frames(B, seed=10, h=H, w=W).to(device), pre_hm=torch.rand(B, 1, H, W, generator=g).to(device),
                   pre_hm_hp=torch.rand(B, 8, H, W, generator=g).to(device))
    for prec in ("f32", "f16x3"):
        eng = model._engine()
        eng.set_precision(prec)
        _, tapped = eng.forward(x, tap=tap, **pre)
        tapped = tapped.clone()
        eng.profile(True)
        feat = model.features(x, **pre)
        torch.cuda.synchronize()
        eng.profile_read()
        roles = eng.profile_roles()
        eng.profile(False)
        assert roles and "head" not in roles and "head_final" not in roles, roles
        assert tuple(feat.shape) == (B, 64, H // 4, W // 4) and feat.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(feat, tapped), prec
        # the module on those features is the model's own heads
        mod = model.head_module().to(device)
        try:
            hip.set_default_precision(prec)
            with torch.no_grad():
                z = mod(feat)
                again = hip.pose_heads_forward(feat, [mod.head_params(h) for h in heads])
        finally:
            hip.set_default_precision("f32")
        want = model(x, **pre)[0]
        for (h, v), a in zip(z.items(), again):
            assert torch.equal(v, a), h   # no_grad: the forward kernel's values bit for bit
            err = float((v - want[h]).abs().max())
            assert err <= FWD_TOL * max(1.0, float(want[h].abs().max())), (prec, h, err)


def test_module_autograd(device):
    """One autograd node over all heads; grad_feat only when the feature map asks for it; heads outside the loss get zeros."""
    torch.manual_seed(0)
    mod = PoseHeads({"hm": 1, "wh": 2, "hps": 16}, 64, 64).to(device)
    case = R.dyadic_case(3, 2, 64, 64, 16, 16, (1, 2, 16))
    with torch.no_grad():
        for name, p in zip(mod.heads, case.params):
            for dst, src in zip(mod.head_params(name), p):
                dst.copy_(src)
    feat = case.feat.to(device)
    z = mod(feat)
    assert list(z) == ["hm", "wh", "hps"] and len({id(v.grad_fn) for v in z.values()}) == 1
    gos = [case.grad_outs[0].to(device), None, case.grad_outs[2].to(device)]
    (z["hm"] * gos[0]).sum().add((z["hps"] * gos[2]).sum()).backward()
    ref = R.reference(case.feat, case.params, [case.grad_outs[0], None, case.grad_outs[2]])
    grads = [tuple(p.grad for p in mod.head_params(n)) for n in mod.heads]
    _check_grads(None, grads, ref, "module")
    assert not any(bool(g.any()) for g in grads[1])
    f2 = feat.clone().requires_grad_(True)
    z2 = mod(f2)
    assert all(torch.equal(z2[k], z[k]) for k in z)
    (z2["hm"] * gos[0]).sum().add((z2["hps"] * gos[2]).sum()).backward()
    err = float((f2.grad.cpu().double() - ref["gfeat"]).abs().max())
    assert err <= GRAD_TOL * float(ref["gfeat"].abs().max())


def test_training_step_on_frozen_backbone(device):
    """The loop of INTEGRATION.md 'Training the heads': dla_34 from synth, B = 2, 256 x 256; one SGD step on the device against
    the same step on the CPU (block in float64, loss through tests/pose_loss_ref.py with the device's choice), then ten Adam
    steps on the same batch, load_heads, and the model runs the trained heads."""
    from centerpose_amd.pose_loss import ObjectPoseLoss
    from centerpose_amd.pose_targets import PoseTargets, pack_annotations
    from tests import pose_loss_cases as PLC
    from tests import pose_loss_ref as LR
    from tests import pose_target_cases as PC

    model, heads = _model("dla_34", device)
    B, res = 2, 64
    recs = []
    topt = None
    for seed in (21, 22):
        topt, anns, w, h, _ = PC.random_case(seed, "chair", n_obj=4, output_res=res, input_res=4 * res, center_3D=False,
                                             use_absolute_scale=False, hps_uncertainty=False, obj_scale_uncertainty=False)
        s = max(w, h) / res
        t = np.array([[1 / s, 0, res / 2 - w / 2 / s], [0, 1 / s, res / 2 - h / 2 / s]])
        recs.append(pack_annotations(anns, t, w, h, False, 0.0, topt))
    records = {k: torch.from_numpy(np.stack([r[k] for r in recs])) for k in ("pt_image", "pt_objects")}
    batch = PoseTargets(topt)(records)
    assert int(batch["reg_mask"].sum()) > 0
    lopt = PLC.make_opt({})
    crit = ObjectPoseLoss(lopt)
    images = synth.frames(B, seed=5, h=4 * res, w=4 * res).to(device)
    feat = model.features(images)
    mod = model.head_module().to(device)
    start = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
    lr = 1e-5   # the synthetic heads start far from these targets (loss in the hundreds, gradients in the thousands)

    optim = torch.optim.SGD(mod.parameters(), lr=lr)
    out = mod(feat)
    loss, stats, choice = crit([out], batch, "train")
    optim.zero_grad()
    loss.backward()
    dev_grads = {n: p.grad.detach().cpu().double() for n, p in mod.named_parameters()}
    optim.step()
    first = float(loss)

    # the same step on the CPU in float64
    params = [tuple(start["%s.%s" % (h, k)] for k in ("0.weight", "0.bias", "2.weight", "2.bias")) for h in heads]
    x = feat.detach().cpu().double()
    ps = [[t.double().requires_grad_(True) for t in p] for p in params]
    hidden, outs = [], {}
    for h, (w0, b0, w1, b1) in zip(heads, ps):
        hh = torch.nn.functional.conv2d(x, w0, b0, padding=1)
        hidden.append(hh.detach())
        outs[h] = torch.nn.functional.conv2d(torch.relu(hh), w1, b1)
    for v in outs.values():
        v.retain_grad()
    b64 = {k: (v.cpu().double() if v.dtype == torch.float32 else v.cpu()) for k, v in batch.items()}
    r = LR.object_pose_loss(lopt, [outs], b64, "train", choice=choice.cpu())
    r["loss"].backward()
    assert abs(first - float(r["loss"])) <= 1e-3 * abs(float(r["loss"])), (first, float(r["loss"]))
    gos = [outs[h].grad if outs[h].grad is not None else None for h in heads]
    allow = R.allowance(x, params, gos, hidden)
    print("training step: loss %.6f, ambiguous share %.3e" % (first, allow["share"]))
    assert allow["share"] <= R.AMBIGUOUS_CAP
    for i, h in enumerate(heads):
        for k, leaf in enumerate(("0.weight", "0.bias", "2.weight", "2.bias")):
            n = "%s.%s" % (h, leaf)
            gc, al = ps[i][k].grad, allow["grads"][i][k]
            gc = gc if gc is not None else torch.zeros_like(ps[i][k])
            scale = float(gc.abs().max())
            d = (dev_grads[n] - gc).abs()
            assert bool((d <= 1e-3 * scale + al).all()), (n, float(d.max()), scale)
            stepped = ps[i][k].detach() - lr * gc
            dp = (mod.state_dict()[n].cpu().double() - stepped).abs()
            assert bool((dp <= 1e-3 * lr * scale + lr * al + 1e-6).all()), (n, float(dp.max()))
    assert any(float(v.abs().max()) > 0 for v in dev_grads.values())

    # ten Adam steps on the same batch end below the first step's loss
    optim = torch.optim.Adam(mod.parameters(), 1e-3)
    last = None
    for _ in range(10):
        loss, _, _ = crit([mod(feat)], batch, "train")
        optim.zero_grad()
        loss.backward()
        optim.step()
        last = float(loss)
    print("training: first loss %.6f, after ten Adam steps %.6f" % (first, last))
    assert last < first
    model.load_heads(mod)
    with torch.no_grad():
        want = mod(feat)["hm"]
    got = model(images)[0]["hm"]
    assert float((got - want).abs().max()) <= FWD_TOL * max(1.0, float(want.abs().max()))
