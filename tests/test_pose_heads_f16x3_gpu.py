"""GPU tests of the PoseHeads backward's f16x3 mode (cp_pose_heads_backward_prec, hip.ops.pose_heads_backward_prec,
PoseHeads.backward_precision) against the float64 reference of tests/pose_heads_ref.py.  The inputs, their premises and the
tolerances are in tests/pose_heads_f16x3_cases.py; tests/test_pose_heads_f16x3_cpu.py asserts the premises for every case and
seed used here.  Each test that claims f16x3 ran first asserts the mask of its shape."""
import pytest
import torch

from centerpose_amd import hip, pose_heads
from centerpose_amd.pose_heads import PoseHeads
from tests import pose_heads_f16x3_cases as C
from tests import pose_heads_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["dla_32", "ragged_13x19", "classes_64"])
def test_f32_through_the_new_entry_is_the_old_call(device, name):
    case = C.cached_case("strict", name)
    feat, params, gos = C.to_device(device, case)
    old = hip.pose_heads_backward(feat, params, gos)
    new = hip.ops.pose_heads_backward_prec(feat, params, gos, precision="f32")
    assert len(C.flat(new)) == 1 + 4 * len(params) and C.bit_equal(old, new)
    C.assert_close(new, C.cached_reference("strict", name), name + " f32")
    old_nf = hip.pose_heads_backward(feat, params, gos, need_feat_grad=False)
    new_nf = hip.ops.pose_heads_backward_prec(feat, params, gos, need_feat_grad=False, precision="f32")
    assert old_nf[0] is None and new_nf[0] is None and C.bit_equal(old_nf, new_nf)


@pytest.mark.parametrize("name", sorted(C.STRICT_SHAPES))
def test_strict_dyadic(device, name):
    """feat and w0 have no lo part and the hidden values are exact: the gate is the reference's, every gradient within GRAD_TOL."""
    case = C.cached_case("strict", name)
    C.assert_f16x3(case)
    got = C.device_backward(device, case)
    assert got[0].is_contiguous(memory_format=torch.channels_last)
    C.assert_close(got, C.cached_reference("strict", name), name)


@pytest.mark.parametrize("kind", C.TWO_LEVEL_KINDS)
@pytest.mark.parametrize("name", sorted(C.TWO_LEVEL_SHAPES))
def test_exact_two_level(device, name, kind):
    """grad_w0, grad_b0, grad_b1 and grad_feat EQUAL the float64 reference: a dropped hi*lo or lo*hi term cannot."""
    case = C.cached_case("two_" + kind, name)
    C.assert_f16x3(case)
    got = C.device_backward(device, case)
    C.assert_close(got, C.cached_reference("two_" + kind, name), "%s %s" % (name, kind),
                   exact=("grad_feat", "grad_w0", "grad_b0", "grad_b1"))


def test_not_a_float32_fallback(device):
    """On Gaussian inputs both modes are within tolerance and their matrix products differ in the last bits."""
    case = C.cached_case("gauss", "dla_32")
    C.assert_f16x3(case)
    ref = C.cached_reference("gauss", "dla_32")
    allow = C.f16x3_allowance(case.feat, case.params, case.grad_outs, ref["hidden"])
    assert allow["share"] <= R.AMBIGUOUS_CAP
    a = C.device_backward(device, case, precision="f32")
    b = C.device_backward(device, case, precision="f16x3")
    C.assert_close(a, ref, "gauss f32", allow)
    C.assert_close(b, ref, "gauss f16x3", allow)
    assert not torch.equal(a[0], b[0])
    for ga, gb in zip(a[1], b[1]):
        assert not torch.equal(ga[0], gb[0])        # grad_w0
        assert torch.equal(ga[3], gb[3])            # grad_b1: the same float32 code in either mode


@pytest.mark.parametrize("exp", [-20, 10])
def test_power_of_two_equivariance(device, exp):
    """grad_out times 2^exp: every gradient of the f16x3 mode, rescaled, equals the unscaled run bit for bit."""
    case = C.cached_case("gauss", "ragged_13x19")
    C.assert_f16x3(case)
    base = C.device_backward(device, case)
    scaled = C.device_backward(device, case, grad_outs=[g * 2.0 ** exp for g in case.grad_outs])
    for (name, x), (_, y) in zip(C.flat(base), C.flat(scaled)):
        assert torch.equal(x, y * 2.0 ** -exp), (name, exp)
    ref = C.cached_reference("gauss", "ragged_13x19")
    C.assert_close(base, ref, "gauss ragged", C.f16x3_allowance(case.feat, case.params, case.grad_outs, ref["hidden"]))


@pytest.mark.parametrize("arch", sorted(C.REALISTIC))
def test_realistic_case_with_widened_allowance(device, arch):
    case = C.cached_case("realistic", arch)
    C.assert_f16x3(case)
    ref = C.cached_reference("realistic", arch)
    allow = C.f16x3_allowance(case.feat, case.params, case.grad_outs, ref["hidden"])
    print("%s: ambiguous share %.3e of the hidden units (cap %.0e)" % (arch, allow["share"], R.AMBIGUOUS_CAP))
    assert allow["share"] <= R.AMBIGUOUS_CAP
    C.assert_close(C.device_backward(device, case), ref, arch, allow)


def test_heads_without_a_gradient(device):
    case = C.cached_case("strict", "resdcn")
    C.assert_f16x3(case)
    for drop in ((1, 4), (0, 2, 3, 5, 6), tuple(range(7))):
        gos = [None if i in drop else g for i, g in enumerate(case.grad_outs)]
        got = C.device_backward(device, case, grad_outs=gos)
        for i in drop:
            assert all(not bool(g.any()) for g in got[1][i]), (drop, i)
        if len(drop) == 7:
            assert not bool(got[0].any())
            continue
        C.assert_close(got, R.reference(case.feat, case.params, gos), "dropped %s" % (drop,))


def test_frozen_backbone_leaves_grad_feat_alone(device):
    case = C.cached_case("strict", "resdcn")
    C.assert_f16x3(case)
    feat = C.to_device(device, case)[0]
    poison = torch.full_like(feat, 1234.5)
    full = C.device_backward(device, case, grad_feat=poison.clone(memory_format=torch.channels_last))
    buf = poison.clone(memory_format=torch.channels_last)
    frozen = C.device_backward(device, case, need_feat_grad=False, grad_feat=buf)
    torch.cuda.synchronize()
    assert frozen[0] is None and torch.equal(buf, poison) and not torch.equal(full[0], poison)
    assert C.bit_equal((None, full[1]), frozen)


def test_reproducible_bit_for_bit(device):
    case = C.cached_case("gauss", "dla_32")
    C.assert_f16x3(case)
    first = C.device_backward(device, case)
    assert C.bit_equal(first, C.device_backward(device, case))


def test_chunk_boundary_inside_the_batch(device):
    """One 64 -> 256 head at 128 x 128 with a partial last chunk (the float32 test's shape): grad_w0, grad_w1 and grad_b0 continue
    across the chunks, each chunk with its own grad_hidden scale, and every gradient equals the reference."""
    H = W = 128
    chunk = hip.pose_heads_chunk_images(64, H, W, 256)
    B = chunk + 1 if chunk >= 1 else 17
    assert hip.pose_heads_chunk_images(B, H, W, 256) == chunk < B
    case = R.dyadic_case(77, B, 64, 256, H, W, (3,))
    C.assert_f16x3(case)
    got = C.device_backward(device, case)
    C.assert_close(got, R.reference(case.feat, case.params, case.grad_outs), "chunked B=%d" % B)


def test_module_autograd_and_switch(device):
    """PoseHeads(backward_precision="f16x3") under autograd, and set_backward_precision on the built module between calls."""
    torch.manual_seed(0)
    mod = PoseHeads({"hm": 1, "wh": 2, "hps": 16}, 64, 64, backward_precision="f16x3").to(device)
    case = C.cached_case("gauss", "resdcn")
    case = type(case)(feat=case.feat, params=case.params[:3], grad_outs=case.grad_outs[:3])
    C.assert_f16x3(case)
    with torch.no_grad():
        for name, p in zip(mod.heads, case.params):
            for dst, src in zip(mod.head_params(name), p):
                dst.copy_(src)
    gos = [case.grad_outs[0], None, case.grad_outs[2]]
    ref = R.reference(case.feat, case.params, gos)
    allow = C.f16x3_allowance(case.feat, case.params, gos, ref["hidden"])

    def step():
        mod.zero_grad(set_to_none=True)
        f = case.feat.to(device).requires_grad_(True)
        z = mod(f)
        assert len({id(v.grad_fn) for v in z.values()}) == 1
        (z["hm"] * gos[0].to(device)).sum().add((z["hps"] * gos[2].to(device)).sum()).backward()
        return f.grad, [tuple(p.grad.clone() for p in mod.head_params(n)) for n in mod.heads]

    a = step()
    C.assert_close(a, ref, "module f16x3", allow)
    assert not any(bool(g.any()) for g in a[1][1])
    direct = C.device_backward(device, case, grad_outs=gos)
    assert C.bit_equal(a, direct)
    assert pose_heads.set_backward_precision(mod, "f32") == 1
    b = step()
    C.assert_close(b, ref, "module f32", allow)
    assert C.bit_equal(b, C.device_backward(device, case, precision="f32", grad_outs=gos)) and not torch.equal(a[0], b[0])
    assert pose_heads.set_backward_precision(mod, "f16x3") == 1
    assert C.bit_equal(step(), a)
