"""CPU tests (no GPU) of the prediction-head block: the C ABI's declarations, workspace arithmetic and refusals
(cp_pose_heads_*, cp_model_features), the PoseHeads module's parameter names and initial values, the HipPoseNet round trip,
and the float64 reference helper (tests/pose_heads_ref.py) against a hand-written backward."""
import ctypes
import json
import os
import re

import pytest
import torch

import __graft_entry__ as ge
from centerpose_amd import hip, synth
from centerpose_amd.lib.models.model import create_model
from tests import pose_heads_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_pose_heads_chunk_images", "cp_pose_heads_forward_workspace_bytes", "cp_pose_heads_forward",
       "cp_pose_heads_backward_workspace_bytes", "cp_pose_heads_backward", "cp_model_features")
DLA = (ctypes.c_int * 7)(*R.DLA_CLASSES)


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_symbols_declared_exported_and_listed(built):
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and hasattr(built, name) and name in hip.exported_symbols(), name
    assert int(re.search(r"#define\s+CP_ABI_VERSION\s+(\d+)", header).group(1)) == 7 == built.cp_abi_version()
    assert built.cp_num_kernel_variants() == 46 and built.cp_num_roles() == 10
    assert int(re.search(r"#define\s+CP_NUM_KERNEL_VARIANTS\s+(\d+)", header).group(1)) == 46
    assert int(re.search(r"#define\s+CP_NUM_ROLES\s+(\d+)", header).group(1)) == 10


def test_workspace_queries_are_host_arithmetic(built):
    fq, bq = built.cp_pose_heads_forward_workspace_bytes, built.cp_pose_heads_backward_workspace_bytes
    for B, H, W, Cin, hid, cls in ((2, 128, 128, 64, 256, DLA), (1, 32, 32, 64, 64, DLA), (1, 24, 24, 128, 96, _ints(3, 5)),
                                   (2, 13, 19, 64, 64, _ints(2, 16)), (3, 1, 1, 32, 32, _ints(1, 4)), (1, 130, 66, 64, 64, _ints(8))):
        assert fq(B, H, W, Cin, hid, len(cls), cls) > 0 and bq(B, H, W, Cin, hid, len(cls), cls) > 0
    # the headline shape: below twice ONE head's hidden map at that batch (nothing like all seven is ever materialised)
    one_hidden = 64 * 128 * 128 * 256 * 4
    assert 0 < bq(64, 128, 128, 64, 256, 7, DLA) < 2 * one_hidden
    assert 0 < fq(64, 128, 128, 64, 256, 7, DLA) < 2 * one_hidden
    # ... in fact a chunk of at most 256 MiB of it
    chunk = built.cp_pose_heads_chunk_images(64, 128, 128, 256)
    assert 1 <= chunk and chunk * 128 * 128 * 256 * 4 <= 256 << 20
    assert bq(64, 128, 128, 64, 256, 7, DLA) < 512 << 20
    assert built.cp_pose_heads_chunk_images(64, 1024, 1024, 256) == 1   # one image is the floor
    sizes = [bq(B, 128, 128, 64, 256, 7, DLA) for B in (1, 2, 8, 16, 17, 32, 64)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[3]
    sizes = [fq(B, 128, 128, 64, 256, 7, DLA) for B in (1, 2, 8, 16, 17, 32, 64)]
    assert sizes == sorted(sizes)


def test_refusals_without_a_device(built):
    fq, bq = built.cp_pose_heads_forward_workspace_bytes, built.cp_pose_heads_backward_workspace_bytes

    def refused(q, args, text):
        assert q(*args) == 0
        assert text in built.cp_last_error(), (args[:6], built.cp_last_error())

    for q in (fq, bq):
        refused(q, (1, 8, 8, 48, 64, 1, _ints(2)), b"Cin must be")
        refused(q, (1, 8, 8, 0, 64, 1, _ints(2)), b"Cin must be")
        refused(q, (1, 8, 8, 64, 100, 1, _ints(2)), b"hidden width must be")
        refused(q, (1, 8, 8, 64, 64, 1, _ints(0)), b"classes must be in 1..64")
        refused(q, (1, 8, 8, 64, 64, 2, _ints(3, 65)), b"classes must be in 1..64")
        refused(q, (1, 8, 8, 64, 64, 0, _ints(1)), b"at least one head")
        refused(q, (0, 8, 8, 64, 64, 1, _ints(1)), b"at least 1")
        refused(q, (1, 0, 8, 64, 64, 1, _ints(1)), b"at least 1")
        refused(q, (64, 1024, 1024, 64, 64, 1, _ints(1)), b"2^31 elements")     # feat: 2^32 elements
        refused(q, (1, 4096, 4096, 64, 256, 1, _ints(1)), b"2^31 elements")     # one image's hidden map: 2^32
    # the calls themselves: refused before any launch (no device is touched; the pointers are never dereferenced)
    n = 2
    cls = _ints(1, 3)
    fake = (ctypes.c_void_p * n)(0x1000, 0x1000)
    null = (ctypes.c_void_p * n)(0, 0)
    p = ctypes.c_void_p(0x1000)
    shape = (2, 16, 16, 64, 64)
    need_f, need_b = fq(*shape, n, cls), bq(*shape, n, cls)
    fwd = lambda feat, ws, nbytes, c=cls, sh=shape: built.cp_pose_heads_forward(
        None, feat, n, fake, fake, fake, fake, c, fake, *sh, ws, nbytes)
    bwd = lambda feat, ws, nbytes, go=fake, g=fake, c=cls, sh=shape: built.cp_pose_heads_backward(
        None, feat, n, fake, fake, fake, fake, c, go, g, g, g, g, None, *sh, ws, nbytes)
    assert fwd(None, p, need_f) == -1 and b"null argument" in built.cp_last_error()
    assert bwd(None, p, need_b) == -1 and b"null argument" in built.cp_last_error()
    assert bwd(p, p, need_b, g=null) == -1 and b"null argument" in built.cp_last_error()
    assert fwd(p, None, need_f) == -1 and b"null argument" in built.cp_last_error()
    assert fwd(p, p, need_f - 1) == -1 and b"workspace too small" in built.cp_last_error()
    assert bwd(p, p, need_b - 1) == -1 and b"workspace too small" in built.cp_last_error()
    assert bwd(p, p, need_b, sh=(2, 16, 16, 40, 64)) == -1 and b"Cin must be" in built.cp_last_error()
    assert fwd(p, p, need_f, sh=(2, 16, 16, 64, 72)) == -1 and b"hidden width" in built.cp_last_error()
    assert bwd(p, p, need_b, c=_ints(1, 65)) == -1 and b"classes must be" in built.cp_last_error()
    # cp_model_features: a NULL model / buffer, and the architectures without a plain head block
    assert built.cp_model_features(None, None, 1, 128, 128, p, None, None, None, p, p, 1 << 20) == -1
    names = (ctypes.c_char_p * 1)(b"hm")
    one = _ints(1)
    for arch, text in ((b"dlav1_34", b"ConvGRU"), (b"hourglass", b"two stacks")):
        h = ctypes.c_void_p()
        assert built.cp_model_create(arch, 0, 1, names, one, 256, ctypes.byref(h)) == 0
        assert built.cp_model_features(h, None, 1, 128, 128, p, None, None, None, p, p, 1 << 20) == -4   # CP_ERR_STATE
        assert text in built.cp_last_error(), built.cp_last_error()
        built.cp_model_destroy(h)


def test_no_cpu_path(built):
    case = R.dyadic_case(1, 1, 32, 32, 4, 4, (2,))
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.pose_heads_forward(case.feat, case.params)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.pose_heads_backward(case.feat, case.params, case.grad_outs)


@pytest.mark.parametrize("arch, keys_file, head_conv", [("dla_34", "state_dict_keys.json", 256),
                                                        ("resdcn_18", "state_dict_keys_resdcn.json", 64)])
def test_pose_heads_parameter_names_and_initial_values(arch, keys_file, head_conv):
    from centerpose_amd.pose_heads import PoseHeads

    gold = json.load(open(os.path.join(REPO, "tests", "golden", keys_file)))
    gold = gold["dla" if arch == "dla_34" else arch]
    keys = list(gold) if isinstance(gold, dict) else [k for k, _ in gold]
    heads = synth.HEADS_POSE
    want = [k for k in keys if k.split(".")[0] in heads]
    torch.manual_seed(0)
    mod = PoseHeads(heads, 64, head_conv)
    sd = mod.state_dict()
    assert want and sorted(sd) == sorted(want)
    assert [n for n, _ in mod.named_parameters()] == list(sd)
    for h, c in heads.items():
        assert tuple(sd[h + ".0.weight"].shape) == (head_conv, 64, 3, 3) and tuple(sd[h + ".2.weight"].shape) == (c, head_conv, 1, 1)
        assert not sd[h + ".0.bias"].any() and float(sd[h + ".0.weight"].abs().max()) > 0
        assert torch.all(sd[h + ".2.bias"] == (-2.19 if "hm" in h else 0.0)), h
    # a reference checkpoint (backbone keys included) loads with strict=False and only the backbone keys are unexpected
    full = synth.make_state_dict(arch, heads, head_conv=head_conv)
    res = mod.load_state_dict(full, strict=False)
    assert not res.missing_keys and all(k.split(".")[0] not in heads for k in res.unexpected_keys)
    assert torch.equal(mod.state_dict()["hps.2.weight"], full["hps.2.weight"])
    for bad in (dict(in_channels=48), dict(head_conv=100), dict(head_conv=0)):
        with pytest.raises(NotImplementedError):
            PoseHeads(heads, **{**dict(in_channels=64, head_conv=256), **bad})
    with pytest.raises(NotImplementedError):
        PoseHeads({"hm": 65}, 64, 64)


def test_hipposenet_round_trip_and_refusals():
    heads = synth.HEADS_POSE
    model = create_model("dla_34", heads, 256, None)
    model.load_state_dict(synth.make_state_dict("dla_34", heads))
    before = {k: v.clone() for k, v in model.state_dict().items()}
    mod = model.head_module()
    for k, v in mod.state_dict().items():
        assert torch.equal(v, before[k]), k
    model._hip = object()   # stands for a cached engine
    model.load_heads(mod)
    assert model._hip is None
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    # trained values travel back, the backbone stays as it was
    with torch.no_grad():
        mod.hm.__getattr__("2").bias.add_(1.0)
    model.load_heads(mod)
    assert torch.equal(model.state_dict()["hm.2.bias"], before["hm.2.bias"] + 1.0)
    assert torch.equal(model.state_dict()["base.level2.tree1.conv1.weight"], before["base.level2.tree1.conv1.weight"])
    with pytest.raises(NotImplementedError, match="head_module"):
        model.train()
    assert model.train(False) is model
    with pytest.raises(RuntimeError, match="does not match"):
        from centerpose_amd.pose_heads import PoseHeads
        model.load_heads(PoseHeads({"hm": 2}, 64, 256))
    for arch in ("dlav1_34", "hourglass"):
        other = create_model(arch, heads, 256, None)
        with pytest.raises(NotImplementedError):
            other.head_module()
        with pytest.raises(NotImplementedError):
            other.features(torch.zeros(1, 3, 128, 128))
    res = create_model("resdcn_18", heads, 64, None)
    assert sorted(res.head_module().state_dict()) == sorted(k for k in res.state_dict() if k.split(".")[0] in heads)
    with pytest.raises(RuntimeError, match="HIP device"):
        model.features(torch.zeros(1, 3, 128, 128))


def test_reference_helper_against_hand_written_backward():
    for seed, (B, Cin, hid, H, W, classes), drop in ((1, (2, 32, 32, 7, 9, (3, 1, 5)), None), (2, (1, 64, 32, 5, 5, (2, 4)), 1)):
        g = torch.Generator().manual_seed(seed)
        feat = torch.randn(B, Cin, H, W, generator=g)
        params = [(torch.randn(hid, Cin, 3, 3, generator=g) * 0.1, torch.randn(hid, generator=g) * 0.1,
                   torch.randn(c, hid, 1, 1, generator=g), torch.randn(c, generator=g)) for c in classes]
        gos = R.gaussian_grad_outs(seed, B, classes, H, W)
        if drop is not None:
            gos[drop] = None
        a, m = R.reference(feat, params, gos), R.manual_backward64(feat, params, gos)
        assert float((a["gfeat"] - m["gfeat"]).abs().max()) <= 1e-12 * float(a["gfeat"].abs().max())
        for i, (ga, gm) in enumerate(zip(a["grads"], m["grads"])):
            for x, y in zip(ga, gm):
                assert x.shape == y.shape and float((x - y).abs().max()) <= 1e-12 * max(float(x.abs().max()), 1e-300), i
            if gos[i] is None:
                assert not any(bool(x.any()) for x in ga)
        outs, hid64 = R.forward64(feat, params)
        assert all(torch.equal(o, r) for o, r in zip(outs, a["outs"]))
        # the allowance is zero without ambiguous units and bounds the effect of flipping one
        al = R.allowance(feat, params, gos, hid64)
        assert 0 <= al["share"] <= 1
        h = hid64[0]
        idx = h.abs().flatten().argmin()
        flipped = h.flatten().clone()
        scale = float(h.abs().max())
        flipped[idx] = 1e-6 * scale
        al = R.allowance(feat, params, gos, [flipped.reshape(h.shape)] + hid64[1:])
        assert al["share"] > 0 and float(al["gfeat"].max()) > 0 and float(al["grads"][0][0].max()) > 0


@pytest.mark.parametrize("name", sorted(R.DYADIC_SHAPES))
def test_dyadic_generator_holds_for_every_gpu_shape(name):
    B, Cin, hid, H, W, classes = R.DYADIC_SHAPES[name]
    if name == "dla_128":
        B, classes = 1, classes[:2]   # the same generator and shape per image and head; the full case runs in the GPU test
    case = R.dyadic_case(sum(map(ord, name)), B, Cin, hid, H, W, classes)   # asserts inside
    assert len(case.params) == len(classes) and case.feat.shape == (B, Cin, H, W)
    smallest = min(float(torch.nn.functional.conv2d(case.feat, w0, b0, padding=1).abs().min()) for w0, b0, _, _ in case.params)
    assert smallest >= 1 / 32


@pytest.mark.parametrize("name", sorted(R.SHARED_CONV_CASES))
def test_dyadic_generator_holds_for_the_shared_conv_cases(name):
    seed, B, Cin, hid, H, W, classes = R.SHARED_CONV_CASES[name]
    case = R.dyadic_case(seed, B, Cin, hid, H, W, classes)   # asserts inside
    assert classes == (1,) and len(case.params) == 1 and case.feat.shape == (B, Cin, H, W)
