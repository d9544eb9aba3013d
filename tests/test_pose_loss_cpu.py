"""CPU tests of the device ObjectPoseLoss (no GPU): the float64 restatement tests/pose_loss_ref.py against the reference's
float32 goldens (and against the reference's live ObjectPoseLoss where that tree is present), the host build of
pose_loss_common.h against the restatement element by element, the refusals at construction, and the C ABI's
argument checks with no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from centerpose_amd import hip
from tests import pose_loss_cases as PC
from tests import pose_loss_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(REPO, "tests", "golden", "pose_loss_ref.npz")


def _f64(outputs, batch, grad=False):
    outs = [{k: torch.from_numpy(v).double().requires_grad_(grad) for k, v in o.items()} for o in outputs]
    bt = {k: (torch.from_numpy(v).double() if v.dtype == np.float32 else torch.from_numpy(v)) for k, v in batch.items()}
    return outs, bt


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-6))) if a.size else 0.0


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_restatement_equals_goldens(gold, name):
    opt, phase, outputs, batch = PC.case(name)
    outs, bt = _f64(outputs, batch, grad=True)
    r = R.object_pose_loss(opt, outs, bt, phase)
    r["loss"].backward()
    assert np.array_equal(r["choice"].numpy(), gold[name + "/choice"])
    assert _rel(float(r["loss"]), gold[name + "/loss"]) < 1e-5
    assert _rel([float(r["stats"][k]) for k in R.STATS], gold[name + "/stats"]) < 1e-5
    for t in R.on_terms(opt):
        assert _rel(r["terms"][t].detach().numpy(), gold[name + "/term_" + t]) < 1e-5, t
    for s, o in enumerate(outs):
        for h, v in o.items():
            key = "%s/grad%d_%s" % (name, s, h)
            if key not in gold.files:
                assert v.grad is None or not v.grad.abs().max(), key
                continue
            g = gold[key]
            assert np.max(np.abs(v.grad.numpy() - g)) <= 1e-5 * max(np.abs(g).max(), 1e-30), key


def test_restatement_equals_live_reference():
    Ref = PC.import_reference_loss()
    if Ref is None:
        pytest.skip("the reference tree is not present")
    for name in sorted(PC.CASES):
        opt, phase, outputs, batch = PC.case(name)
        outs32 = [{k: torch.from_numpy(v) * 1 for k, v in o.items()} for o in outputs]
        loss, stats, choice = Ref(opt)(outs32, {k: torch.from_numpy(v) for k, v in batch.items()}, phase)
        outs, bt = _f64(outputs, batch)
        r = R.object_pose_loss(opt, outs, bt, phase)
        assert torch.equal(choice, r["choice"]), name
        assert _rel([float(stats[k]) for k in R.STATS], [float(r["stats"][k]) for k in R.STATS]) < 1e-5, name
        # the reference's side effect: outputs[s]['hm'] holds clamp(sigmoid)
        assert torch.allclose(outs32[0]["hm"].double(), r["maps"][0]["hm"], atol=1e-7), name


def _host():
    out = os.path.join(REPO, "tests", "_build", "libcp_pose_loss_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(REPO, "tests", "native", "pose_loss_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
    return ctypes.CDLL(out)


def _dp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_host_focal_formulas_match_restatement():
    L = _host()
    rng = np.random.default_rng(0)
    n = 4000
    x = np.concatenate([rng.normal(0, 4, n - 6), [20.0, -20.0, 9.21024, -9.21024, 0.0, 30.0]])
    g = np.where(rng.random(n) < 0.2, 1.0, rng.uniform(0, 1, n) * (rng.random(n) < 0.5))
    outs = [np.zeros(n) for _ in range(4)]
    L.pl_host_focal(0, n, _dp(x), _dp(g), *[_dp(o) for o in outs])
    p, pos, neg, dl = outs
    xt = torch.from_numpy(x).requires_grad_()
    gt = torch.from_numpy(g)
    q = R.clamp_sigmoid(xt)
    val = torch.log(q) * (1 - q) ** 2 * (gt == 1) + torch.log(1 - q) * q ** 2 * (1 - gt) ** 4 * (gt < 1)
    val.sum().backward()
    assert np.allclose(p, q.detach().numpy(), rtol=1e-14, atol=0)
    ref_pos = (torch.log(q) * (1 - q) ** 2).detach().numpy()
    ref_neg = (torch.log(1 - q) * q ** 2 * (1 - gt) ** 4).detach().numpy()
    assert np.allclose(pos, ref_pos, rtol=1e-12, atol=1e-300)
    assert np.allclose(neg, ref_neg, rtol=1e-12, atol=1e-300)
    assert np.allclose(dl, xt.grad.numpy(), rtol=1e-10, atol=1e-300)
    # float32 build: the device's arithmetic, within float32 rounding of the float64 values
    L.pl_host_focal(1, n, _dp(x), _dp(g), *[_dp(o) for o in outs])
    assert np.allclose(outs[1], ref_pos, rtol=1e-5, atol=1e-6)
    assert np.allclose(outs[3], xt.grad.numpy(), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("mode,kind", [(0, "l1"), (1, "resid"), (2, "rel"), (3, "kld_key"), (4, "kld_scale")])
def test_host_reg_formulas_match_restatement(mode, kind):
    L = _host()
    rng = np.random.default_rng(mode)
    n = 3000
    t = rng.normal(0, 1, n)
    t[::17] = 0.0
    p = rng.normal(0, 1, n)
    p[::23] = t[::23]  # abs at 0: gradient 0
    m = (rng.random(n) < 0.7).astype(np.float64)
    u = rng.normal(0, 0.5, n)
    ref, kl = 1.3, float(np.float32(0.1))
    val, dp, du = np.zeros(n), np.zeros(n), np.zeros(n)
    L.pl_host_reg(0, mode, n, _dp(t), _dp(p), _dp(m), _dp(u), ctypes.c_double(ref), ctypes.c_double(kl), _dp(val), _dp(dp),
                  _dp(du))
    # the restatement's term on a [1,1,n,1] layout: one image, one variant, n entries of one channel
    head = torch.from_numpy(p).reshape(1, 1, 1, n).requires_grad_()
    unc = torch.from_numpy(u).reshape(1, 1, 1, n).requires_grad_()
    ind = torch.arange(n).reshape(1, 1, n)
    mt = torch.from_numpy(m).reshape(1, 1, n, 1)
    tt = torch.from_numpy(t).reshape(1, 1, n, 1)
    r = R.reg(head, ind, tt, mt, kind, unc=unc, ref=[ref], kl=kl)
    den = m.sum() + (1e-6 if mode >= 3 else 1e-4)
    assert abs(val.sum() / den - float(r)) <= 1e-12 * abs(float(r))
    r.backward()
    g = head.grad.numpy().reshape(-1)  # 1 - exp(-a/kl) cancels at small a: compare to 1e-12 of the largest value
    assert np.allclose(dp / den, g, rtol=1e-10, atol=1e-12 * np.abs(g).max())
    if mode >= 3:
        g = unc.grad.numpy().reshape(-1)
        assert np.allclose(du / den, g, rtol=1e-10, atol=1e-12 * np.abs(g).max())
    else:
        assert not du.any()


@pytest.mark.parametrize("field,value", [("mse_loss", True), ("dense_hp", True), ("reg_loss", "sl1"),
                                         ("eval_oracle_hm", True), ("eval_oracle_hmhp", True), ("eval_oracle_kps", True),
                                         ("eval_oracle_hp_offset", True)])
def test_refused_options_raise_at_construction(field, value):
    from centerpose_amd.pose_loss import ObjectPoseLoss

    ObjectPoseLoss(PC.make_opt({}))
    with pytest.raises(NotImplementedError):
        ObjectPoseLoss(PC.make_opt({field: value}))


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def test_pose_loss_symbols_exported_and_declared(built):
    names = ("cp_pose_loss_workspace_bytes", "cp_pose_loss_forward", "cp_pose_loss_backward")
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    for n in names:
        assert hasattr(built, n) and n in hip.exported_symbols() and (n + "(") in header


def _desc(B=2, S=4, K=10, H=32, W=32, J=8, ns=1):
    d = hip.PoseLossDesc()
    d.B, d.S, d.K, d.H, d.W, d.num_classes, d.num_joints, d.num_stacks = B, S, K, H, W, 1, J, ns
    d.terms = 1 << 0 | 1 << 3
    fake = 256  # never dereferenced: every call here is refused before any launch
    d.gt_hm, d.ind, d.gt_hps, d.hps_mask = fake, fake, fake, fake
    for st in range(ns):
        d.head[st][0], d.head[st][2], d.clamped[st][0] = fake, fake, fake
    return d


def test_null_and_oversized_arguments_are_refused_without_a_device(built):
    L = built
    ok = _desc()
    assert L.cp_pose_loss_workspace_bytes(ctypes.byref(ok)) > 0
    assert L.cp_pose_loss_workspace_bytes(None) == 0
    assert L.cp_pose_loss_forward(None, None, None, None, None, None, None, 0) == -1
    cases = []
    for f, v in (("S", 65), ("S", 0), ("K", 257), ("num_stacks", 5), ("num_joints", 33), ("H", 33), ("B", 0)):
        d = _desc()
        setattr(d, f, v)
        if f == "H":
            d.W = 33  # H*W not a multiple of 4
        cases.append(d)
    big = _desc(B=64, S=64, H=512, W=512)  # gt hm of 2^34 elements
    cases.append(big)
    nul = _desc()
    nul.gt_hm = None
    cases.append(nul)
    nohead = _desc()
    nohead.head[0][2] = None
    cases.append(nohead)
    for field in ("gt_hm", "head", "clamped"):  # the float4 heat-map pointers must be 16-byte aligned
        mis = _desc()
        if field == "gt_hm":
            mis.gt_hm = 256 + 4
        else:
            getattr(mis, field)[0][0] = 256 + 8
        cases.append(mis)
    # 28000^2 pixels: the 2-channel heads fit below 2^31 elements, the 3-channel scale head does not
    scale3 = _desc(B=1, S=1, H=28000, W=28000, J=1)
    assert L.cp_pose_loss_workspace_bytes(ctypes.byref(scale3)) > 0
    scale3.terms |= 1 << 6
    scale3.reg_mask, scale3.gt_scale, scale3.head[0][6] = 256, 256, 256
    cases.append(scale3)
    for d in cases:
        assert L.cp_pose_loss_workspace_bytes(ctypes.byref(d)) == 0
        assert L.cp_pose_loss_forward(None, ctypes.byref(d), 256, 256, 256, None, 256, 1 << 30) == -1
        assert L.cp_pose_loss_backward(None, ctypes.byref(d), 256, None, (ctypes.c_void_p * 44)(), 256, 1 << 30) == -1
    # an accepted descriptor with a short workspace or no gradients
    n = L.cp_pose_loss_workspace_bytes(ctypes.byref(ok))
    assert L.cp_pose_loss_forward(None, ctypes.byref(ok), 256, 256, 256, None, 256, n - 1) == -1
    assert b"workspace" in L.cp_last_error()
    assert L.cp_pose_loss_backward(None, ctypes.byref(ok), 256, None, (ctypes.c_void_p * 44)(), 256, n) == -1
    assert b"gradient" in L.cp_last_error()
    assert L.cp_pose_loss_backward(None, ctypes.byref(ok), 256, None, None, 256, n) == -1


def test_binding_refuses_cpu_tensors():
    from centerpose_amd.pose_loss import ObjectPoseLoss

    opt, phase, outputs, batch = PC.case("s1")
    outs = [{k: torch.from_numpy(v) for k, v in o.items()} for o in outputs]
    with pytest.raises((ValueError, RuntimeError)):
        ObjectPoseLoss(opt)(outs, {k: torch.from_numpy(v) for k, v in batch.items()}, phase)
