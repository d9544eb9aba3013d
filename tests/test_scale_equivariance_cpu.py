"""The two transforms of tests/scale_gauge_ref.py on the oracle, bit for bit: what tests/test_scale_equivariance_gpu.py
takes for granted when it compares the engine of a transformed model with the cached reference of the base model.  The
base passes are layer_parity_ref.reference's; this module adds only the transformed ones."""
import pytest
import torch

from tests import layer_parity_ref as R
from tests import scale_gauge_ref as G

ALPHAS = (2.0 ** 14, 2.0 ** -14)
T = 12
F32_KEYS = ("dla_34-2x96x160", "dlav1_34-1x128x128", "hourglass-1x128x256", "resdcn_18-2x96x160")  # one per graph
PASSES = [(key, torch.float64) for key in R.CASES] + [(key, torch.float32) for key in F32_KEYS]
IDS = ["%s-%s" % (k, str(d).split(".")[1]) for k, d in PASSES]


def _base(key, dtype):
    ref = R.reference(key)
    return ref.f64 if dtype == torch.float64 else ref.f32


def _transformed(key, dtype, sd, x, kw):
    taps, z = R.oracle(key, dtype, sd=sd, x=x, kw=kw)
    got = dict(taps)
    got.update(("head:" + h, v) for h, v in z.items())
    return got


@pytest.mark.parametrize("key", list(R.CASES))
def test_transforms_touch_the_intended_keys(key):
    sd = R.state_dict(key)
    arch = R.CASES[key]["arch"]
    a = ALPHAS[0]
    up, down = G.homogeneous_keys(sd)
    assert up and all(k.endswith((".bias", ".running_mean")) and "conv_offset_mask" not in k for k in up)
    assert all(k.endswith("conv_offset_mask.weight") for k in down)
    n_dcn = sum(k.endswith("conv_offset_mask.bias") for k in sd)
    assert len(down) == n_dcn == {"dla": 16, "dlav1": 16, "hourglass": 0, "resdcn": 3}[arch.split("_")[0]]
    h = G.homogeneous(sd, a)
    assert list(h) == list(sd)
    for k, v in sd.items():
        want = v * a if k in up else v / a if k in down else v
        assert torch.equal(h[k], want) and h[k].dtype == v.dtype, k
    # every additive constant is in `up`: nothing 1-D but a BN / GN gamma and a variance stays
    for k, v in sd.items():
        if v.is_floating_point() and k not in up and k not in down and v.dim() == 1:
            assert k.endswith((".weight", ".running_var", "conv_offset_mask.bias")), k

    g, factors, moved = G.gauge(sd, T)
    sites = G.gauge_sites(sd)
    assert list(factors) == [s[0] for s in sites] and len(set(factors)) == len(sites)
    assert all(G.is_pow2(f) for f in factors.values()) and all(G.is_pow2(al) for al in ALPHAS)
    fs = list(factors.values())
    assert all(fs[i] == 2.0 ** (T if i % 2 == 0 else -T) for i in range(len(fs)))  # neighbours differ by 2^(2T)
    touched = {}
    for site, ups, downs, tap in sites:
        for k in ups:
            assert k not in touched and torch.equal(g[k], sd[k] * factors[site]), k
            touched[k] = site
        for k in downs:
            assert k not in touched and torch.equal(g[k], sd[k] / factors[site]), k
            touched[k] = site
    assert all(torch.equal(g[k], v) for k, v in sd.items() if k not in touched)
    blocks = [k[:-11] for k in sd if k.endswith(".bn1.weight") and k[:-10] + "conv2.weight" in sd]
    heads = R.CASES[key]["heads"]
    n_heads = {"dla": len(heads), "dlav1": len(heads), "hourglass": 2 * len(heads), "resdcn": len(heads)}[arch.split("_")[0]]
    extra = {"dla": 2, "dlav1": 2, "hourglass": 0, "resdcn": 3}[arch.split("_")[0]]  # the stem and level0; the BNs after the DCNs
    assert len(sites) == len(blocks) + n_heads + extra
    in_case = [t for t in moved if t in R.CASES[key]["taps"]]
    if arch.startswith("dla"):
        assert len(in_case) == 12 + 2 and sum(t.endswith(".conv1") for t in in_case) == 12
    elif arch.startswith("resdcn"):
        assert in_case == ["deconv_layers.2", "deconv_layers.8", "deconv_layers.14"]
    else:
        assert in_case == []


def test_scope_of_the_homogeneous_transform():
    for key, c in R.CASES.items():
        names = list(c["taps"]) + ["head:" + h for h in c["heads"]]
        out = [n for n in names if not G.in_scope(key, n)]
        if c["arch"].startswith("dlav1"):
            assert out == [t for t in c["taps"] if t in R.GRU_TAPS] + ["head:" + h for h in c["heads"]]
            assert names[names.index("feat") + 1:] == out  # everything through feat is in scope
        else:
            assert out == []
    assert G.homogeneous_factor("ida_up.node_1.offmask", 4.0) == 1.0 and G.homogeneous_factor("ida_up.node_1", 4.0) == 4.0


HOM_PASSES = [(k, d, a) for k, d in PASSES for a in ALPHAS if d == torch.float64 or a == ALPHAS[0]]  # one float32 pass per graph


@pytest.mark.parametrize("key,dtype,a", HOM_PASSES, ids=["%s-%s-a=%g" % (k, str(d).split(".")[1], a) for k, d, a in HOM_PASSES])
def test_homogeneous_scaling_is_exact_on_the_oracle(key, dtype, a):
    base = _base(key, dtype)
    x, kw = R.inputs(key)
    got = _transformed(key, dtype, G.homogeneous(R.state_dict(key), a), *G.homogeneous_inputs(x, kw, a))
    assert set(got) == set(base)
    for name in R.reference(key).names:
        same = torch.equal(got[name], base[name] * G.homogeneous_factor(name, a))
        # out of scope means it does move: sigmoid, tanh and GroupNorm are not homogeneous
        assert same == G.in_scope(key, name), (name, R.rel_err(got[name] / G.homogeneous_factor(name, a), base[name].double()))


@pytest.mark.parametrize("key,dtype", PASSES, ids=IDS)
def test_gauge_change_preserves_the_function_on_the_oracle(key, dtype):
    base = _base(key, dtype)
    x, kw = R.inputs(key)
    sd, factors, moved = G.gauge(R.state_dict(key), T)
    got = _transformed(key, dtype, sd, x, kw)
    for name in R.reference(key).names:
        f = moved.get(name, 1.0)
        assert torch.equal(got[name], base[name] * f), (name, f)
        if f != 1.0:
            assert not torch.equal(got[name], base[name]), name
