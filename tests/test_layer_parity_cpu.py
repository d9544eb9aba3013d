"""The oracle side of the per-layer parity test (tests/layer_parity_ref.py): its tap names against the engine's source, the
float32 pass's own distance from the float64 pass (the unit the GPU test's limit is written in), the two DCN restatements
against each other, and the premise of the whole exercise -- a border fault the head gates let through is far outside a
per-layer limit."""
import os
import re

import pytest
import torch

from oracle import dcn as odcn
from tests import layer_parity_ref as R

ENGINE_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "centerpose_amd", "csrc", "engine_forward.hip")

# tap name -> the call in engine_forward.hip that serves it
ENGINE_TAP_CALLS = [
    (r"^(base\.base_layer|base\.level0|base\.level1|feat|pre|maxpool)$", lambda m: 'tap("%s", ' % m.group(1)),
    (r"\.tree[12]\.conv1$", lambda m: 'tap(p + ".conv1", t);'),
    (r"\.tree[12]$", lambda m: "tap(p, o);"),
    (r"\.bottom$", lambda m: 'tap(p + ".bottom", '),
    (r"\.project$", lambda m: 'tap(p + ".project", proj);'),
    (r"\.root$", lambda m: 'tap(p + ".root", o);'),
    (r"\.(proj|node)_\d\.offmask$", lambda m: 'tap(p + ".offmask", om, 27);'),
    (r"\.(proj|node)_\d$", lambda m: "if (!up) tap(p, o);"),
    (r"\.up_\d$", lambda m: 'tap(p + ".up_" + k, u);'),
    (r"^convGRU\.step\d$", lambda m: 'tap(("convGRU.step" + std::to_string(st)).c_str(), h);'),
    (r"^kps\.\d(\.low2)*$", lambda m: "tap(p, out);"),
    (r"^cnvs\.\d$", lambda m: 'tap("cnvs." + ks, cnv);'),
    (r"^layer[1-4]$", lambda m: "tap(ln, x);"),
    (r"^deconv_layers\.(2|8|14)$", lambda m: 'tap("deconv_layers." + std::to_string(6 * i + 2), x);'),
    (r"^deconv_layers\.(5|11|17)$", lambda m: 'tap("deconv_layers." + std::to_string(6 * i + 5), x);'),
]


@pytest.mark.parametrize("key", list(R.CASES))
def test_tap_names_are_the_oracles_and_the_engines(key):
    ref = R.reference(key)
    assert ref.recorded == list(R.CASES[key]["taps"])  # the same set, in network order
    with open(ENGINE_SRC) as f:
        src = f.read()
    for name in R.CASES[key]["taps"]:
        calls = [make(m) for pat, make in ENGINE_TAP_CALLS for m in [re.search(pat, name)] if m]
        assert len(calls) == 1, name
        assert calls[0] in src, (name, calls[0])


def test_form_table():
    changing = [t for t in R.DLA_TAPS if R.changes_form(t)]
    assert changing[0] == "base.base_layer" and len(changing) == 1 + 4 + 8 + 8  # the stem, the projections, the nodes and their maps
    assert not any(R.changes_form(t) for t in R.GRU_TAPS + R.HOURGLASS_TAPS + R.RESDCN_TAPS)
    assert not R.changes_form("ida_up.proj_1.offmask") and R.changes_form("ida_up.node_1.offmask")
    assert all(m * R.E32_CAP <= 1e-4 for m in R.M.values())  # no tap is allowed more than 1e-4 of its range


@pytest.mark.parametrize("key", list(R.CASES))
def test_float32_floor_is_capped(key):
    """The limit's unit must not drift up through a sick reference: every tap and head of the float32 pass is within 1e-5 of
    range of the float64 pass (measured: 3e-7 at the stems, 4.1e-6 at the worst tap, a ConvGRU step)."""
    ref = R.reference(key)
    assert len(ref.names) == len(R.CASES[key]["taps"]) + len(R.CASES[key]["heads"])
    for name in ref.names:
        assert ref.f64[name].dtype == torch.float64 and ref.f32[name].dtype == torch.float32, name
        assert ref.f64[name].shape == ref.f32[name].shape, name
        assert bool(torch.isfinite(ref.f64[name]).all()), name
        assert 0.0 < ref.e32[name] <= R.E32_CAP, (name, ref.e32[name])


def test_dcn_float64_and_float32_port_agree():
    """Every deformable layer of the dla_34 case on its float32 inputs: the C port (float32) against the float64 gather."""
    key = "dla_34-2x96x160"
    ref = R.reference(key)
    sd = R.state_dict(key)
    t = ref.f32
    layers = [t["base.level0"], t["base.level1"], t["base.level2.root"], t["base.level3.tree2.root"],
              t["base.level4.tree2.root"], t["base.level5.root"]]
    dcns = []  # (name, input): the walk of DLAUp.forward / IDAUp.forward over the recorded tensors

    def ida(layers, p, startp, endp):
        for i in range(startp + 1, endp):
            k = i - startp
            dcns.append(("%s.proj_%d" % (p, k), layers[i]))
            dcns.append(("%s.node_%d" % (p, k), t["%s.up_%d" % (p, k)]))  # (the tap is the sum the node reads)
            layers[i] = t["%s.node_%d" % (p, k)]

    out = [layers[-1]]
    for i in range(3):
        ida(layers, "dla_up.ida_%d" % i, 6 - i - 2, 6)
        out.insert(0, layers[-1])
    ida(out[:3], "ida_up", 0, 3)
    assert len(dcns) == 16
    for name, x in dcns:
        om = t[name + ".offmask"]
        off, mask = om[:, :18].contiguous(), om[:, 18:].contiguous()
        w, b = sd[name + ".conv.weight"], sd[name + ".conv.bias"]
        y32 = odcn.dcn_v2_forward(x, w, b, off, mask, 3, 3, 1, 1, 1, 1, 1, 1, 1)
        y64 = odcn.dcn_v2_forward(x.double(), w, b, off, mask, 3, 3, 1, 1, 1, 1, 1, 1, 1)  # dispatches on the input's type
        assert y32.dtype == torch.float32 and y64.dtype == torch.float64 and y32.shape == y64.shape, name
        assert R.rel_err(y32, y64) <= 1e-5, (name, R.rel_err(y32, y64))


def test_head_gates_miss_a_border_fault_a_layer_limit_catches():
    """The last output row of base.level2.tree1.conv2 scaled by 0.99 in the float32 oracle: both heat-maps move by less
    than the 1e-3 the whole-network tests allow, while the layer's own output is far outside 32 x its float32 floor."""
    key = "dla_34-2x96x160"
    ref = R.reference(key)

    def fault(name, kind, y):
        if name != "base.level2.tree1.conv2":
            return None
        y = y.clone()
        y[:, :, -1, :] *= 0.99
        return y

    taps0, z0 = R.oracle(key, torch.float32, hook=lambda name, kind, y: None)  # (the hooked path, no fault)
    taps1, z1 = R.oracle(key, torch.float32, hook=fault)
    for h in ("hm", "hm_hp"):
        d = float((torch.sigmoid(z1[h]) - torch.sigmoid(z0[h])).abs().max())
        print("%s: %.3e" % (h, d))
        assert 0.0 < d < 1e-3, (h, d)
    tap = "base.level2.tree1"
    moved = float((taps1[tap] - taps0[tap]).abs().max() / ref.f64[tap].abs().max())
    print("%s: %.3e of range, floor %.3e" % (tap, moved, ref.e32[tap]))
    assert moved > 32 * ref.e32[tap], (moved, ref.e32[tap])
    assert R.rel_err(taps1[tap], ref.f64[tap]) > 32 * ref.e32[tap]
