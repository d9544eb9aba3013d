"""Layer-by-layer parity of the engine against a float64 oracle: the cases, their tap names in network order, the float64 and
float32 oracle passes (computed once per case and shared) and the limit a tap is held to.  No tests in here:
tests/test_layer_parity_cpu.py checks the oracle side, tests/test_layer_parity_gpu.py the engine.

A tap or head t of a case is measured as  err[t] = max|engine - f64| / max|f64|  and held to

    err[t] <= M[precision] * max(e32[t], E32_MIN),      e32[t] = max|f32 oracle - f64 oracle| / max|f64|

i.e. the engine may be M times as far from the float64 tensor as a plain float32 evaluation of the same graph is (or as
E32_MIN, about 2.5 float32 epsilons, where that evaluation happens to land closer).  E32_CAP keeps a sick reference from
raising the limit: with M <= 8 no tap is allowed more than 1e-4 of its range, a tenth of the whole-network head gates.

M is 4 x the largest ratio err / max(e32, E32_MIN) measured on an MI355X over every tap, case and kernel selection, rounded
up to a power of two and capped at 8 ("Per-layer error against float64"); the factor 4 is the box-to-box and
summation-order spread of a max statistic, the same headroom the per-operator tests keep.  Measured: f32 1.35 -> 8.
f16x3 5.37: the rule asks for 32, the cap holds it at 8, so that mode has 1.5 x headroom and not 4 x.  Its distance grows
with depth from 0.9 x the float32 floor at the stem to 3 - 5 x from level 4 on, in every kernel alike: the split into two
binary16 numbers keeps 22 of float32's 24 mantissa bits of each operand, by construction, and no single layer is at fault."""
import re
from collections import OrderedDict

import torch

from centerpose_amd import synth

E32_MIN = 3e-7
E32_CAP = 1e-5
M = {"f32": 8, "f16x3": 8}
assert all(v * E32_CAP <= 1e-4 for v in M.values())

# every tap of the DLA-34 graph the oracle records, in the order the network computes them
DLA_TAPS = (
    "base.base_layer", "base.level0", "base.level1",
    "base.level2.bottom", "base.level2.project",
    "base.level2.tree1.conv1", "base.level2.tree1", "base.level2.tree2.conv1", "base.level2.tree2", "base.level2.root",
    "base.level3.bottom", "base.level3.tree1.bottom", "base.level3.tree1.project",
    "base.level3.tree1.tree1.conv1", "base.level3.tree1.tree1", "base.level3.tree1.tree2.conv1", "base.level3.tree1.tree2",
    "base.level3.tree1.root",
    "base.level3.tree2.tree1.conv1", "base.level3.tree2.tree1", "base.level3.tree2.tree2.conv1", "base.level3.tree2.tree2",
    "base.level3.tree2.root",
    "base.level4.bottom", "base.level4.tree1.bottom", "base.level4.tree1.project",
    "base.level4.tree1.tree1.conv1", "base.level4.tree1.tree1", "base.level4.tree1.tree2.conv1", "base.level4.tree1.tree2",
    "base.level4.tree1.root",
    "base.level4.tree2.tree1.conv1", "base.level4.tree2.tree1", "base.level4.tree2.tree2.conv1", "base.level4.tree2.tree2",
    "base.level4.tree2.root",
    "base.level5.bottom", "base.level5.project",
    "base.level5.tree1.conv1", "base.level5.tree1", "base.level5.tree2.conv1", "base.level5.tree2", "base.level5.root",
    "dla_up.ida_0.proj_1.offmask", "dla_up.ida_0.proj_1", "dla_up.ida_0.up_1", "dla_up.ida_0.node_1.offmask", "dla_up.ida_0.node_1",
    "dla_up.ida_1.proj_1.offmask", "dla_up.ida_1.proj_1", "dla_up.ida_1.up_1", "dla_up.ida_1.node_1.offmask", "dla_up.ida_1.node_1",
    "dla_up.ida_1.proj_2.offmask", "dla_up.ida_1.proj_2", "dla_up.ida_1.up_2", "dla_up.ida_1.node_2.offmask", "dla_up.ida_1.node_2",
    "dla_up.ida_2.proj_1.offmask", "dla_up.ida_2.proj_1", "dla_up.ida_2.up_1", "dla_up.ida_2.node_1.offmask", "dla_up.ida_2.node_1",
    "dla_up.ida_2.proj_2.offmask", "dla_up.ida_2.proj_2", "dla_up.ida_2.up_2", "dla_up.ida_2.node_2.offmask", "dla_up.ida_2.node_2",
    "dla_up.ida_2.proj_3.offmask", "dla_up.ida_2.proj_3", "dla_up.ida_2.up_3", "dla_up.ida_2.node_3.offmask", "dla_up.ida_2.node_3",
    "ida_up.proj_1.offmask", "ida_up.proj_1", "ida_up.up_1", "ida_up.node_1.offmask", "ida_up.node_1",
    "ida_up.proj_2.offmask", "ida_up.proj_2", "ida_up.up_2", "ida_up.node_2.offmask", "ida_up.node_2",
    "feat",
)
GRU_TAPS = ("convGRU.step0", "convGRU.step1", "convGRU.step2", "convGRU.step3")
HOURGLASS_TAPS = (
    "pre",
    "kps.0.low2.low2.low2.low2", "kps.0.low2.low2.low2", "kps.0.low2.low2", "kps.0.low2", "kps.0", "cnvs.0",
    "kps.1.low2.low2.low2.low2", "kps.1.low2.low2.low2", "kps.1.low2.low2", "kps.1.low2", "kps.1", "cnvs.1",
)
RESDCN_TAPS = (
    "maxpool", "layer1", "layer2", "layer3", "layer4",
    "deconv_layers.2", "deconv_layers.5", "deconv_layers.8", "deconv_layers.11", "deconv_layers.14", "deconv_layers.17",
)

# The smallest shapes at which every level is still ragged or at its minimum (level 5 of 96 x 160 is 3 x 5, the deepest
# hourglass level of 128 x 256 is 1 x 2).  key -> arch, heads, tracking task, HipModel keywords, (B, H, W), taps in network order
CASES = OrderedDict([
    ("dla_34-2x96x160", dict(arch="dla_34", heads=synth.HEADS_POSE, tracking=False, kw={}, shape=(2, 96, 160),
                             taps=DLA_TAPS)),
    ("dla_34-3x160x96", dict(arch="dla_34", heads=synth.HEADS_POSE, tracking=False, kw={}, shape=(3, 160, 96),
                             taps=DLA_TAPS)),
    ("dlav1_34_track-2x96x160", dict(arch="dlav1_34", heads=synth.HEADS_TRACK, tracking=True, kw={}, shape=(2, 96, 160),
                                     taps=DLA_TAPS + GRU_TAPS)),
    ("dlav1_34-1x128x128", dict(arch="dlav1_34", heads=synth.HEADS_POSE, tracking=False, kw={}, shape=(1, 128, 128),
                                taps=DLA_TAPS + GRU_TAPS[:3])),
    ("hourglass-1x128x256", dict(arch="hourglass", heads=synth.HEADS_POSE, tracking=False, kw={}, shape=(1, 128, 256),
                                 taps=HOURGLASS_TAPS)),
    ("resdcn_18-2x96x160", dict(arch="resdcn_18", heads=synth.HEADS_POSE, tracking=False, kw=dict(head_conv=64),
                                shape=(2, 96, 160), taps=RESDCN_TAPS)),
])

_NODE = re.compile(r"\.node_\d+(\.offmask)?$")


def changes_form(tap):
    """Does a tap of this name move the engine's launch sequence beyond switching the fused heads off?  (engine_forward.hip:
    the stem + level0 fusion yields to a tap on the stem's output; project_fusable(): a tap on any entry's projection runs every
    projection as a launch of its own; ida(): a tap on a node or its offset / mask map runs the IDAUps' stand-alone up-sample + add
    launches.)  Every other tap is form-preserving: the tapped pass launches what the untapped pass does, heads aside."""
    return tap == "base.base_layer" or tap.endswith(".project") or _NODE.search(tap) is not None


def state_dict(key):
    c = CASES[key]
    return synth.make_state_dict(c["arch"], c["heads"], c["tracking"])


def inputs(key):
    """-> (x, keyword inputs) on the CPU; the tracking task gets all three previous-frame inputs"""
    c = CASES[key]
    B, H, W = c["shape"]
    x = synth.frames(B, seed=29, h=H, w=W)
    kw = {}
    if c["tracking"]:
        kw = dict(pre_img=synth.frames(B, seed=30, h=H, w=W),
                  pre_hm=torch.rand(B, 1, H, W, generator=synth._gen(29, "pre_hm")) ** 8,
                  pre_hm_hp=torch.rand(B, 8, H, W, generator=synth._gen(29, "pre_hm_hp")) ** 8)
    return x, kw


def oracle(key, dtype, hook=None, sd=None, x=None, kw=None):
    """One oracle pass of a case in `dtype` -> (taps in the order recorded, heads).  `sd`, `x`, `kw`: another state dict and
    other inputs of the case's graph and shape (tests/scale_gauge_ref.py's transformed models); the case's own by default."""
    from oracle import backbone as ob
    from oracle import hourglass as oh
    from tests.resdcn_ref import torch_resdcn_forward

    c = CASES[key]
    if sd is None:
        sd = state_dict(key)
    if x is None:
        x, kw = inputs(key)
    taps = OrderedDict()
    nthreads = torch.get_num_threads()
    torch.set_num_threads(min(16, nthreads))
    try:
        with torch.no_grad():
            if c["arch"] == "hourglass":
                assert hook is None
                sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
                z = oh.hourglass_forward(sd, x.to(dtype), c["heads"], hook=lambda name, t: taps.__setitem__(name, t))
            elif c["arch"].startswith("resdcn"):
                assert hook is None
                z = torch_resdcn_forward(sd, x, int(c["arch"].split("_")[1]), c["heads"], dtype=dtype, taps=taps)
            else:
                z = ob.dlaseg_forward(sd, x, c["heads"], arch=c["arch"].split("_")[0], tracking_task=c["tracking"],
                                      hook=hook, taps=taps, dtype=dtype, **kw)
    finally:
        torch.set_num_threads(nthreads)  # process-global: later tests see the setting they started with
    assert all(t.dtype == dtype for t in taps.values()) and all(t.dtype == dtype for t in z.values()), key
    return taps, OrderedDict((h, z[h]) for h in c["heads"])


def rel_err(t, ref64):
    """max|t - ref| / max|ref| in float64"""
    return float((t.double() - ref64).abs().max() / ref64.abs().max())


class Reference:
    """names: the case's taps in network order, then its heads as 'head:<name>'; f64[name], f32[name]: the oracle's tensors;
    e32[name]: the float32 pass's own distance from the float64 one."""

    def __init__(self, key):
        taps64, z64 = oracle(key, torch.float64)
        taps32, z32 = oracle(key, torch.float32)
        self.key = key
        self.recorded = list(taps64)  # as the oracle named and ordered them
        self.f64, self.f32 = OrderedDict(), OrderedDict()
        for name in CASES[key]["taps"]:
            self.f64[name], self.f32[name] = taps64[name], taps32[name]
        for h in z64:
            self.f64["head:" + h], self.f32["head:" + h] = z64[h], z32[h]
        self.names = list(self.f64)
        self.e32 = OrderedDict((n, rel_err(self.f32[n], self.f64[n])) for n in self.names)

    def limit(self, name, precision):
        return M[precision] * max(self.e32[name], E32_MIN)


_refs = {}


def reference(key):
    """The case's oracle passes, computed once per process and left unchanged."""
    if key not in _refs:
        _refs[key] = Reference(key)
    return _refs[key]
