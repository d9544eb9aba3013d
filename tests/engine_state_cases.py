"""What tests/test_engine_state_gpu.py shares: the models, shapes and call kinds of the history-independence tests, and the
reference of every one of them -- the same call as the FIRST call of a freshly built model.

The property under test is that a HipModel has no memory: whatever it was asked before (another shape, precision, switch
setting, a tap, a profile, another detect kind, a refused call), a call returns bit for bit what a model built a moment ago
from the same state dict returns for it.  The fresh model's single call is already held to the float64 oracle layer by layer
(tests/test_layer_parity_gpu.py), so nothing numeric is re-derived here and every comparison is ``torch.equal``.

A result is an OrderedDict name -> tensor (a clone: detect's outputs belong to the model) or int.  ``forward`` and ``features``
results also carry the pass's ``maxpool_launches`` and ``workspace_used``."""
from collections import OrderedDict

import torch

from centerpose_amd import hip, synth
from tests.engine_plan_cases import MODELS

A = (1, 128, 128)     # the pinned pair of work-space sizes: 8,781,824 bytes in f16x3, 20,709,376 in f32 (engine_plan_pins.json)
B = (2, 96, 160)      # ragged at every level
A_WIDE = (1, 128, 256)  # (the hourglass takes multiples of 128 only: its second shape)
LEAN_HW = (256, 256)  # the lean detect's frames; the batch is found with the query (lean_batch)

_sd = {}
_fresh = {}
_side = {}


def state_dict(key):
    if key not in _sd:
        arch, heads, tracking, kw = MODELS[key]
        _sd[key] = synth.make_state_dict(arch, heads, tracking)
    return _sd[key]


def build(key, prec):
    """A new HipModel of MODELS[key]: never shared, never cached."""
    arch, heads, tracking, kw = MODELS[key]
    return hip.HipModel(arch, heads, state_dict(key), tracking_task=tracking, precision=prec, **kw)


def inputs(key, shape, device, seed=29):
    """-> (images, keywords): the tracking task gets all three previous-frame inputs"""
    n, h, w = shape
    x = synth.frames(n, seed=seed, h=h, w=w).to(device)
    kw = {}
    if MODELS[key][2]:
        kw = dict(pre_img=synth.frames(n, seed=seed + 1, h=h, w=w).to(device),
                  pre_hm=(torch.rand(n, 1, h, w, generator=synth._gen(seed, "pre_hm")) ** 8).to(device),
                  pre_hm_hp=(torch.rand(n, 8, h, w, generator=synth._gen(seed, "pre_hm_hp")) ** 8).to(device))
    return x, kw


def side(device):
    """The non-default stream every call of these tests runs on (a graph capture needs one)."""
    if str(device) not in _side:
        _side[str(device)] = torch.cuda.Stream(device=device)
    return _side[str(device)]


def lean_batch(m):
    """The smallest batch of LEAN_HW frames for which detect(heads="lazy") takes the lean path on ``m``."""
    for n in range(1, 33):
        if m.lean_supported(n, *LEAN_HW):
            return n
    raise AssertionError("no batch up to 32 of %dx%d frames takes the lean path" % LEAN_HW)


def _counters(m, r):
    r["maxpool_launches"] = m.maxpool_launches()
    r["workspace_used"] = m.workspace_used()
    return r


def call(m, kind, x, kw, K=100, graph=False):
    """One call of ``kind`` on ``m``, on the side stream, synchronised -> (result, what detect returned for the heads or None).
    kinds: "forward", "forward_sig" (sigmoid_hm=True), "features", "tap:<name>", "dense" (detect, every map), "lazy" (detect,
    the lean path where the model supports it)."""
    s = side(x.device)
    r, heads = OrderedDict(), None
    with torch.cuda.stream(s):
        if kind in ("forward", "forward_sig"):
            for k, v in m.forward(x, sigmoid_hm=kind == "forward_sig", **kw).items():
                r[k] = v
            _counters(m, r)
        elif kind == "features":
            r["features"] = m.features(x, **kw)
            _counters(m, r)
        elif kind.startswith("tap:"):
            outs, t = m.forward(x, tap=kind[4:], **kw)
            for k, v in outs.items():
                r[k] = v
            r[kind] = t
        elif kind in ("dense", "lazy"):
            heads, det = m.detect(x, K=K, graph=graph, heads=kind, **kw)
            if isinstance(heads, hip.LazyHeads):
                r["hm"], r["hm_hp"] = heads["hm"], heads["hm_hp"]
                r["pk_score"], r["pk_ind"] = heads.pk_score, heads.pk_ind
                for k, v in heads.gathered.items():
                    r["gathered:" + k] = v
            else:
                for k, v in heads.items():
                    r[k] = v
            r["det"] = det
        else:
            raise ValueError(kind)
        s.synchronize()
        for k, v in r.items():
            if torch.is_tensor(v):
                r[k] = v.clone()
        s.synchronize()
    return r, heads


def fresh(key, prec, kind, shape, device, seed=29, K=100, sel=0, cached=True):
    """The reference: ``kind`` as the first and only call of a model built for it (under the switches ``sel``).  Computed once
    per argument tuple and shared; ``cached=False`` builds another model and computes it again (the control)."""
    ck = (key, prec, kind, tuple(shape), seed, K, int(sel))
    if cached and ck in _fresh:
        return _fresh[ck]
    m = build(key, prec)
    x, kw = inputs(key, shape, device, seed)
    with hip.select_kernels(sel):
        r, _ = call(m, kind, x, kw, K=K)
    del m
    if cached:
        _fresh[ck] = r
    return r


def differing(got, want):
    """Names whose values are not bit-equal (or missing on one side): [] means the two results are the same."""
    bad = [k for k in want if k not in got] + [k for k in got if k not in want]
    for k in want:
        if k in got:
            a, b = got[k], want[k]
            same = (a.shape == b.shape and torch.equal(a, b)) if torch.is_tensor(b) else a == b
            if not same:
                bad.append(k if torch.is_tensor(b) else "%s (%r, fresh %r)" % (k, a, b))
    return bad
