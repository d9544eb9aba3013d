"""The f16x3 pre-scale (every tensor's running |max|: cp_amax_commit / cp_amax_read / cp_amax_to_scale) under the two exact
transforms of tests/scale_gauge_ref.py, at every tap of every case of tests/layer_parity_ref.py.

synth's models keep every activation at O(1), where binary16 has 2^14 of room either way: a launch that forgets to commit its
|max|, reads another tensor's slot or takes a bound that is none passes every parity test.  Here the stored activations sit
2^14 above or below that (A: homogeneous scaling, all alike) or alternate by 2^24 from one tensor to the next (B: the gauge
change), and the engine must compute what it computed for the base model:

  A1  engine(homogeneous(sd, a), a x) / a within layer_parity_ref's limit of the cached float64 reference of the BASE case
      (tests/test_scale_equivariance_cpu.py: the transformed model's oracle is a times that one, bit for bit);
  A2  ... and equal to a times the base model's engine tensor, bit for bit: every partial sum is scaled by the same power of
      two.  f32 is the control: plain IEEE, no |max| involved;
  B   the gauged model's taps and heads bit-identical to the base model's (the tensors between the gauged pairs times their f),
      the records of detect() included;
  C   A2 and B under every forced kernel selection that has load / commit code of its own;
      and, bitwise on the untapped heads, at 8 x 256 x 256, where the whole-launch kernels have launches to take;
  D   a pass does not depend on the magnitudes of the pass before it (the slot block is zeroed per pass);
  E   the teeth: without the pre-scale (KernelSel.NO_PRESCALE) the scaled hourglass case fails A1.

No tolerance of its own: the gate is layer_parity_ref's limit, everything else is torch.equal."""
import pytest
import torch

from centerpose_amd import hip, synth
from tests import layer_parity_ref as R
from tests import scale_gauge_ref as G
from tests import test_layer_parity_gpu as L
from tests.test_lean_detect_gpu import dla  # noqa: F401  (the small dla_34 fixture: heads, state dict, f16x3 model)

pytestmark = pytest.mark.gpu

S = hip.KernelSel
ALPHAS = {"2^14": 2.0 ** 14, "2^-14": 2.0 ** -14}
T = 12
PRECS = ("f32", "f16x3")

_models = {}
_reached = set()  # every kernel variant a scaled or gauged pass ran, for the table in DESIGN.md


def _variant_sd(key, variant):
    """variant: 'base', ('hom', a) or 'gauge' -> (state dict, x, keyword inputs, {tap or head: factor against the base})"""
    sd = R.state_dict(key)
    x, kw = R.inputs(key)
    names = R.reference(key).names
    if variant == "base":
        return sd, x, kw, {n: 1.0 for n in names}
    if variant == "gauge":
        sd, _, moved = G.gauge(sd, T)
        return sd, x, kw, {n: moved.get(n, 1.0) for n in names}
    a = variant[1]
    x, kw = G.homogeneous_inputs(x, kw, a)
    return G.homogeneous(sd, a), x, kw, {n: G.homogeneous_factor(n, a) for n in names if G.in_scope(key, n)}


def _model(key, variant):
    c = R.CASES[key]
    mk = (c["arch"], tuple(c["heads"]), c["tracking"], variant)
    if mk not in _models:
        _models[mk] = hip.HipModel(c["arch"], c["heads"], _variant_sd(key, variant)[0], tracking_task=c["tracking"], **c["kw"])
    return _models[mk]


_passes = {}


def _engine(key, prec, switches, variant, device, profile_all=False):
    """Every tap and head of one model variant -> ({name: tensor}, kernels of the untapped pass, kernels of all passes)"""
    ck = (key, prec, int(switches), variant)
    if ck in _passes and not (profile_all and _passes[ck][2] is None):
        return _passes[ck]
    c = R.CASES[key]
    m = _model(key, variant)
    m.set_precision(prec)
    _, x, kw, _ = _variant_sd(key, variant)
    x = x.to(device)
    kw = {k: v.to(device) for k, v in kw.items()}
    got = {}

    def taps():
        for tap in c["taps"]:
            _, got[tap] = m.forward(x, tap=tap, **kw)

    with hip.select_kernels(switches):
        heads, rows0 = L._launch_rows(m, lambda: m.forward(x, **kw))  # untapped: the production head kernels
        for h in c["heads"]:
            got["head:" + h] = heads[h]
        if profile_all:
            _, rows = L._launch_rows(m, taps)
        else:
            taps()
        torch.cuda.synchronize()
    _passes[ck] = (got, sorted({r[0] for r in rows0}), sorted({r[0] for r in rows} | {r[0] for r in rows0}) if profile_all else None)
    return _passes[ck]


def _first_moved(key, got, base, factors):
    """A2 / B: the first tap or head in network order that is not the base engine's times its factor, or None"""
    for name in R.reference(key).names:
        if name not in factors:
            continue
        want = base[name] * factors[name]
        if got[name].shape != want.shape or not torch.equal(got[name], want):
            if got[name].shape != want.shape:
                return "%s: shape %s, the base model's is %s" % (name, tuple(got[name].shape), tuple(want.shape))
            d = (got[name].double() - want.double()).abs()
            return "%s (x %g): %d of %d elements differ, max |diff| %.3e of the tensor's range, %d non-finite" % (
                name, factors[name], int((got[name] != want).sum()), want.numel(),
                float(d[torch.isfinite(d)].max() / want.double().abs().max()) if bool(torch.isfinite(d).any()) else float("nan"),
                int((~torch.isfinite(got[name])).sum()))
    return None


def _gate(key, prec, got, factors):
    """A1 -> (first tap or head in network order over layer_parity_ref's limit or None, worst err / max(e32, E32_MIN), its name)"""
    ref = R.reference(key)
    first, worst, at = None, 0.0, None
    for name in ref.names:
        if name not in factors:
            continue
        r = L._measure(got[name] / factors[name], ref.f64[name])
        if isinstance(r, str):
            first = first or "%s: %s" % (name, r)
            worst, at = float("inf"), at if worst == float("inf") else name
            continue
        err, idx = r
        ratio = err / max(ref.e32[name], R.E32_MIN)
        if ratio > worst:
            worst, at = ratio, name
        if err > ref.limit(name, prec) and first is None:
            first = "%s: err %.3e of range > limit %.3e, worst element %s" % (name, err, ref.limit(name, prec), idx)
    return first, worst, at


def _check_homogeneous(device, key, prec, switches, label, profile_all=False):
    base, k0, _ = _engine(key, prec, switches, "base", device)
    problems, ran = [], set()
    for an, a in ALPHAS.items():
        got, kernels, every = _engine(key, prec, switches, ("hom", a), device, profile_all)
        ran |= set(every or kernels)
        factors = _variant_sd(key, ("hom", a))[3]
        over, worst, at = _gate(key, prec, got, factors)
        print("scale-equivariance A1 %s %s %s a=%s: worst err / max(e32, %g) = %.2f at %s (M = %d), %d tensors"
              % (key, prec, label, an, R.E32_MIN, worst, at, R.M[prec], len(factors)))
        if over:
            problems.append("A1 a=%s: first tensor over its limit, in network order -- %s" % (an, over))
        moved = _first_moved(key, got, base, factors)
        if moved:
            problems.append("A2 a=%s: first tensor that is not a x the base model's, in network order -- %s" % (an, moved))
        if problems and kernels != k0:
            problems.append("kernels of the untapped pass, a=%s: %s" % (an, " ".join(kernels)))
    _reached.update(ran)
    print("scale-equivariance A %s %s %s: kernels of the scaled passes: %s" % (key, prec, label, " ".join(sorted(ran))))
    if problems:
        problems.append("kernels of the base model's untapped pass: %s" % " ".join(k0))
    return problems, ran


def _check_gauge(device, key, prec, switches, label, profile_all=False):
    base, k0, _ = _engine(key, prec, switches, "base", device)
    got, kernels, every = _engine(key, prec, switches, "gauge", device, profile_all)
    factors = _variant_sd(key, "gauge")[3]
    assert set(factors) == set(R.reference(key).names)  # the function is unchanged: every tap and head, GRU and GroupNorm included
    problems = []
    moved = _first_moved(key, got, base, factors)
    if moved:
        problems.append("B t=%d: first tensor that is not the base model's (times its f), in network order -- %s" % (T, moved))
        problems.append("kernels of the untapped pass: %s" % " ".join(kernels))
        problems.append("kernels of the base model's untapped pass: %s" % " ".join(k0))
    _reached.update(every or kernels)
    print("scale-equivariance B %s %s %s: %s; kernels of the gauged passes: %s"
          % (key, prec, label, "MOVED" if moved else "bit-identical", " ".join(every or kernels)))
    return problems, set(every or kernels)


AB = [(key, prec) for key in R.CASES for prec in PRECS]


@pytest.mark.parametrize("key,prec", AB, ids=["%s-%s" % p for p in AB])
def test_homogeneous_scaling(device, key, prec):
    """A1 and A2, a = 2^14 and 2^-14; dlav1_34: the taps through feat (sigmoid, tanh and GroupNorm are not homogeneous)"""
    problems, _ = _check_homogeneous(device, key, prec, 0, "default")
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("key,prec", AB, ids=["%s-%s" % p for p in AB])
def test_gauge_change(device, key, prec):
    """B: neighbouring tensors 2^24 apart, every tap and head as the base model's"""
    problems, _ = _check_gauge(device, key, prec, 0, "default")
    assert not problems, "\n".join(problems)


def test_gauge_change_leaves_the_detections_alone(device, dla):  # noqa: F811
    """B through detect(): the gauged hidden layer of every head through heads_at_rows (lean) and the grouped fused heads (dense)"""
    heads, sd, model = dla
    gauged = hip.HipModel("dla_34", heads, G.gauge(sd, T)[0], precision="f16x3")
    x = synth.frames(8, seed=59, h=256, w=256).to(device)
    assert model.lean_supported(8, 256, 256)
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        for mode in ("lazy", "dense"):
            _, det0 = model.detect(x, graph=False, heads=mode)
            det0 = det0.clone()
            outs, det1 = gauged.detect(x, graph=False, heads=mode)
            side.synchronize()
            assert isinstance(outs, hip.LazyHeads) == (mode == "lazy")
            assert bool(torch.isfinite(det0).all()) and float(hip.split_detections(det0)["scores"].max()) > 0.1
            assert torch.equal(det1, det0), (mode, int((det1 != det0).sum()))


# selections whose kernel has a launch to take at this shape only (tests/test_layer_parity_gpu.py: _has_site)
DETECT_SHAPE_SELECTIONS = {"default": 0, "upadd": L.SELECTIONS["upadd"][0], "DCN16S_ALWAYS": S.DCN16S_ALWAYS, "HALO_NEVER": S.HALO_NEVER}


@pytest.mark.parametrize("sel", list(DETECT_SHAPE_SELECTIONS))
def test_production_kernels_at_the_detect_shape(device, dla, sel):  # noqa: F811
    """A2 and B on the untapped heads at 8 x 256 x 256, the shape of the detect tests: none of layer_parity_ref's cases is large
    enough for the whole-launch kernels (patch-resident and streamed DCN, the fused up-add, halo16, the grouped fused heads), so
    the production sequence of a realistic shape gets its own pass.  No tap, no gate (no oracle pass of this size): bitwise only."""
    heads, sd, model = dla
    x = synth.frames(8, seed=59, h=256, w=256).to(device)
    problems, ran = [], set()
    with hip.select_kernels(DETECT_SHAPE_SELECTIONS[sel]):
        base, rows = L._launch_rows(model, lambda: model.forward(x))
        ran |= {r[0] for r in rows}
        variants = [("gauge t=%d" % T, G.gauge(sd, T)[0], 1.0)] + [("a=%s" % an, G.homogeneous(sd, a), a) for an, a in ALPHAS.items()]
        for label, vsd, a in variants:
            m = hip.HipModel("dla_34", heads, vsd, precision="f16x3")
            got, rows = L._launch_rows(m, lambda: m.forward(x * a))
            ran |= {r[0] for r in rows}
            torch.cuda.synchronize()
            for h in heads:
                if not torch.equal(got[h], base[h] * a):
                    problems.append("%s: head %s is not %g x the base model's (%d of %d elements differ)"
                                    % (label, h, a, int((got[h] != base[h] * a).sum()), base[h].numel()))
    print("scale-equivariance 8x256x256 %s: kernels: %s" % (sel, " ".join(sorted(ran))))
    _reached.update(ran)
    assert not problems, "\n".join(problems + ["kernels: " + " ".join(sorted(ran))])


CASE_C = "dla_34-2x96x160"
FORCED = [(name, CASE_C, L.SELECTIONS[name][0]) for name in L.SELECTIONS]
FORCED += [(f.name, CASE_C, f) for f in (S.HALO_ALWAYS, S.HALO_NEVER, S.PW16_NEVER, S.DCN16S_ALWAYS, S.DCN16P_ALWAYS, S.NO_HEAD_FUSION,
                                         S.STEM_LEVEL0_UNFUSED, S.NO_LOWC)]
FORCED += [(S.GRU_UNFUSED.name, "dlav1_34-1x128x128", S.GRU_UNFUSED)]


@pytest.mark.parametrize("sel,key,switches", FORCED, ids=[f[0] for f in FORCED])
def test_forced_kernels(device, sel, key, switches):
    """C: A2 (with its gate) and B in f16x3 under each forced selection; prints the kernel variants the scaled passes ran"""
    pa, ran_a = _check_homogeneous(device, key, "f16x3", switches, sel, profile_all=True)
    pb, ran_b = _check_gauge(device, key, "f16x3", switches, sel, profile_all=True)
    _reached.update(ran_a | ran_b)
    print("scale-equivariance C union so far (%d variants): %s" % (len(_reached), " ".join(sorted(_reached))))
    assert not (pa + pb), "\n".join(pa + pb)


def test_a_pass_forgets_the_one_before(device, dla):  # noqa: F811
    """D: x, then 2^14 x, then x on ONE model: the third pass is the first, bit for bit (heads and a deep tap); the same
    through detect()."""
    key = "dla_34-2x96x160"
    c = R.CASES[key]
    m = hip.HipModel(c["arch"], c["heads"], R.state_dict(key), precision="f16x3")
    x = R.inputs(key)[0].to(device)
    big = x * 2.0 ** 14
    tap = "base.level5.root"
    first = m.forward(x), m.forward(x, tap=tap)[1]
    loud = m.forward(big), m.forward(big, tap=tap)[1]
    third = m.forward(x), m.forward(x, tap=tap)[1]
    torch.cuda.synchronize()
    assert float(loud[1].abs().max()) > 2.0 ** 10 * float(first[1].abs().max())  # (the pass in between really was loud)
    for h in c["heads"]:
        assert torch.equal(third[0][h], first[0][h]), h
    assert torch.equal(third[1], first[1])

    heads, sd, model = dla
    x = synth.frames(8, seed=59, h=256, w=256).to(device)
    big = x * 2.0 ** 14
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        det0 = model.detect(x, graph=False)[1].clone()
        model.detect(big, graph=False)
        det2 = model.detect(x, graph=False)[1]
        side.synchronize()
        assert torch.equal(det2, det0)


def test_without_the_prescale_the_scaled_case_leaves_binary16(device):
    """E: the hourglass (no data-dependent addressing) at a = 2^14 under NO_PRESCALE fails the gate: A and B do depend on the
    pre-scale.  a = 2^-14 is printed only (binary16's subnormals lose bits gradually)."""
    key, prec = "hourglass-1x128x256", "f16x3"
    for an, a in ALPHAS.items():
        got, kernels, _ = _engine(key, prec, S.NO_PRESCALE, ("hom", a), device)
        over, worst, at = _gate(key, prec, got, _variant_sd(key, ("hom", a))[3])
        print("scale-equivariance E %s NO_PRESCALE a=%s: worst err / max(e32, %g) = %s at %s; first over the limit: %s"
              % (key, an, R.E32_MIN, "%.3e" % worst, at, over))
        if a > 1:
            assert over is not None, "a = 2^14 without the pre-scale passes the gate: the scaled cases do not leave binary16's range"
