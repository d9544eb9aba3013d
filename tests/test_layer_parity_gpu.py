"""Every engine layer against the float64 oracle, tap by tap (tests/layer_parity_ref.py has the cases, the reference and
the limit; tests/test_layer_parity_cpu.py checks that side).

One test per (case, precision, kernel selection): one forward per tap plus one untapped forward, whose heads come from the
production (fused) head kernels.  Each tensor must have the oracle's shape, be finite and lie within
M[precision] * max(e32, 3e-7) of the float64 tensor, as a fraction of that tensor's range.  A failure names the first tap in
network order over its limit -- the layer to open -- and then prints the whole table (as does a run with -s).

The form check makes this a test of the production kernels and not of a tap form: for every tap that leaves the launch
sequence alone (layer_parity_ref.changes_form) the ordered launch rows of the tapped pass -- variant, M, N, K, kh, stride,
role, from the CP_PROFILE_DUMP rows -- equal those of the untapped pass once the head stage's rows (roles head and head_final:
a tap switches the fused heads off) are taken out of both.  The taps that do change the sequence (the stem's output, the
entries' projections, the IDAUp nodes and their offset / mask maps) are compared all the same; the table marks them "plain":
they ran the plain launch sequence."""
import os
import tempfile

import pytest
import torch

from centerpose_amd import hip
from tests import layer_parity_ref as R

pytestmark = pytest.mark.gpu

S = hip.KernelSel
# selection -> (switches, prefix of the kernel variant that must then have run where it has a launch to take: _has_site)
SELECTIONS = {
    "default": (0, None),
    "upadd": (S.DCN16P_ALWAYS | S.DCN16T_ALWAYS, "dcn16t_f16x3"),  # (the switches of tests/engine_plan_cases.py's fused IDAUp pins)
    "strm16": (S.STRM16_ALWAYS, "strm16_f16x3"),
    "level1rows": (S.LEVEL1_ROWS_ALWAYS, "lowc_3x3s2_c16_rows_f16x3"),
}
PARAMS = [(key, prec, "default") for key in R.CASES for prec in ("f32", "f16x3")]
# the forced selections where the architecture has the site (the DLA graphs), in the arithmetic that has the kernel
PARAMS += [(key, "f16x3", sel) for key in R.CASES if R.CASES[key]["arch"].startswith("dla")
           for sel in ("upadd", "strm16", "level1rows")]


def _has_site(key, sel):
    """Does the forced kernel have a launch to take at the case's shape?  strm16 and the row-streamed level1 take any size.
    dcn16t -- like every patch-resident DCN kernel (cp_dcn16p_supported) -- takes whole launches over maps of whole 8 x 16
    patches only, and the up-add sites are the 64-channel nodes at a quarter of the input: such a node is a whole launch from
    128 tiles of 128 pixels on (engine_forward.hip: kSplitTiles; below that it is cut along K and runs on the gather kernel).
    None of the cases reaches that, 16384 node pixels, and an oracle pass that does takes tens of seconds: at these shapes the
    selection must leave the IDAUps on the plain sequence, whose up-sample + add launch every `up_k` tap compares;
    tests/test_upadd_epilogue_gpu.py holds the fused epilogue to that launch bit for bit."""
    B, H, W = R.CASES[key]["shape"]
    h, w = H // 4, W // 4
    return sel != "upadd" or (h % 8 == 0 and w % 16 == 0 and B * h * w >= 128 * 128)


_models = {}


def _model(key):
    c = R.CASES[key]
    mk = (c["arch"], tuple(c["heads"]), c["tracking"])
    if mk not in _models:
        _models[mk] = hip.HipModel(c["arch"], c["heads"], R.state_dict(key), tracking_task=c["tracking"], **c["kw"])
    return _models[mk]


def _launch_rows(m, run):
    """The pass `run` under the profiler -> (what it returned, its launch rows in order)"""
    m.profile(True)
    fd, dump = tempfile.mkstemp(suffix=".csv")
    os.close(fd)
    try:
        out = run()
        torch.cuda.synchronize()
        os.environ["CP_PROFILE_DUMP"] = dump  # per-launch rows: name, M, N, K, kh, stride, ms, TFLOP/s, role
        try:
            m.profile_read()
        finally:
            del os.environ["CP_PROFILE_DUMP"]
        rows = []
        with open(dump) as f:
            for line in f:
                name, M, N, K, kh, stride, _ms, _tf, role = line.strip().split(",")
                rows.append((name, int(M), int(N), int(K), int(kh), int(stride), role))
    finally:
        m.profile(False)
        os.remove(dump)
    return out, rows


def _body(rows):
    return [r for r in rows if r[6] not in ("head", "head_final")]


def _measure(t, ref64):
    """-> (error as a fraction of the reference's range, index of the worst element), or a string saying what is wrong"""
    if tuple(t.shape) != tuple(ref64.shape):
        return "shape %s, the oracle's is %s" % (tuple(t.shape), tuple(ref64.shape))
    t = t.detach().cpu().double()
    if not bool(torch.isfinite(t).all()):
        return "%d non-finite values" % int((~torch.isfinite(t)).sum())
    d = (t - ref64).abs()
    i = int(d.argmax())
    idx = []
    for n in reversed(ref64.shape):
        idx.append(i % n)
        i //= n
    return float(d.max() / ref64.abs().max()), tuple(reversed(idx))


@pytest.mark.parametrize("key,prec,sel", PARAMS, ids=["%s-%s-%s" % p for p in PARAMS])
def test_layers_vs_float64_oracle(device, key, prec, sel):
    ref = R.reference(key)
    c = R.CASES[key]
    switches, must_run = SELECTIONS[sel]
    m = _model(key)
    m.set_precision(prec)
    x, kw = R.inputs(key)
    x = x.to(device)
    kw = {k: v.to(device) for k, v in kw.items()}
    got, form = {}, {}
    problems = []
    with hip.select_kernels(switches):
        heads = m.forward(x, **kw)  # untapped: the production head kernels
        for h in c["heads"]:
            got["head:" + h], form["head:" + h] = heads[h], "untapped"
        _, rows0 = _launch_rows(m, lambda: m.forward(x, **kw))
        ran = must_run is not None and any(r[0].startswith(must_run) for r in rows0)
        if must_run and ran != _has_site(key, sel):
            problems.append("%s* launches under %s: %s, expected %s (%s)"
                            % (must_run, sel, ran, _has_site(key, sel), sorted({r[0] for r in rows0})))
        for tap in c["taps"]:
            _, got[tap] = m.forward(x, tap=tap, **kw)
            if R.changes_form(tap):
                form[tap] = "plain"  # compared as well, on the plain launch sequence
                continue
            form[tap] = "same"
            _, rows = _launch_rows(m, lambda: m.forward(x, tap=tap, **kw))
            if _body(rows) != _body(rows0):
                form[tap] = "MOVED"
                diff = [(i, a, b) for i, (a, b) in enumerate(zip(_body(rows), _body(rows0))) if a != b][:3]
                problems.append("tap %s changes the launch sequence (%d rows, untapped %d; first differences %s)"
                                % (tap, len(_body(rows)), len(_body(rows0)), diff))
        torch.cuda.synchronize()

    table = ["layer-parity %s %s %s   (M = %d)" % (key, prec, sel, R.M[prec]),
             "layer-parity kernels of the untapped pass: %s" % " ".join(sorted({r[0] for r in rows0})),
             "layer-parity %-34s %10s %10s %7s %10s  %-8s %s" % ("tap", "err", "e32", "ratio", "limit", "form", "worst at")]
    first = None
    for name in ref.names:
        r = _measure(got[name], ref.f64[name])
        if isinstance(r, str):
            table.append("layer-parity %-34s %s" % (name, r))
            first = first or "%s: %s" % (name, r)
            continue
        err, idx = r
        lim = ref.limit(name, prec)
        over = err > lim
        table.append("layer-parity %-34s %10.3e %10.3e %7.2f %10.3e  %-8s %s%s"
                     % (name, err, ref.e32[name], err / max(ref.e32[name], R.E32_MIN), lim, form[name], idx, "  <-- OVER" if over else ""))
        if over and first is None:
            first = "%s: err %.3e of range > limit %.3e (%s form), worst element %s" % (name, err, lim, form[name], idx)
    text = "\n".join(table)
    print("\n" + text)
    if first is not None:
        problems.insert(0, "first layer over its limit, in network order -- " + first)
    assert not problems, "\n".join(problems) + "\n" + text
