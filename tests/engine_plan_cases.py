"""The cases of tests/golden/engine_plan_pins.json and how one is recorded: shared by tools/make_engine_plan_pins.py (which writes
the fixture) and tests/test_engine_plan_pins_gpu.py (which replays it).

A pin holds what the engine's host code decides for one (model, precision, shape, switches, tap) -- the ordered launch rows, the
per-variant launch / FLOP / byte totals, the work-space query's answer, the peak a real pass reached and the stand-alone maxpool2
launches -- and a SHA-256 of every tensor the pass returns.  Shapes are the smallest at which each decision is live; the epilogue
tests (test_upadd_epilogue_gpu, test_idaup_boundary_gpu, test_project_epilogue_gpu, test_pooled_store_gpu) say why each triggers
what."""
import hashlib
import os
import tempfile
from collections import OrderedDict

import torch

from centerpose_amd import hip, synth

S = hip.KernelSel
DCN = S.DCN16P_ALWAYS | S.DCN16T_ALWAYS  # the IDAUp sites fuse at the small shapes as well

# model key -> (arch, heads, tracking, HipModel keywords)
MODELS = OrderedDict([
    ("dla_34", ("dla_34", synth.HEADS_POSE, False, {})),
    ("dlav1_34_track", ("dlav1_34", synth.HEADS_TRACK, True, {})),
    ("dlav1_34", ("dlav1_34", synth.HEADS_POSE, False, {})),
    ("hourglass", ("hourglass", synth.HEADS_POSE, False, {})),
    ("resdcn_18", ("resdcn_18", synth.HEADS_POSE, False, dict(head_conv=64))),
])

# (model key, precision, (B, H, W), switches, tap or None, call)
CASES = [
    # three up-add sites and one fused projection; all three IDAUp forms; the unfused-entry form
    ("dla_34", "f16x3", (2, 256, 512), 0, None, "forward"),
    ("dla_34", "f16x3", (2, 256, 512), DCN, None, "forward"),
    ("dla_34", "f16x3", (2, 256, 512), DCN, "ida_up.node_1", "forward"),
    ("dla_34", "f16x3", (2, 256, 512), DCN, "dla_up.ida_2.node_3", "forward"),
    ("dla_34", "f16x3", (2, 256, 512), DCN, "base.level2.project", "forward"),
    # pooled copy from level1 and level2's Root; four maxpool2 launches
    ("dla_34", "f16x3", (4, 256, 256), S.LEVEL1_ROWS_ALWAYS, None, "forward"),
    ("dla_34", "f16x3", (4, 256, 256), S.PW16_FRAG_A | S.LEVEL1_ROWS_NEVER, None, "forward"),
    # split-K and 64 x 64-tile plans; the float32 path
    ("dla_34", "f16x3", (1, 128, 128), 0, None, "forward"),
    ("dla_34", "f16x3", (1, 128, 128), S.NO_LOWC, None, "forward"),
    ("dla_34", "f16x3", (1, 128, 128), S.STEM_LEVEL0_UNFUSED, None, "forward"),
    ("dla_34", "f32", (1, 128, 128), 0, None, "forward"),
    # the lean head stage, which starts at 32768 output pixels
    ("dla_34", "f16x3", (2, 512, 512), 0, None, "detect"),
    # all three GroupNorm hook forms and the GRU role
    ("dlav1_34_track", "f16x3", (1, 128, 128), 0, None, "forward"),
    ("dlav1_34_track", "f16x3", (1, 128, 128), S.GN_HEAD_F32, None, "forward"),
    ("dlav1_34_track", "f16x3", (1, 128, 128), S.GN_HEAD_MFMA, None, "forward"),
    ("dlav1_34_track", "f16x3", (1, 128, 128), S.GRU_UNFUSED, None, "forward"),
    ("dlav1_34_track", "f32", (1, 128, 128), 0, None, "forward"),
    ("dlav1_34", "f16x3", (1, 128, 128), 0, None, "forward"),
    # role + NCHW-output call sites
    ("hourglass", "f16x3", (1, 128, 128), 0, None, "forward"),
    ("hourglass", "f16x3", (1, 128, 128), S.NO_HEAD_FUSION, None, "forward"),
    ("resdcn_18", "f16x3", (1, 128, 128), 0, None, "forward"),
    ("resdcn_18", "f16x3", (1, 128, 128), S.NO_HEAD_FUSION, None, "forward"),
]


def case_id(case):
    key, prec, (B, H, W), sel, tap, call = case
    return "%s-%s-%dx%dx%d-sel%08x-%s-%s" % (key, prec, B, H, W, int(sel), tap or "notap", call)


_models = {}


def model(key):
    """One HipModel per architecture (set_precision moves it between the arithmetic modes)."""
    if key not in _models:
        arch, heads, tracking, kw = MODELS[key]
        sd = synth.make_state_dict(arch, heads, tracking)
        _models[key] = hip.HipModel(arch, heads, sd, tracking_task=tracking, **kw)
    return _models[key]


def _inputs(key, B, H, W, device):
    x = synth.frames(B, seed=29, h=H, w=W).to(device)
    kw = {}
    if MODELS[key][2]:  # the tracking task: all three previous-frame inputs
        kw = dict(pre_img=synth.frames(B, seed=30, h=H, w=W).to(device),
                  pre_hm=(torch.rand(B, 1, H, W, generator=synth._gen(29, "pre_hm")) ** 8).to(device),
                  pre_hm_hp=(torch.rand(B, 8, H, W, generator=synth._gen(29, "pre_hm_hp")) ** 8).to(device))
    return x, kw


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _run(m, x, kw, tap, call):
    """-> {name: tensor} of what one pass returns"""
    if call == "detect":
        _, det = m.detect(x, graph=False, **kw)
        return {"det": det}
    if tap:
        outs, t = m.forward(x, tap=tap, **kw)
        return dict(outs, **{"tap:" + tap: t})
    return dict(m.forward(x, **kw))


def record(case, device, passes=1):
    """One case -> its pin (a JSON-ready dict).  The digests come from passes without profiling; `passes` > 1 repeats them and
    lists under "unstable" what differed between the repeats."""
    key, prec, (B, H, W), sel, tap, call = case
    m = model(key)
    m.set_precision(prec)
    x, kw = _inputs(key, B, H, W, device)
    pin = OrderedDict(id=case_id(case))
    with hip.select_kernels(sel):
        pin["workspace_bytes"] = m.workspace_bytes(B, H, W)
        digests = []
        for _ in range(passes):
            out = _run(m, x, kw, tap, call)
            torch.cuda.synchronize()
            digests.append(OrderedDict((k, _sha(v)) for k, v in out.items()))
        pin["digests"] = digests[0]
        unstable = sorted(k for k in digests[0] if any(d[k] != digests[0][k] for d in digests))
        if unstable:
            pin["unstable"] = unstable
        m.profile(True)
        _run(m, x, kw, tap, call)
        torch.cuda.synchronize()
        pin["workspace_used"] = m.workspace_used()
        pin["maxpool_launches"] = m.maxpool_launches()
        fd, dump = tempfile.mkstemp(suffix=".csv")
        os.close(fd)
        os.environ["CP_PROFILE_DUMP"] = dump  # per-launch rows: name, M, N, K, kh, stride, ms, TFLOP/s, role
        try:
            ran = m.profile_read()
        finally:
            del os.environ["CP_PROFILE_DUMP"]
            m.profile(False)
        rows = []
        with open(dump) as f:
            for line in f:
                name, M, N, K, kh, stride, _ms, _tf, role = line.strip().split(",")
                rows.append([name, int(M), int(N), int(K), int(kh), int(stride), role])
        os.remove(dump)
    pin["launch_rows"] = rows  # variant, M, N, K, kh, stride, role -- in launch order
    # (the doubles as hexadecimal literals: exact)
    pin["variants"] = OrderedDict((k, dict(launches=v["launches"], flops=float(v["flops"]).hex(), bytes=float(v["bytes"]).hex()))
                                  for k, v in ran.items())
    return pin
