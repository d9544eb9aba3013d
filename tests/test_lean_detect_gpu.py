"""cp_model_detect_lean: the regression heads evaluated at the decoded peaks only.

Tolerance T(head) between a lean (pixel-list kernel) and a dense (halo kernel) value of one head entry: 2e-5 * max(1, max|head|),
the bound test_fused_head_matches_unfused_path already accepts between the halo form and the per-tap implicit-GEMM form of the
same fused head (same products, another float32 summation order) -- the pixel-list kernel IS the per-tap form.  Beyond the
summation order only the second product's per-wave power-of-two pre-scale differs (a wave of listed rows holds other pixels than
a wave of a dense tile), which moves last bits of hidden values that are tiny beside their wave's maximum.

Run with -s to see the measured figures (profiles/lean_detect_parity.txt holds those of the recorded run)."""
import sys
from collections import OrderedDict

import pytest
import torch

from centerpose_amd import hip, synth

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
REG = lambda heads: [k for k in heads if k not in ("hm", "hm_hp")]


def T(dense):
    return 2e-5 * max(1.0, float(dense.abs().max()))


def _gather_tables(z, pk_ind):
    """Exact copies of the dense maps' entries at the peaks, in the compact layouts of cp_decode_gathered."""
    B, _, K = pk_ind.shape
    out = {}
    for k, v in z.items():
        if k in ("hm", "hm_hp"):
            continue
        flat = v.reshape(B, v.shape[1], -1)
        if k == "hp_offset":
            idx = pk_ind[:, 1:].long()                                              # [B,8,K]
            out[k] = torch.stack([torch.gather(flat[:, c].unsqueeze(1).expand(B, 8, -1), 2, idx) for c in range(2)], 2).contiguous()
        else:
            idx = pk_ind[:, 0].long().unsqueeze(1).expand(B, v.shape[1], K)
            out[k] = torch.gather(flat, 2, idx).contiguous()
    return out


def _random_heads(B, H, W, device, track, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda c, lo, hi: (torch.rand(B, c, H, W, generator=g) * (hi - lo) + lo).to(device)
    z = OrderedDict(hm=(torch.rand(B, 1, H, W, generator=g) ** 8).to(device), hm_hp=(torch.rand(B, 8, H, W, generator=g) ** 4).to(device),
                    hps=(torch.randn(B, 16, H, W, generator=g) * 5).to(device), wh=r(2, 5, 35), reg=r(2, 0, 1), hp_offset=r(2, 0, 1),
                    scale=r(3, 0.5, 1.5))
    if track:
        z.update(hps_uncertainty=r(16, -2, 2), scale_uncertainty=r(3, -2, 2), tracking=r(2, -3, 3), tracking_hp=r(16, -3, 3))
    return z


@pytest.mark.parametrize("grid", [(32, 32), (128, 256), (136, 256)])   # one-kernel peaks (4 / 8 keys per lane) and the tiled form
@pytest.mark.parametrize("track", [False, True])
def test_decode_halves_on_exact_tables_are_bit_equal_to_the_dense_decode(device, grid, track):
    H, W = grid
    z = _random_heads(2, H, W, device, track, 11 + H)
    dense = hip.decode_raw if H * W <= 32768 else hip.decode_raw_tiled
    for rep_mode in (0, 1):
        for fit in (False, True):
            pk_score, pk_ind = hip.decode_peaks(z["hm"], z["hm_hp"], K=100)
            t = _gather_tables(z, pk_ind)
            det = hip.decode_gathered(z["hm_hp"], pk_score, pk_ind, t["hps"], t["wh"], t.get("hps_uncertainty"), t["scale"],
                                      t.get("scale_uncertainty"), t["reg"], t["hp_offset"], t.get("tracking"), t.get("tracking_hp"),
                                      rep_mode=rep_mode, fit_gaussian=fit)
            ref = dense(z["hm"], z["hps"], z["wh"], z["hm_hp"], z.get("hps_uncertainty"), z["scale"], z.get("scale_uncertainty"),
                        z["reg"], z["hp_offset"], z.get("tracking"), z.get("tracking_hp"), K=100, rep_mode=rep_mode, fit_gaussian=fit)
            assert torch.equal(det, ref), (grid, track, rep_mode, fit)
    # without the optional heads (+0.5 / zero-fill rules)
    det = hip.decode_gathered(z["hm_hp"], pk_score, pk_ind, t["hps"], t["wh"])
    assert torch.equal(det, dense(z["hm"], z["hps"], z["wh"], z["hm_hp"], K=100))


@pytest.fixture(scope="module")
def dla(device):
    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("dla_34", heads)
    return heads, sd, hip.HipModel("dla_34", heads, sd, precision="f16x3")


def test_heads_at_borders_duplicates_and_short_lists(device, dla):
    heads, _, model = dla
    x = synth.frames(8, seed=53, h=256, w=256).to(device)
    G = 64
    assert model.lean_supported(8, 256, 256)
    assert not model.lean_supported(1, 512, 512) and model.lean_supported(2, 512, 512)   # small calls keep the dense path
    z = {k: v.clone() for k, v in model(x, sigmoid_hm=True).items()}
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        model.detect(x, graph=False)
        corners = [0, G - 1, (G - 1) * G, G * G - 1]
        border = list(range(1, G - 1, 7)) + [r * G for r in range(1, G - 1, 9)] + [r * G + G - 1 for r in range(2, G - 1, 9)] + \
            [(G - 1) * G + c for c in range(3, G - 1, 11)]
        inner = [17 * G + 23, 40 * G + 5]
        lists = {"short": corners + [inner[0]] * 3,                                  # 7 rows: less than one tile, a triple
                 "long": corners + border + inner + [inner[1]] * 70 + corners}       # duplicates across waves of 32 rows and tiles
        for name, l in lists.items():
            idx = torch.tensor([l if b % 2 == 0 else l[::-1] for b in range(8)], dtype=torch.int32, device=device)
            t = model.heads_at(idx)
            side.synchronize()
            for k in REG(heads):
                want = torch.gather(z[k].reshape(8, heads[k], -1), 2, idx.long().unsqueeze(1).expand(8, heads[k], -1))
                err = float((t[k] - want).abs().max())
                print("heads_at %-5s %-9s max|lean - dense| %.3e  T %.3e" % (name, k, err, T(z[k])))
                assert err <= T(z[k]), (name, k, err)
                # the same pixel listed twice: bit-equal inside one wave (32 consecutive rows), within T across waves
                tc = t[k].cpu()
                for b in range(3):
                    li = idx[b].tolist()
                    for i in range(len(li)):
                        for j in range(i + 1, len(li)):
                            if li[i] == li[j]:
                                d = float((tc[b, :, i] - tc[b, :, j]).abs().max())
                                m0, m1 = b * len(li) + i, b * len(li) + j
                                assert d == 0.0 if m0 // 32 == m1 // 32 else d <= T(z[k]), (name, k, b, i, j, d)


def _field_tolerances(Th):
    """Per record field: (absolute tolerance, float32 roundings at the field's magnitude).  A field is a gathered value or one
    or two __fadd_rn / __fsub_rn of gathered values with an integer pixel coordinate (decode.hip: assoc_kernel)."""
    g = lambda k: Th.get(k, 0.0)
    tol = {"bboxes": (g("reg") + g("wh") / 2, 2), "scores": (0.0, 0), "clses": (0.0, 0),
           "kps": (max(g("hps"), g("hp_offset")), 1), "obj_scale": (g("scale"), 0),
           "kps_displacement_mean": (g("hps"), 1), "kps_heatmap_mean": (g("hp_offset"), 3),
           "kps_heatmap_std": (0.0, 0), "kps_heatmap_height": (0.0, 0),
           # sqrt(exp(v)) [* balance]: d/dv = field / 2
           "obj_scale_uncertainty": (None, 4), "kps_displacement_std": (None, 4),
           "tracking": (g("tracking"), 0), "tracking_hp": (g("tracking_hp"), 0)}
    return tol


def _flipped_records(a, b, Th):
    """Records of a / b [B,K,118] in which some field differs by more than its tolerance (a discrete decision flipped:
    nearest candidate, reject / filter mask, or -- between arithmetic modes -- the peak itself)."""
    bad = torch.zeros(a.shape[:2], dtype=torch.bool, device=a.device)
    ra, rb = hip.split_detections(a), hip.split_detections(b)
    for k, (t, nr) in _field_tolerances(Th).items():
        va, vb = ra[k], rb[k]
        mag = torch.maximum(va.abs(), vb.abs())
        if t is None:
            head = "scale_uncertainty" if k == "obj_scale_uncertainty" else "hps_uncertainty"
            lim = Th.get(head, 0.0) * 0.5 * mag + nr * EPS * mag
        else:
            lim = t + nr * EPS * mag
        bad |= ((va - vb).abs() > lim).any(-1)
    return int(bad.sum())


def _parity_of(model, model32, x, heads, label, **kw):
    """The compact tables at the peaks, the records and the lazy maps of one model and batch (kw: detect's pre_* inputs and
    decode options); prints the measured figures."""
    side = torch.cuda.Stream(device=x.device)
    pre = {k: v for k, v in kw.items() if k.startswith("pre_")}
    z = {k: v.clone() for k, v in model(x, sigmoid_hm=True, **pre).items()}
    z32 = model32(x, sigmoid_hm=True, **pre)
    with torch.cuda.stream(side):
        _, det32 = model32.detect(x, graph=False, heads="dense", **kw)
        det32 = det32.clone()
        _, det_dense = model.detect(x, graph=False, heads="dense", **kw)
        det_dense = det_dense.clone()
        outs, det = model.detect(x, graph=False, **kw)
        side.synchronize()
        assert isinstance(outs, hip.LazyHeads) and not outs.materialised() and list(outs) == list(heads)
        exact = _gather_tables(z, outs.pk_ind)
        exact32 = _gather_tables(z32, outs.pk_ind)
        Th = {}
        for k in REG(heads):
            Th[k] = T(z[k])
            d = (outs.gathered[k] - exact[k]).abs()
            same = float((outs.gathered[k] == exact[k]).float().mean())
            d32 = float((exact[k] - exact32[k]).abs().max())
            print("%s table %-9s max|lean - dense| %.3e  bit-identical %.4f  T %.3e  max|dense f16x3 - dense f32| %.3e"
                  % (label, k, float(d.max()), same, Th[k], d32))
            assert float(d.max()) <= Th[k], (k, float(d.max()))
        r, rd = hip.split_detections(det), hip.split_detections(det_dense)
        assert torch.equal(r["scores"], rd["scores"]) and torch.equal(r["clses"], rd["clses"])
        n_lean = _flipped_records(det, det_dense, Th)
        n_yard = _flipped_records(det_dense, det32, Th)
        print("%s records %d: flipped lean vs dense %d, flipped dense f16x3 vs dense f32 (yardstick) %d"
              % (label, det.shape[0] * det.shape[1], n_lean, n_yard))
        assert n_lean <= n_yard, (n_lean, n_yard)
        for k in heads:                          # lazy maps == forward's, bit for bit
            assert torch.equal(outs[k], z[k]), k
        assert outs.materialised()
        stale, _ = model.detect(x, graph=False, **kw)
        model.detect(x, graph=False, **kw)
        side.synchronize()
        assert stale["hm"].shape == z["hm"].shape
        with pytest.raises(RuntimeError, match="next detect"):
            stale["wh"]
    sys.stdout.flush()


def test_lean_detect_small_dla(device, dla):
    heads, sd, model = dla
    model32 = hip.HipModel("dla_34", heads, sd, precision="f32")
    assert not model32.lean_supported(8, 256, 256)
    x = synth.frames(8, seed=59, h=256, w=256).to(device)
    _parity_of(model, model32, x, heads, "dla_34 B=8 256x256")
    # below the engine's size threshold "lazy" is the dense call: a plain dict, every map there
    x1 = synth.frames(1, seed=60, h=256, w=256).to(device)
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        outs, det = model.detect(x1, graph=False)
        side.synchronize()
    assert not isinstance(outs, hip.LazyHeads) and list(outs) == list(heads)
    z1 = model(x1, sigmoid_hm=True)
    for k in heads:
        assert torch.equal(outs[k], z1[k]), k


def test_lean_detect_on_the_bench_pipeline(device):
    import bench

    pipe = bench.Pipeline("full", 64, device, seed=317, precision="f16x3")
    assert pipe.model.lean_supported(64, 512, 512)
    sd = synth.make_state_dict(pipe.arch, pipe.heads, False)
    model32 = hip.HipModel(pipe.arch, pipe.heads, sd, precision="f32")
    _parity_of(pipe.model, model32, pipe.x, pipe.heads, "bench full B=64 512x512")


def test_lean_detect_hourglass(device):
    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("hourglass", heads)
    model = hip.HipModel("hourglass", heads, sd, precision="f16x3")
    model32 = hip.HipModel("hourglass", heads, sd, precision="f32")
    x = torch.cat([synth.frames(8, seed=317 + i) for i in range(0, 16, 8)]).to(device)
    assert model.lean_supported(16, 512, 512)
    _parity_of(model, model32, x, heads, "hourglass B=16 512x512")


def test_lean_detect_tracking_heads_and_profile(device):
    """dla_34 with the tracking heads (previous-frame stems, HEADS_TRACK): eight centre-indexed heads in the grouped launch; and
    the profile names the pixel-list kernel with the FLOPs it executes."""
    heads = synth.HEADS_TRACK
    sd = synth.make_state_dict("dla_34", heads, True)
    model = hip.HipModel("dla_34", heads, sd, tracking_task=True, precision="f16x3")
    x = synth.frames(8, seed=61, h=256, w=256).to(device)
    g = torch.Generator(device="cpu").manual_seed(5)
    pre = dict(pre_img=synth.frames(8, seed=62, h=256, w=256).to(device),
               pre_hm=(torch.rand(8, 1, 256, 256, generator=g) ** 16).to(device),
               pre_hm_hp=(torch.rand(8, 8, 256, 256, generator=g) ** 16).to(device))
    model32 = hip.HipModel("dla_34", heads, sd, tracking_task=True, precision="f32")
    _parity_of(model, model32, x, heads, "dla_34 tracking B=8 256x256", fit_gaussian=True, **pre)
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        model.profile(True)
        model.detect(x, fit_gaussian=True, graph=False, **pre)
        side.synchronize()
        prof = model.profile_read()
        model.profile(False)
    rows = prof["igemm16_head_rows_f16x3_m128n128"]
    assert rows["launches"] == 2
    K, hid, c2 = 100, 256, sum(c for k, c in heads.items() if k not in ("hm", "hm_hp", "hp_offset"))
    M = 8 * K   # rows of the centre list: batch x K
    want = 2.0 * M * (8 * hid) * 576 + 2.0 * M * c2 * hid + 2.0 * (8 * M) * hid * 576 + 2.0 * (8 * M) * 2 * hid
    assert abs(rows["flops"] - want) <= 1e-9 * want


def test_lean_detect_graph_replay(device, dla):
    heads, _, model = dla
    x = synth.frames(8, seed=67, h=256, w=256).to(device)
    x2 = synth.frames(8, seed=68, h=256, w=256).to(device)
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        eager = model.detect(x, graph=False)[1].clone()
        outs, det = model.detect(x, graph=True)            # capture + first replay
        side.synchronize()
        assert torch.equal(det, eager)
        z1 = model(x, sigmoid_hm=True)
        for k in heads:
            assert torch.equal(outs[k], z1[k]), k
        eager2 = model.detect(x2, graph=False)[1].clone()
        x.copy_(x2)                                        # new frames into the captured input
        outs, det = model.detect(x, graph=True)            # pure replay
        side.synchronize()
        assert torch.equal(det, eager2)
        z2 = model(x2, sigmoid_hm=True)
        for k in heads:                                    # the replayed call's feature map serves the lazy maps too
            assert torch.equal(outs[k], z2[k]), k
