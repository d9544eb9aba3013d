"""resdcn_N on the device: the dense deconv kernel (deconv16.hip) against torch in float64, the whole network against
the reference module's golden and a torch-CPU restatement, determinism, and the detector with --arch resdcn_18."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centerpose_amd import hip, synth
from tests.resdcn_ref import torch_resdcn_forward as _torch_resdcn_forward

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(params=["f32", "f16x3"])
def prec(request):
    hip.set_default_precision(request.param)
    yield request.param
    hip.set_default_precision("f32")


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 7, 9, 64, 64), (3, 5, 12, 128, 128), (1, 16, 11, 256, 256),
                                            (3, 4, 5, 2048, 256), (1, 3, 3, 64, 96)])
@pytest.mark.parametrize("affine", [False, True])
def test_conv_transpose2d_vs_torch(device, prec, B, H, W, Cin, Cout, affine):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cin, Cout, 4, 4, generator=g) / (2.0 * Cin ** 0.5)
    ref = F.conv_transpose2d(x.double(), w.double(), None, stride=2, padding=1)
    scale = shift = None
    if affine:
        scale = torch.rand(Cout, generator=g) + 0.5
        shift = torch.randn(Cout, generator=g) * 0.1
        ref = torch.relu(ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    out = hip.conv_transpose2d(x.permute(0, 2, 3, 1).contiguous().to(device), w.to(device),
                               None if scale is None else scale.to(device), None if shift is None else shift.to(device),
                               act=1 if affine else 0)
    o = out.permute(0, 3, 1, 2).cpu().double()
    assert o.shape == ref.shape
    err = float((o - ref).abs().max() / ref.abs().max())
    assert err < 1e-5, err  # float32 accumulation over K = 4 * Cin (up to 8192 terms)


@pytest.mark.parametrize("xmag", [1e-5, 1e-3, 1e3, 1e5])
@pytest.mark.parametrize("wmag", [1e-4, 1e-2])
def test_f16x3_deconv_is_range_safe(device, xmag, wmag):
    hip.set_default_precision("f16x3")
    try:
        g = torch.Generator().manual_seed(91)
        x = torch.randn(2, 64, 10, 12, generator=g) * xmag
        w = torch.randn(64, 128, 4, 4, generator=g) * wmag
        ref = F.conv_transpose2d(x.double(), w.double(), None, stride=2, padding=1)
        out = hip.conv_transpose2d(x.permute(0, 2, 3, 1).contiguous().to(device), w.to(device))
        err = float((out.permute(0, 3, 1, 2).cpu().double() - ref).abs().max() / ref.abs().max())
        assert err < 2e-5, err
    finally:
        hip.set_default_precision("f32")


@pytest.mark.parametrize("depth", [18, 101])
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_resdcn_vs_reference_golden(device, depth, precision):
    """Engine vs the reference PoseResNet's own output on the seeded weights (tools/make_resdcn_goldens.py)."""
    heads = synth.HEADS_POSE
    gold = np.load(os.path.join(GOLD, "backbone_resdcn_%d.npz" % depth))
    sd = synth.make_state_dict("resdcn_%d" % depth, heads)
    assert synth.abs_checksum(sd) == float(gold["_weights_checksum"])
    x = torch.from_numpy(gold["x"])
    model = hip.HipModel("resdcn_%d" % depth, heads, sd, head_conv=64, precision=precision)
    z = model(x.to(device))
    for k in heads:
        ref = torch.from_numpy(gold["head_" + k])
        err = float((z[k].cpu() - ref).abs().max())
        assert err < 1e-3 * max(1.0, float(ref.abs().max())), (k, err)
    hm = torch.sigmoid(z["hm"].cpu())
    assert float((hm - torch.sigmoid(torch.from_numpy(gold["head_hm"]))).abs().max()) < 1e-3
    # the taps place a failure: backbone (layer4), first DCN + deconv stage (deconv_layers.5), last stage (.17)
    for tap in ("layer4", "deconv_layers.2", "deconv_layers.5", "deconv_layers.17"):
        ref = torch.from_numpy(gold["tap_" + tap])
        _, t = model.forward(x.to(device), tap=tap)
        assert t.shape == ref.shape, tap
        err = float((t.cpu() - ref).abs().max())
        assert err < 1e-3 * max(1.0, float(ref.abs().max())), (tap, err)


def test_resdcn_18_512_batch_vs_torch_cpu(device):
    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("resdcn_18", heads)
    x = synth.frames(8, seed=11, h=512, w=512)
    nthreads = torch.get_num_threads()
    torch.set_num_threads(16)
    try:
        with torch.no_grad():
            ref = _torch_resdcn_forward(sd, x, 18, heads)
    finally:
        torch.set_num_threads(nthreads)  # process-global: later tests see the setting they started with
    for precision in ("f32", "f16x3"):
        model = hip.HipModel("resdcn_18", heads, sd, head_conv=64, precision=precision)
        z = model(x.to(device))
        for k in heads:
            err = float((z[k].cpu() - ref[k]).abs().max())
            assert err < 1e-3 * max(1.0, float(ref[k].abs().max())), (precision, k, err)


def test_resdcn_18_batch64_deterministic_and_size_checks(device):
    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("resdcn_18", heads)
    model = hip.HipModel("resdcn_18", heads, sd, head_conv=64, precision="f16x3")
    x = synth.frames(64, seed=5, h=256, w=256).to(device)
    a = {k: v.clone() for k, v in model(x).items()}
    b = model(x)
    for k in heads:
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(RuntimeError):
        model(synth.frames(1, seed=1, h=200, w=200).to(device))  # not a multiple of 32


def test_detector_run_and_run_batch_resdcn_18(device, tmp_path):
    """--arch resdcn_18 through opts -> create_model -> load_model -> ObjectPoseDetector: the DLA output schema, and
    run_batch equals run by value."""
    from centerpose_amd.lib.detectors.detector_factory import detector_factory
    from centerpose_amd.lib.models.model import create_model, save_model
    from centerpose_amd.lib.opts import opts
    from tests import scene

    o = opts().parser.parse_args(["--arch", "resdcn_18", "--c", "cup", "--debug", "5"])
    o.nms = True
    o.obj_scale = True
    o.use_pnp = True
    opt = opts().init(opts().parse(o))
    assert opt.head_conv == 64
    sd = synth.make_state_dict("resdcn_18", opt.heads)
    ck = os.path.join(str(tmp_path), "synthetic_resdcn_18.pth")
    m = create_model(opt.arch, opt.heads, opt.head_conv, opt)
    m.load_state_dict(sd, strict=True)
    save_model(ck, 7, m)
    opt.load_model = ck
    det = detector_factory[opt.task](opt)
    rng = np.random.RandomState(0)
    meta_inp = {"camera_matrix": scene.K_DEMO}
    img = rng.randint(0, 255, (480, 640, 3)).astype(np.uint8)
    img2 = rng.randint(0, 255, (480, 640, 3)).astype(np.uint8)
    ret = det.run(img, meta_inp=meta_inp)
    assert set(ret) == {"results", "boxes", "output", "tot", "load", "pre", "net", "dec", "post", "merge", "pnp", "track"}
    assert set(ret["output"]) >= set(opt.heads)
    r2 = det.run(img2, meta_inp=meta_inp)
    images, meta = det.pre_process(img, 1.0, meta_inp)
    i2, m2 = det.pre_process(img2, 1.0, meta_inp)
    outs = det.run_batch(torch.cat([images, i2]), [meta, m2])
    for single, batched in ((ret, outs[0]), (r2, outs[1])):
        assert len(single["results"]) == len(batched["results"])
        for a, b in zip(single["results"], batched["results"]):
            np.testing.assert_allclose(a["bbox"], b["bbox"], atol=1e-3)
            assert abs(a["score"] - b["score"]) < 1e-5
