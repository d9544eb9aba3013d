"""GPU tests of the training input images (centerpose_amd/train_inputs.py, cp_train_inputs): every case of
tests/train_input_cases.py against the numpy restatement (bit for bit without colour) and the host build of
train_inputs_common.h (bit for bit with colour, fed the device's own grey means), reproducibility and independence of
the images of a call, the inference warp as the special case, reads confined to each frame, and the tracking task's
2B-frame call."""
import numpy as np
import pytest
import torch

from centerpose_amd import hip
from centerpose_amd.train_inputs import MEAN, STD, TrainInputs, pack_frames, split_tracking
from tests import train_input_cases as TC
from tests import train_inputs_ref as R
from tests.test_train_inputs_cpu import COLOR_TOL, bits

pytestmark = pytest.mark.gpu
I = hip.TI_IMG


def _ti(side):
    return TrainInputs(TC.SimpleNamespace(new_data_augmentation=False, input_res=side))


def _run(frames, recs, side, device):
    out, means = _ti(side)(frames, recs, device=device, return_means=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), means.cpu().numpy()


@pytest.mark.parametrize("name", sorted(TC.BATCHES))
def test_device_equals_restatement_and_host_build(device, name):
    frames, recs, side = TC.batch(name)
    out, means = _run(frames, recs, side, device)
    assert out.shape == (5, 3, side, side) and out.dtype == np.float32
    f32, f64 = R.batch(frames, recs, side, "f32"), R.batch(frames, recs, side, "f64")
    host, _ = TC.host_batch(frames, recs, side, gs_means=means)
    for n in range(5):
        if recs[n, I["color"]]:
            gs_mean = R.grey(R.warp_u8(frames[n], recs[n], side).astype(np.float64) / 255.).mean()
            err = np.abs(out[n] - f64[n]).max()
            print("%s/%d colour: gs_mean %.9g (float64 %.9g), %.3g against the float64 restatement"
                  % (name, n, means[n], gs_mean, err))
            # a float32 grey value below 1 carries five roundings of at most 2^-24 each (the division, the coefficient,
            # the product, two sums); the float64 sum adds nothing visible and the final float32 rounding half an ulp
            assert abs(float(means[n]) - gs_mean) <= 6 * 2.0 ** -24
            assert np.array_equal(bits(out[n]), bits(host[n])), n
            assert err < COLOR_TOL, (n, err)
        else:
            assert means[n] == 0
            assert np.array_equal(bits(out[n]), bits(f32[n])), n


@pytest.mark.parametrize("name", ["mixed48", "odd35"])
def test_reproducible_and_independent_of_the_batch(device, name):
    frames, recs, side = TC.batch(name)
    a, ma = _run(frames, recs, side, device)
    b, mb = _run(frames, recs, side, device)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(ma), bits(mb))
    for n in range(5):  # the per-image offset, record and grey-mean indexing
        one, m1 = _run(frames[n:n + 1], recs[n:n + 1], side, device)
        assert np.array_equal(bits(one[0]), bits(a[n])) and bits(m1)[0] == bits(ma)[n], n


def test_inference_warp_is_the_special_case(device):
    side, (h, w) = 36, TC.SIZES["a"]
    frames = torch.from_numpy(np.stack([TC.frame("a", 900 + n) for n in range(3)]))
    trans = TC.transform("rot+30", "a", side, False)
    recs = np.stack([TC.pack_input(trans, h, w, False)["ti_image"]] * 3)
    out = _ti(side)(frames.to(device), recs)
    ref = hip.preprocess_batch(frames.to(device), trans, MEAN, STD, side, side)
    torch.cuda.synchronize()
    assert out.device.type == "cuda" and out.shape == ref.shape

    def levels(t):  # un-normalise and round: 1 / 255 apart, against errors of a few float32 ulps
        v = (t.cpu().numpy().astype(np.float64) * STD[None, :, None, None] + MEAN[None, :, None, None]) * 255.
        assert np.abs(v - np.rint(v)).max() < 1e-3
        return np.rint(v).astype(np.int64)

    lv = levels(out)
    assert np.array_equal(lv, levels(ref))
    assert np.array_equal(lv[1].transpose(1, 2, 0), R.warp_u8(frames[1].numpy(), recs[1], side))
    assert lv.min() == 0 and lv.max() > 200  # border and image are both in view


@pytest.mark.parametrize("name", ["border48", "mixed48"])
def test_no_reads_outside_a_frame(device, name):
    """255-filled guard bands between (and around) the frames against a tight packing: a tap read outside its frame
    would show in the border-heavy and singular images, whose border must stay the constant 0."""
    frames, recs, side = TC.batch(name)
    band = 4096
    tight, guarded = recs.copy(), recs.copy()
    tight[:, I["offset"]] = np.cumsum([0] + [f.size for f in frames[:-1]])
    guarded[:, I["offset"]] = tight[:, I["offset"]] + band * (1 + np.arange(5))
    outs = []
    for r in (tight, guarded):
        buf = np.full(int(r[-1, I["offset"]]) + frames[-1].size + (band if r is guarded else 0), 255, np.uint8)
        for n, f in enumerate(frames):
            o = int(r[n, I["offset"]])
            buf[o:o + f.size] = f.reshape(-1)
        out = torch.empty(5, 3, side, side, dtype=torch.float32, device=device)
        hip.train_inputs(torch.from_numpy(buf).to(device), r, MEAN, STD, out)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    ref, _ = _run(frames, recs, side, device)  # and both equal the aligned packing of TrainInputs
    assert np.array_equal(bits(outs[0]), bits(ref))


def test_tracking_task_halves(device):
    cur, rc, side = TC.batch("geometry36")
    pre, rp, _ = TC.batch("orders36")
    both, _ = _run(cur + pre, np.concatenate([rc, rp]), side, device)
    halves = split_tracking(torch.from_numpy(both))
    assert sorted(halves) == ["input", "pre_img"] and halves["input"].shape == (5, 3, side, side)
    a, _ = _run(cur, rc, side, device)
    b, _ = _run(pre, rp, side, device)
    assert np.array_equal(bits(halves["input"].numpy()), bits(a))
    assert np.array_equal(bits(halves["pre_img"].numpy()), bits(b))


def test_refused_before_any_launch(device):
    frames, recs, side = TC.batch("geometry36")
    buf, packed = pack_frames(frames, recs)
    packed[4, I["order"]] = 7
    out = torch.empty(5, 3, side, side, dtype=torch.float32, device=device)
    with pytest.raises(ValueError, match="order code 7"):
        hip.train_inputs(buf.to(device), packed, MEAN, STD, out)
    packed[4, I["order"]] = 0
    with pytest.raises(ValueError, match="outside the frames buffer"):
        hip.train_inputs(buf[:-FRAME_TAIL].to(device), packed, MEAN, STD, out)


def e2e_batch():
    """Two decoded frames of differing sizes with annotations, as a dataset following INTEGRATION.md's example returns
    them: (frames, collated records, target opt).  64 x 64 input, 16 x 16 output."""
    from centerpose_amd.pose_targets import pack_annotations
    from centerpose_amd.train_inputs import draw_color_aug
    from tests import pose_target_cases as PC

    frames, recs, topt = [], [], None
    for seed, flipped in ((21, False), (22, True)):  # 480 x 640 and 640 x 480 (width x height)
        topt, anns, w, h, _ = PC.random_case(seed, "chair", n_obj=4, output_res=16, input_res=64, center_3D=False,
                                             use_absolute_scale=False, hps_uncertainty=False, obj_scale_uncertainty=False)
        rng = np.random.RandomState(seed)
        c = np.array([w / 2., h / 2.], dtype=np.float32)
        if flipped:
            c[0] = w - c[0] - 1
        s = max(h, w) * 1.0
        rec = pack_annotations(anns, TC.get_affine_transform(c, s, 0, [16, 16]), w, h, flipped, 0.0, topt)
        rec.update(TC.pack_input(TC.get_affine_transform(c, s, 0, [64, 64]), h, w, flipped, draw_color_aug(rng)))
        frames.append(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        recs.append(rec)
    return frames, {k: torch.from_numpy(np.stack([r[k] for r in recs])) for k in recs[0]}, topt


def test_training_step_from_decoded_frames(device):
    """Decoded frames + records -> TrainInputs, PoseTargets -> PoseNet -> ObjectPoseLoss -> backward: input, targets and
    loss all produced on the device."""
    from centerpose_amd import synth
    from centerpose_amd.pose_loss import ObjectPoseLoss
    from centerpose_amd.pose_net import PoseNet
    from centerpose_amd.pose_targets import PoseTargets
    from tests import pose_loss_cases as PLC
    from tests import pose_net_ref as NR

    hip.set_default_precision("f32")
    frames, records, topt = e2e_batch()
    assert frames[0].shape != frames[1].shape
    images = TrainInputs(topt)(frames, records["ti_image"], device=device)
    batch = PoseTargets(topt)(records)
    assert images.shape == (2, 3, 64, 64) and int(batch["reg_mask"].sum()) > 0
    ref = R.batch(frames, records["ti_image"].numpy(), 64, "f64")
    assert np.abs(images.cpu().numpy() - ref).max() < COLOR_TOL
    net = PoseNet(synth.HEADS_POSE, head_conv=NR.HEAD_CONV,
                  opt=TC.SimpleNamespace(pre_img=False, pre_hm=False, pre_hm_hp=False))
    net.load_state_dict(NR.case_state_dict(False), strict=True)
    net = net.to(device).train()
    out = [{h: v.clone(memory_format=torch.contiguous_format) for h, v in z.items()} for z in net(images)]
    loss, stats, _ = ObjectPoseLoss(PLC.make_opt({}))(out, batch, "train")
    loss.backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and float(loss) > 0
    grads = {n: p.grad for n, p in net.named_parameters()}
    missing = [n for n, g in grads.items() if g is None]
    assert all(NR.unused(n) for n in missing), missing  # dla_34's two projections that its graph never reaches
    assert not [n for n, g in grads.items() if g is not None and not torch.isfinite(g).all()]
    stem = next(iter(grads))  # the first convolution, which reads the device-built input
    assert stem.startswith("base.base_layer.0") and float(grads[stem].abs().max()) > 0


FRAME_TAIL = 512  # cuts into the last frame of geometry36 (37 x 53 x 3 bytes, padded to a multiple of 256)
