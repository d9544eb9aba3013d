"""GPU tests of the ObjectPose training targets (centerpose_amd/pose_targets.py, cp_pose_targets): every golden case
against the reference-built arrays (tests/golden/pose_targets_ref.npz), seeded full-size batches against the host
restatement (tests/pose_targets_ref.py), reproducibility across streams, and ObjectPoseLoss on device-built targets
against the same loss on the reference-built ones."""
import numpy as np
import pytest
import torch

from centerpose_amd.pose_loss import ObjectPoseLoss
from centerpose_amd.pose_targets import PoseTargets, num_symmetry, pack_annotations, target_keys
from tests import pose_loss_cases as PLC
from tests import pose_target_cases as PC
from tests import pose_targets_ref as R
from tests.test_pose_targets_cpu import golden_arrays, random_records

pytestmark = pytest.mark.gpu
GOLD = np.load(__file__.rsplit("/", 1)[0] + "/golden/pose_targets_ref.npz")
MAPS = ("hm", "hm_hp")


def _records(names):
    return {"pt_image": torch.from_numpy(np.stack([GOLD[n + "/pt_image"] for n in names])),
            "pt_objects": torch.from_numpy(np.stack([GOLD[n + "/pt_objects"] for n in names]))}


def _compare(dev, ref, keys, where):
    """Integers and masks exactly; maps bit for bit or within one float32 ulp.  Returns the count of map elements that
    are not bit-identical."""
    differ = 0
    for k in keys:
        a = dev[k].cpu().numpy()
        b = ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (where, k, a.dtype, b.dtype, a.shape, b.shape)
        if k in MAPS:
            ne = a.view(np.int32) != b.view(np.int32)
            differ += int(ne.sum())
            assert np.all(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32)) <= 1), (where, k)
        else:
            assert np.array_equal(a, b), (where, k, np.argwhere(a != b)[:5])
    return differ


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_device_equals_goldens(device, name):
    opt = PC.make_opt(PC.CASES[name][1])
    out = PoseTargets(opt)(_records([name]))
    torch.cuda.synchronize()
    assert sorted(out) == sorted(target_keys(opt))
    differ = _compare(out, golden_arrays(GOLD, name, opt), target_keys(opt), name)
    print("%s: %d map elements not bit-identical to the reference" % (name, differ))
    assert differ == 0


@pytest.mark.parametrize("S, Rr", [(1, 128), (4, 128), (12, 128), (4, 96), (12, 96), (4, 75)])
def test_device_equals_restatement(device, S, Rr):
    cat = {1: "camera", 4: "chair", 12: "bottle"}[S]
    rng = np.random.default_rng(1000 * S + Rr)
    B = 32 if Rr != 75 else 6  # R = 75: R*R is odd, every plane after the first starts off a 16-byte boundary
    imgs, objs = random_records(rng, B, S, Rr, cat)
    for center_3D, abs_scale in ((False, False), (True, True)):
        opt = PC.make_opt(dict(c=cat, num_symmetry=S, output_res=Rr, center_3D=center_3D, use_absolute_scale=abs_scale,
                               hps_uncertainty=True, obj_scale_uncertainty=True))
        out = PoseTargets(opt)({"pt_image": torch.from_numpy(imgs), "pt_objects": torch.from_numpy(objs)})
        torch.cuda.synchronize()
        ref = R.batch_targets(imgs, objs, S, Rr, center_3D, abs_scale)
        differ = _compare(out, ref, target_keys(opt), (S, Rr, center_3D))
        print("S=%d R=%d center_3D=%d: %d map elements not bit-identical, %d objects kept"
              % (S, Rr, center_3D, differ, int(ref["reg_mask"].sum())))
        assert differ == 0
        assert ref["reg_mask"].sum() > B  # the batch is not empty


def test_full_draw_list(device):
    """max_objs = 64 and an image that keeps all 64 objects: its hm plane's draw list holds 64 entries, the capacity of
    the map writer's plain form.  R = 75: odd planes, every plane after the first off a 16-byte boundary."""
    S, Rr, K, cat = 4, 75, 64, "chair"
    opt = PC.make_opt(dict(c=cat, num_symmetry=S, output_res=Rr, hps_uncertainty=True))
    rng = np.random.default_rng(64)
    imgs, objs = [], []
    for b, (w, h) in enumerate(((640, 480), (480, 640))):
        syms = ["True", "False"] if b else ["True"]  # image 0: every object in every variant
        anns = PC.synth_annotations(rng, [(syms[k % len(syms)], "pose") for k in range(K)], w, h)
        s = Rr / max(w, h)  # the whole image lands inside the map: no object leaves it
        t = np.array([[s, 0, (Rr - s * w) / 2], [0, s, (Rr - s * h) / 2]])
        rec = pack_annotations(anns, t, w, h, bool(b), 0.0, opt, max_objs=K)
        imgs.append(rec["pt_image"])
        objs.append(rec["pt_objects"])
    imgs, objs = np.stack(imgs), np.stack(objs)
    ref = R.batch_targets(imgs, objs, S, Rr)
    kept = ref["reg_mask"].sum(axis=2)  # [B, S]
    print("objects kept per (image, variant):", kept.tolist())
    assert kept.max() == K and (kept[0] == K).all()
    out = PoseTargets(opt, max_objs=K)({"pt_image": torch.from_numpy(imgs), "pt_objects": torch.from_numpy(objs)})
    torch.cuda.synchronize()
    differ = _compare(out, ref, target_keys(opt), "64 draws")
    print("64 draws: %d map elements not bit-identical" % differ)
    assert differ == 0


def test_two_streams_bitwise(device):
    rng = np.random.default_rng(7)
    imgs, objs = random_records(rng, 32, 12, 128, "bottle")
    opt = PC.make_opt(dict(c="bottle", num_symmetry=12, output_res=128, hps_uncertainty=True))
    recs = {"pt_image": torch.from_numpy(imgs), "pt_objects": torch.from_numpy(objs)}
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            outs.append(PoseTargets(opt)(recs))
        st.synchronize()
    for k in outs[0]:
        assert torch.equal(outs[0][k].view(torch.uint8) if outs[0][k].dtype == torch.float32 else outs[0][k],
                           outs[1][k].view(torch.uint8) if outs[1][k].dtype == torch.float32 else outs[1][k]), k


def test_loss_on_device_targets_equals_reference_targets(device):
    names = ["chair_carry", "flip_on", "flip_off"]  # S = 4, R = 64, the same target options (flip is in the records)
    topt = PC.make_opt(PC.CASES["chair_carry"][1])
    built = PoseTargets(topt)(_records(names))
    gold = [golden_arrays(GOLD, n, PC.make_opt(PC.CASES[n][1])) for n in names]
    ref = {k: torch.from_numpy(np.concatenate([g[k] for g in gold])).to(device) for k in target_keys(topt)}
    lopt = PLC.make_opt({})
    rng = np.random.default_rng(11)
    outputs = PLC.make_outputs(rng, lopt, len(names), 64, 8)

    def run(batch):
        leaves = [{k: torch.from_numpy(v).to(device).requires_grad_() for k, v in o.items()} for o in outputs]
        outs = [{k: v * 1 for k, v in o.items()} for o in leaves]
        loss, stats, choice = ObjectPoseLoss(lopt)(outs, batch, "train")
        loss.backward()
        torch.cuda.synchronize()
        return loss, stats, choice, leaves

    a, b = run(built), run(ref)
    assert torch.equal(a[0], b[0])
    assert all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    assert torch.equal(a[2], b[2])
    for la, lb in zip(a[3], b[3]):
        for h in la:
            ga, gb = la[h].grad, lb[h].grad
            assert (ga is None) == (gb is None), h
            if ga is not None:
                assert torch.equal(ga, gb), h
    assert float(a[0]) > 0
