"""GPU tests of the tracking task's training targets (centerpose_amd/pose_targets_track.py, cp_pose_targets_track):
every golden case against the reference-built arrays (tests/golden/pose_targets_track_ref.npz), seeded batches against
the host restatement (tests/pose_targets_track_ref.py) at the sizes where the kernels take another path,
reproducibility across streams, cp_pose_targets' unchanged results, and one training step of PoseNetGRU and
ObjectPoseLoss on device-built targets."""
import numpy as np
import pytest
import torch

from centerpose_amd import hip
from centerpose_amd.pose_loss import ObjectPoseLoss
from centerpose_amd.pose_targets import PoseTargets, num_symmetry, target_keys
from centerpose_amd.pose_targets_track import TrackPoseTargets, track_target_keys
from tests import pose_loss_cases as PLC
from tests import pose_target_cases as PC
from tests import pose_target_track_cases as TC
from tests import test_pose_targets_cpu as CUR
from tests.test_pose_targets_track_cpu import RECORDS, golden_arrays, random_records, restate

pytestmark = pytest.mark.gpu
HERE = __file__.rsplit("/", 1)[0]
GOLD = np.load(HERE + "/golden/pose_targets_track_ref.npz")
MAPS = ("hm", "hm_hp", "pre_hm", "pre_hm_hp")


def _records(names):
    return {k: np.stack([GOLD[n + "/" + k] for n in names]) for k in RECORDS}


def _compare(dev, ref, keys, where):
    """Integers, masks and float regression targets exactly; every map element within one float32 ulp (a hard
    condition).  Returns the count of map elements that are not bit-identical."""
    differ = 0
    for k in keys:
        a = dev[k].cpu().numpy()
        b = ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (where, k, a.dtype, b.dtype, a.shape, b.shape)
        if k in MAPS:
            ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)  # non-negative floats: ordered
            differ += int((ia != ib).sum())
            assert np.all(np.abs(ia - ib) <= 1), (where, k, int(np.abs(ia - ib).max()))
        else:
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (where, k, np.argwhere(a != b)[:5])
    return differ


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_device_equals_goldens(device, name):
    opt = TC.make_opt(TC.CASES[name][1])
    out = TrackPoseTargets(opt)(_records([name]))
    torch.cuda.synchronize()
    assert sorted(out) == sorted(track_target_keys(opt))
    differ = _compare(out, golden_arrays(GOLD, name, opt), track_target_keys(opt), name)
    print("%s: %d map elements not bit-identical to the reference" % (name, differ))


def _batch_opt(S, inp, Rr, **over):
    cat = {1: "camera", 4: "chair", 12: "bottle"}[S]
    o = dict(c=cat, num_symmetry=S, input_res=max(inp), input_w=inp[0], input_h=inp[1], output_res=Rr, hps_uncertainty=True,
             obj_scale_uncertainty=True, hm_hp_disturb=0.3)  # joints land beside the map now and then
    o.update(over)
    return TC.make_opt(o)


def _check_batch(opt, recs, max_pre_objs, where):
    out = TrackPoseTargets(opt, max_pre_objs=max_pre_objs)(recs)
    torch.cuda.synchronize()
    ref = restate(recs, opt)
    differ = _compare(out, ref, track_target_keys(opt), where)
    kept = sum(q["kept"] for im in ref["pre"] for q in im)
    print("%s: %d map elements not bit-identical, %d previous objects kept, %d / %d tracking / tracking_hp masks set"
          % (where, differ, kept, int(ref["tracking_mask"].sum()), int(ref["tracking_hp_mask"].sum())))
    B = recs["pt_image"].shape[0]
    assert kept > B and ref["reg_mask"].sum() > B and ref["tracking_mask"].sum() >= B
    assert ref["tracking_hp_mask"].sum() > 8 * B and (ref["pre_hm"] > 0).sum() > 100 * B
    return ref


# input 300 / output 75: 75 * 75 is odd, so the current planes start off 16-byte boundaries; 384 x 256: a rectangular input
@pytest.mark.parametrize("S, inp, Rr", [(1, (256, 256), 64), (4, (256, 256), 64), (12, (256, 256), 64), (4, (300, 300), 75),
                                        (4, (384, 256), 64)])
def test_device_equals_restatement(device, S, inp, Rr):
    rng = np.random.default_rng(1000 * S + inp[0])
    for center_3D, mode in ((False, 1), (True, 0)):
        opt = _batch_opt(S, inp, Rr, center_3D=center_3D, use_absolute_scale=center_3D, tracking_label_mode=mode,
                         hm_heat_random=not center_3D, hm_hp_heat_random=not center_3D)
        _check_batch(opt, random_records(rng, 8, opt), None, (S, inp, Rr, center_3D))


def test_full_draw_lists(device):
    """max_pre_objs = 64, every centre kept and every false-positive uniform below its threshold: a plane's draw list
    holds 128 entries, the smallest shape that crosses the map writer's one-wavefront compaction."""
    opt = _batch_opt(1, (256, 256), 64, hm_disturb=0.01, hm_hp_disturb=0.01, hm_heat_random=False)
    rng = np.random.default_rng(64)
    recs = random_records(rng, 8, opt, max_pre_objs=64, n_objects=8, edits=[("allfp",)])
    ref = _check_batch(opt, recs, 64, "128 draws")
    full = [sum(1 for q in im for c, _, _, k in q["draws"] if c == 0 and k) for im in ref["pre"]]
    print("centre draws per image:", full)
    assert max(full) == 128
    joints = [sum(1 for q in im for c, _, _, k in q["draws"] if c == 1 + j and k) for im in ref["pre"] for j in range(8)]
    assert max(joints) > 64


def test_two_streams_bitwise(device):
    opt = _batch_opt(4, (256, 256), 64)
    recs = random_records(np.random.default_rng(7), 8, opt)
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            outs.append(TrackPoseTargets(opt)(recs))
        st.synchronize()
    assert sorted(outs[0]) == sorted(track_target_keys(opt))
    for k in outs[0]:
        assert torch.equal(outs[0][k].view(torch.uint8), outs[1][k].view(torch.uint8)), k


def test_current_frame_entry_unchanged(device):
    """cp_pose_targets through PoseTargets on its own goldens: still bit-identical (it shares the objects kernel)."""
    gold = np.load(HERE + "/golden/pose_targets_ref.npz")
    for name in sorted(PC.CASES):
        opt = PC.make_opt(PC.CASES[name][1])
        out = PoseTargets(opt)({"pt_image": gold[name + "/pt_image"][None], "pt_objects": gold[name + "/pt_objects"][None]})
        torch.cuda.synchronize()
        for k, v in CUR.golden_arrays(gold, name, opt).items():
            a = out[k].cpu().numpy()
            assert a.dtype == v.dtype and np.array_equal(a.view(np.uint8), v.view(np.uint8)), (name, k)


def _loss_opt(**kw):
    return PLC.make_opt(dict(tracking=True, tracking_hp=True, **kw))


def test_loss_on_device_targets_equals_reference_targets(device):
    """ObjectPoseLoss with the tracking terms on, on device-built against reference-built golden targets: bitwise."""
    for names in (["chair_filter"], ["center3d"], ["label0_plain", "leave_clip", "out_flip_twice"]):
        topts = [TC.make_opt(TC.CASES[n][1]) for n in names]
        recs = _records(names)
        if len(names) > 1:  # one option set for the batch: these cases differ in what the records carry (flip) and in
            # the label mode / disturbances, so they are built one by one and concatenated
            built = [TrackPoseTargets(o)({k: v[i:i + 1] for k, v in recs.items()}) for i, o in enumerate(topts)]
            built = {k: torch.cat([b[k] for b in built]) for k in built[0]}
        else:
            built = TrackPoseTargets(topts[0])(recs)
        keys = track_target_keys(topts[0])
        gold = [golden_arrays(GOLD, n, o) for n, o in zip(names, topts)]
        ref = {k: torch.from_numpy(np.concatenate([g[k] for g in gold])).to(device) for k in keys}
        lopt = _loss_opt()
        outputs = PLC.make_outputs(np.random.default_rng(11), lopt, len(names), 64, 8)

        def run(batch):
            leaves = [{k: torch.from_numpy(v).to(device).requires_grad_() for k, v in o.items()} for o in outputs]
            outs = [{k: v * 1 for k, v in o.items()} for o in leaves]
            loss, stats, choice = ObjectPoseLoss(lopt)(outs, batch, "train")
            loss.backward()
            torch.cuda.synchronize()
            return loss, stats, choice, leaves

        a, b = run(built), run(ref)
        assert torch.equal(a[0], b[0]), names
        assert all(torch.equal(a[1][k], b[1][k]) for k in a[1]), names
        assert torch.equal(a[2], b[2])
        for la, lb in zip(a[3], b[3]):
            for h in la:
                assert (la[h].grad is None) == (lb[h].grad is None) and (la[h].grad is None or
                                                                          torch.equal(la[h].grad, lb[h].grad)), (names, h)
        assert float(a[0].detach()) > 0 and float(a[1]["tracking_loss"]) > 0 and float(a[1]["tracking_hp_loss"]) > 0, names


def test_training_step_end_to_end(device):
    """Packed records -> TrackPoseTargets -> PoseNetGRU(pre_img, pre_hm, pre_hm_hp) -> ObjectPoseLoss -> backward, B = 2.
    The input is 64 x 64, the short side of tests/test_pose_net_gru_gpu.py's 64 x 96: the current frame's targets are
    square (output_res = 16)."""
    from centerpose_amd import synth
    from centerpose_amd.pose_net_gru import PoseNetGRU
    from tests import pose_net_gru_ref as NR

    hip.set_default_precision("f32")
    opt = _batch_opt(4, (64, 64), 16, hm_hp_disturb=0.02)
    recs = random_records(np.random.default_rng(5), 2, opt, n_objects=4)
    ref = restate(recs, opt)
    assert ref["tracking_mask"].sum() >= 2 and ref["tracking_hp_mask"].sum() >= 16
    batch = TrackPoseTargets(opt)(recs)
    assert batch["pre_hm"].shape == (2, 1, 64, 64) and batch["pre_hm_hp"].shape == (2, 8, 64, 64)
    net = PoseNetGRU(synth.HEADS_TRACK, head_conv=NR.HEAD_CONV, opt=opt)
    net.load_state_dict(NR.case_state_dict(True), strict=True)
    net = net.to(device).train()
    gen = torch.Generator().manual_seed(3)
    x, pre_img = (torch.rand(2, 3, 64, 64, generator=gen).to(device) for _ in range(2))
    out = net(x, pre_img, batch["pre_hm"], batch["pre_hm_hp"])
    # channels_last head maps (views) -> the loss's own NCHW tensors (it overwrites hm / hm_hp in place)
    out = [{h: v.clone(memory_format=torch.contiguous_format) for h, v in z.items()} for z in out]
    loss, stats, _ = ObjectPoseLoss(_loss_opt(hps_uncertainty=True, obj_scale_uncertainty=True))(out, batch, "train")
    loss.backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and float(loss) > 0
    assert float(stats["tracking_loss"]) > 0 and float(stats["tracking_hp_loss"]) > 0
    for head in ("tracking", "tracking_hp"):
        grads = [p.grad for n, p in net.named_parameters() if n.startswith(head + ".")]
        assert grads and all(g is not None and torch.isfinite(g).all() for g in grads), head
        assert all(float(g.abs().max()) > 0 for g in grads), head
