"""lib.trains on the device: an epoch of the trainer is the hand-written loop bit for bit, adds no host synchronisation
of its own, hands the weights back for checkpoints and resumes from them, makes the loss fall, and carries the other
network families.  Smallest shapes (tests/train_loop_cases.py)."""
import os
import subprocess
import sys

import pytest
import torch

from tests import train_loop_cases as TL

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LOSS_NAMES = ["loss", "hm_loss", "hp_loss", "hm_hp_loss", "hp_offset_loss", "wh_loss", "off_loss", "obj_scale_loss",
              "tracking_loss", "tracking_hp_loss"]


@pytest.fixture(scope="module", autouse=True)
def deterministic(device):
    from centerpose_amd import hip

    hip.set_default_precision("f32")
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(False)


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    """Four synthetic frames in two videos, 160 x 120, single-frame and tracking layouts."""
    from centerpose_amd import synth

    d = tmp_path_factory.mktemp("synthetic")
    synth.write_dataset(str(d), 4, "chair", splits=("train", "val"))
    synth.write_dataset(str(d), 4, "chair", splits=("train", "val"), tracking=True)
    return d


@pytest.fixture(scope="module")
def hand(data_dir, device):
    """The hand-written loop's two iterations from the seeded state: (parameters and buffers, averages), computed once."""
    from centerpose_amd.optim import Adam

    opt = TL.make_opt(data_dir)
    TL.seed_host()
    net = TL.fresh_posenet(opt, device)
    log = TL.hand_loop(opt, net, Adam(net.parameters(), opt.lr, max_grad_norm=100.), TL.make_loader(opt), 2)
    assert len(log) == 2
    return TL.state_of(net), TL.averages(log)


def _train_epoch(data_dir, device, wrap=None):
    from centerpose_amd.lib.trains.train_factory import train_factory
    from centerpose_amd.optim import Adam

    opt = TL.make_opt(data_dir)
    TL.seed_host()
    net = TL.fresh_posenet(opt, device)
    model = wrap(net) if wrap is not None else net
    trainer = train_factory["object_pose"](opt, model, Adam(net.parameters(), opt.lr, max_grad_norm=100.))
    trainer.set_device(opt.gpus, opt.chunk_sizes, opt.device)
    ret, results, imgs = trainer.train(1, TL.make_loader(opt))
    assert results == {} and imgs == []
    return TL.state_of(net), ret


def _assert_same_run(state, ret, hand):
    want_state, want_avg = hand
    assert list(state) == list(want_state)
    different = [k for k in state if not torch.equal(state[k], want_state[k])]
    assert not different, different[:5]
    assert sorted(ret) == sorted(LOSS_NAMES + ["time"])
    for k in LOSS_NAMES:
        assert abs(ret[k] - want_avg[k]) <= 1e-12 * abs(want_avg[k]), (k, ret[k], want_avg[k])
    assert ret["loss"] > 0 and ret["tracking_loss"] == 0


def test_epoch_is_the_hand_written_loop(data_dir, device, hand):
    state, ret = _train_epoch(data_dir, device)
    print("averages:", {k: ret[k] for k in LOSS_NAMES})
    _assert_same_run(state, ret, hand)


def test_epoch_under_data_parallel_world_1(data_dir, device, hand):
    from centerpose_amd.data_parallel import DataParallel

    state, ret = _train_epoch(data_dir, device, wrap=DataParallel)
    _assert_same_run(state, ret, hand)


def test_no_synchronisation_of_its_own(data_dir, device):
    """The host transfers of run_epoch: none from the trainer's own code before the last step is enqueued, the same number
    after it whatever num_iters is, and inside the library's modules exactly those the hand-written loop makes too."""
    from centerpose_amd.lib.trains.train_factory import train_factory
    from centerpose_amd.optim import Adam

    def trainer_run(num_iters):
        opt = TL.make_opt(data_dir, num_iters=num_iters, print_iter=0)
        TL.seed_host()
        net = TL.fresh_posenet(opt, device)
        optimizer = Adam(net.parameters(), opt.lr, max_grad_norm=100.)
        trainer = train_factory["object_pose"](opt, net, optimizer)
        trainer.set_device(opt.gpus, opt.chunk_sizes, opt.device)
        loader = TL.make_loader(opt, repeat=2)  # four batches
        torch.cuda.synchronize()
        with TL.TransferCounter() as counter:
            counter.count_step(optimizer)
            trainer.run_epoch("train", 1, loader)
        assert counter.steps == num_iters
        return counter

    def hand_run(num_iters):
        opt = TL.make_opt(data_dir)
        TL.seed_host()
        net = TL.fresh_posenet(opt, device)
        optimizer = Adam(net.parameters(), opt.lr, max_grad_norm=100.)
        loader = TL.make_loader(opt, repeat=2)
        torch.cuda.synchronize()
        with TL.TransferCounter() as counter:
            counter.count_step(optimizer)
            TL.hand_loop(opt, net, optimizer, loader, num_iters)
        assert counter.steps == num_iters
        return counter

    t2, t4, h4 = trainer_run(2), trainer_run(4), hand_run(4)
    for counter, n in ((t2, 2), (t4, 4)):
        own_early = [c for c in counter.during(n) if c[2]]
        assert not own_early, own_early  # the trainer's own code asks the device nothing while iterating
        assert counter.after(n) and all(c[2] for c in counter.after(n))  # the read-back of the meter
    print("trainer num_iters 2:", t2.calls)
    print("trainer num_iters 4:", t4.calls)
    print("hand loop, 4 iterations:", h4.calls)
    assert [c[0] for c in t2.after(2)] == [c[0] for c in t4.after(4)]  # independent of num_iters
    # inside the library's modules: what the hand-written loop does as well, iteration by iteration
    assert not h4.after(4)
    assert [c[:2] for c in t4.during(4)] == [c[:2] for c in h4.during(4)]


def _hip_model(opt):
    from centerpose_amd.lib.models.model import create_model

    model = create_model(opt.arch, opt.heads, opt.head_conv, opt=opt)
    model.load_state_dict(TL.initial_state(opt.arch, opt))
    return model


def _hip_trainer(opt, model, optimizer):
    from centerpose_amd.lib.trains.train_factory import train_factory

    trainer = train_factory["object_pose"](opt, model, optimizer)
    trainer.set_device(opt.gpus, opt.chunk_sizes, opt.device)
    return trainer


def _epoch(trainer, opt, epoch):
    TL.seed_host(TL.SEED + epoch)  # every run sees the same draws in the same epoch
    return trainer.train(epoch, TL.make_loader(opt))


def test_hand_off_checkpoint_resume_and_lr(data_dir, device, tmp_path):
    from centerpose_amd.lib.models.model import create_model, load_model, save_model
    from centerpose_amd.optim import Adam

    opt = TL.make_opt(data_dir, no_color_aug=True)
    # the uninterrupted run: two epochs, a checkpoint after the first, as the reference's main writes it
    model = _hip_model(opt)
    optimizer = Adam(model.parameters(), opt.lr, max_grad_norm=100.)
    trainer = _hip_trainer(opt, model, optimizer)
    before = model.state_dict()
    _epoch(trainer, opt, 1)
    net = trainer.model_with_loss.model
    trained = TL.state_of(net)
    path = str(tmp_path / "chair_last.pth")
    save_model(path, 1, model, optimizer)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(ckpt) == ["epoch", "optimizer", "state_dict"] and ckpt["epoch"] == 1
    assert sorted(ckpt["optimizer"]) == ["param_groups", "state"] and len(ckpt["optimizer"]["state"]) > 100
    assert any(not torch.equal(before[k], trained[k]) for k in trained)
    reloaded = load_model(create_model(opt.arch, opt.heads, opt.head_conv, opt=opt), path)
    sd = reloaded.state_dict()
    assert list(sd) == list(trained) and all(torch.equal(sd[k], trained[k]) for k in sd)
    # a detector on the trained weights returns finite records
    from centerpose_amd import synth
    dets = reloaded.to(device)._engine().detect(synth.frames(1, seed=5, h=128, w=128, device=device), K=10, graph=False)[1]
    assert torch.isfinite(dets).all()
    _epoch(trainer, opt, 2)
    want = TL.state_of(net)

    # resumed: a new model and optimizer from the checkpoint, then the second epoch
    model2 = create_model(opt.arch, opt.heads, opt.head_conv, opt=opt)
    optimizer2 = Adam(model2.parameters(), opt.lr, max_grad_norm=100.)
    model2, optimizer2, start = load_model(model2, path, optimizer2, True, opt.lr, opt.lr_step)
    assert start == 1
    trainer2 = _hip_trainer(opt, model2, optimizer2)
    _epoch(trainer2, opt, 2)
    got = TL.state_of(trainer2.model_with_loss.model)
    different = [k for k in want if not torch.equal(want[k], got[k])]
    assert not different, different[:5]
    handed = model2.state_dict()
    assert all(torch.equal(handed[k], got[k]) for k in got)  # load_module after the epoch

    # an lr edit on the caller's param_groups is what the next step reads: at 0 no parameter moves
    model3 = create_model(opt.arch, opt.heads, opt.head_conv, opt=opt)
    optimizer3 = Adam(model3.parameters(), opt.lr, max_grad_norm=100.)
    model3, optimizer3, _ = load_model(model3, path, optimizer3, True, opt.lr, opt.lr_step)
    trainer3 = _hip_trainer(opt, model3, optimizer3)
    for group in optimizer3.param_groups:
        group["lr"] = 0.0
    _epoch(trainer3, opt, 2)
    frozen = TL.state_of(trainer3.model_with_loss.model)
    params = [k for k, _ in trainer3.model_with_loss.model.named_parameters()]
    assert all(torch.equal(frozen[k], trained[k]) for k in params)
    assert any(not torch.equal(want[k], trained[k]) for k in params)


def test_loss_falls(data_dir, device):
    """Three epochs of ten iterations on the same two frames (no flip, no crop, no colour, no shift or scale)."""
    from centerpose_amd.lib.trains.train_factory import train_factory
    from centerpose_amd.optim import Adam

    opt = TL.make_opt(data_dir, flip=0.0, not_rand_crop=True, no_color_aug=True, shift=0.0, scale=0.0)
    TL.seed_host()
    net = TL.fresh_posenet(opt, device)
    trainer = train_factory["object_pose"](opt, net, Adam(net.parameters(), opt.lr, max_grad_norm=100.))
    trainer.set_device(opt.gpus, opt.chunk_sizes, opt.device)
    from centerpose_amd.lib.datasets.dataset_combined import ObjectPoseDataset
    from centerpose_amd.lib.datasets.dataset_factory import collate_fn_filtered
    two = torch.utils.data.Subset(ObjectPoseDataset(opt, "train"), [0, 1])
    loader = torch.utils.data.DataLoader(torch.utils.data.ConcatDataset([two] * 10), batch_size=2, shuffle=False,
                                         collate_fn=collate_fn_filtered)
    losses = [trainer.train(epoch, loader)[0]["loss"] for epoch in (1, 2, 3)]
    print("average loss per epoch:", losses)
    assert all(l == l and l > 0 for l in losses)
    assert losses[2] < losses[0], losses


FAMILIES = {
    "dlav1_34_tracking": ("dlav1_34", TL.TRACK_FLAGS),
    "hourglass": ("hourglass", []),
    "resdcn_18": ("resdcn_18", []),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_other_families_one_iteration(family, data_dir, device):
    from centerpose_amd.optim import Adam

    arch, extra = FAMILIES[family]
    opt = TL.make_opt(data_dir, arch=arch, extra=extra, num_iters=1)
    assert opt.num_stacks == (2 if arch == "hourglass" else 1)
    model = _hip_model(opt)
    optimizer = Adam(model.parameters(), opt.lr, max_grad_norm=100.)
    trainer = _hip_trainer(opt, model, optimizer)
    net = trainer.model_with_loss.model
    assert type(net).__name__ == {"dlav1_34": "PoseNetGRU", "hourglass": "PoseNetHourglass", "resdcn_18": "PoseNetResDCN"}[arch]
    TL.seed_host()
    ret, _, _ = trainer.train(1, TL.make_loader(opt))
    assert sorted(ret) == sorted(LOSS_NAMES + ["time"])
    assert all(ret[k] == ret[k] and abs(ret[k]) < float("inf") for k in LOSS_NAMES) and ret["loss"] > 0
    if extra:
        assert ret["tracking_loss"] > 0 and ret["tracking_hp_loss"] > 0
    grads = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    assert len(grads) > 50 and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert net.training
    buffers = {k: v.detach().clone() for k, v in net.named_buffers()}
    params = {k: v.detach().clone() for k, v in net.named_parameters()}
    TL.seed_host()
    val, _, _ = trainer.val(1, TL.make_loader(opt))
    assert not net.training and sorted(val) == sorted(ret) and val["loss"] == val["loss"]
    assert all(torch.equal(v, buffers[k]) for k, v in net.named_buffers())  # running statistics untouched
    assert all(torch.equal(v, params[k]) for k, v in net.named_parameters())


def test_train_tool_on_a_synthetic_set(tmp_path, device):
    out = tmp_path / "exp"
    cmd = [sys.executable, os.path.join(REPO, "tools", "train.py"), "--synthetic", "4", "--num_epochs", "1", "--num_iters", "2",
           "--batch_size", "2", "--input_res", "128", "--head_conv", "64", "--num_workers", "0", "--print_iter", "1",
           "--out_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for name in ("chair_last.pth", "opt.txt", "log.txt"):
        assert (out / name).is_file(), name
    ckpt = torch.load(str(out / "chair_last.pth"), map_location="cpu", weights_only=False)
    assert ckpt["epoch"] == 1 and "optimizer" in ckpt
    assert "train_loss" in (out / "log.txt").read_text()
    assert r.stdout.count("object_pose/default| train: [1]") == 2
