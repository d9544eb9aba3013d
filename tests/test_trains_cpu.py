"""lib.trains on the CPU: the loop's logic with a two-parameter module, a stand-in loss and injected expanders; the
small modules the reference's entry points import; and the entry points themselves resolving against the mirror."""
import importlib.util
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from centerpose_amd.lib.trains.base_trainer import BaseTrainer, ModelWithLoss
from tests import pose_target_cases as PC

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ["loss", "hm_loss", "wh_loss"]


class TwoParams(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(0.5))
        self.b = torch.nn.Parameter(torch.tensor(-0.25))
        self.seen_training = []

    def forward(self, x, pre_img=None, pre_hm=None, pre_hm_hp=None):
        self.seen_training.append(self.training)
        return [{"hm": x * self.w + self.b}]


class StandInLoss(torch.nn.Module):
    """loss = mean((hm - target)^2); hm_loss a second tensor statistic; wh_loss reported as a plain number (a head that
    is off).  Keeps every statistic it returned, as float32 values."""

    def __init__(self):
        super().__init__()
        self.log = []

    def forward(self, outputs, batch, phase):
        loss = ((outputs[-1]["hm"] - batch["target"]) ** 2).mean()
        stats = {"loss": loss, "hm_loss": (outputs[-1]["hm"].detach().abs().mean() * 3).float(), "wh_loss": 0}
        self.log.append((phase, float(loss.detach()), float(stats["hm_loss"]), int(batch["input"].size(0))))
        return loss, stats, None


class Trainer(BaseTrainer):
    def _get_losses(self, opt):
        return list(NAMES), StandInLoss()


def make_opt(**kw):
    o = dict(num_iters=-1, print_iter=0, debug=0, hide_data_time=False, task="object_pose", exp_id="t", tracking_task=False,
             gpus=[0])
    o.update(kw)
    return SimpleNamespace(**o)


def batches(sizes, seed=0):
    """Collated stand-in batches: 'ti_image' carries the values the stand-in input expander returns."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        if n is None:
            out.append(None)
            continue
        x = torch.randn(n, 4, generator=g, dtype=torch.float64)
        out.append({"frame": [np.zeros((2, 2, 3), np.uint8)] * n, "ti_image": x, "y": torch.randn(n, 4, generator=g)})
    return out


def expanders():
    calls = {"inputs": 0, "targets": 0}

    def inputs(frames, records, device=None):
        calls["inputs"] += 1
        assert isinstance(frames, list) and len(frames) == records.shape[0]
        return records.float()

    def targets(batch):
        calls["targets"] += 1
        return {"target": batch["y"]}

    return inputs, targets, calls


def build(opt, lr=0.1):
    net = TwoParams()
    optimizer = torch.optim.SGD(net.parameters(), lr)
    inputs, targets, calls = expanders()
    return Trainer(opt, net, optimizer, inputs=inputs, targets=targets), net, optimizer, calls


def weighted_mean(log, column):
    """The batch-size-weighted mean, in float64, of the float32 values the loss returned."""
    total = sum(np.float64(np.float32(row[column])) * row[3] for row in log)
    return total / sum(row[3] for row in log)


def test_num_iters_cut_off_and_none_batches():
    trainer, net, _, calls = build(make_opt(num_iters=3))
    ret, results, writer_imgs = trainer.train(1, batches([2, None, 3, 2, 2]))
    # the reference counts the loader's index: batch 1 is skipped, batch 3 is the first one at or beyond num_iters
    assert [row[3] for row in trainer.loss.log] == [2, 3] and calls == {"inputs": 2, "targets": 2}
    assert results == {} and writer_imgs == []
    assert sorted(ret) == sorted(NAMES + ["time"]) and ret["time"] >= 0
    trainer2, _, _, _ = build(make_opt())
    trainer2.train(1, batches([2, None, 3, 2, 2]))
    assert [row[3] for row in trainer2.loss.log] == [2, 3, 2, 2]


def test_train_updates_val_does_not_and_modes():
    trainer, net, _, _ = build(make_opt())
    before = [p.detach().clone() for p in net.parameters()]
    trainer.val(1, batches([2, 3]))
    assert all(torch.equal(a, b) for a, b in zip(before, net.parameters()))
    assert not net.training and net.seen_training == [False, False]
    assert all(p.grad is None for p in net.parameters())
    trainer.train(1, batches([2, 3]))
    assert all(not torch.equal(a, b) for a, b in zip(before, net.parameters()))
    assert net.training and net.seen_training[2:] == [True, True]
    assert [row[0] for row in trainer.loss.log] == ["val", "val", "train", "train"]


@pytest.mark.parametrize("phase", ["train", "val"])
def test_averages_are_the_weighted_float64_means(phase):
    trainer, _, _, _ = build(make_opt())
    ret, _, _ = getattr(trainer, phase)(1, batches([1, 4, 2, 3, 5], seed=3))
    log = trainer.loss.log
    assert len(log) == 5
    for name, column in (("loss", 1), ("hm_loss", 2)):
        want = weighted_mean(log, column)
        assert abs(ret[name] - want) <= 1e-12 * abs(want), (name, ret[name], want)
    assert ret["wh_loss"] == 0  # reported as a non-tensor: never counted


def test_printed_line(capsys):
    trainer, _, _, _ = build(make_opt(print_iter=2))
    trainer.train(7, batches([2, 2, 2]))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("object_pose/t|")]
    assert len(lines) == 2 and "train: [7][0/3]" in lines[0] and "train: [7][2/3]" in lines[1]
    assert "|loss " in lines[0] and "|Data " in lines[0] and "|Net " in lines[0]
    want = weighted_mean(trainer.loss.log[:1], 1)
    assert "|loss %.4f " % want in lines[0]


def test_debug_warns_once_and_goes_on():
    trainer, net, _, _ = build(make_opt(debug=5))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        ret1, _, imgs1 = trainer.train(1, batches([2]))
        ret2, _, imgs2 = trainer.val(1, batches([2]))
        trainer.train(2, batches([2]))
    mine = [w for w in caught if "debug" in str(w.message)]
    assert len(mine) == 1 and "not built" in str(mine[0].message)
    assert imgs1 == [] and imgs2 == [] and len(trainer.loss.log) == 3
    with pytest.raises(NotImplementedError, match="debug pictures"):
        trainer.debug({}, {}, 0, None)
    with pytest.raises(NotImplementedError, match="save_result"):
        trainer.save_result({}, {}, {})


def test_set_device_refuses_two_gpus_by_name():
    trainer, net, optimizer, _ = build(make_opt())
    with pytest.raises(NotImplementedError, match=r"centerpose_amd\.data_parallel\.DataParallel"):
        trainer.set_device([0, 1], [1, 1], "cpu")
    from centerpose_amd.lib.models.data_parallel import DataParallel
    with pytest.raises(NotImplementedError, match=r"centerpose_amd\.data_parallel\.DataParallel"):
        DataParallel(net, device_ids=[0, 1], chunk_sizes=[1, 1])
    trainer.set_device([0], [2], "cpu")
    assert trainer.device == torch.device("cpu")


def test_clip_only_when_the_optimizer_does_not_fold_it_in(monkeypatch):
    seen = []
    inner = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda params, norm: seen.append(norm) or inner(params, norm))
    trainer, _, optimizer, _ = build(make_opt())
    trainer.train(1, batches([2, 2]))
    assert seen == [100., 100.]
    trainer.val(1, batches([2]))
    assert len(seen) == 2
    optimizer.param_groups[0]["max_grad_norm"] = 100.  # centerpose_amd.optim.Adam(max_grad_norm=100.)'s group key
    trainer.train(2, batches([2, 2]))
    assert len(seen) == 2


def test_model_with_loss_returns_the_last_stack_and_contiguous_heads():
    class TwoStacks(torch.nn.Module):
        def forward(self, x, pre_img=None, pre_hm=None, pre_hm_hp=None):
            assert pre_img is not None and pre_hm is None
            y = x.contiguous(memory_format=torch.channels_last)
            return [{"hm": y}, {"hm": y + 1}]

    seen = {}

    def loss(outputs, batch, phase):
        seen["layouts"] = [z["hm"].is_contiguous() for z in outputs]
        return outputs[0]["hm"].sum(), {"loss": 1}, "choice"

    x = torch.randn(2, 4, 3, 3)
    out, l, stats, choice = ModelWithLoss(TwoStacks(), loss)({"input": x, "pre_img": x}, "train")
    assert seen["layouts"] == [True, True] and torch.equal(out["hm"], x + 1) and choice == "choice"


def test_factory_and_loss_names():
    from centerpose_amd import hip
    from centerpose_amd.lib.trains import object_pose
    from centerpose_amd.lib.trains.train_factory import train_factory
    from centerpose_amd.pose_loss import ObjectPoseLoss

    assert train_factory == {"object_pose": object_pose.ObjectPoseTrainer}
    assert object_pose.ObjectPoseLoss is ObjectPoseLoss
    # the reference's loss_states (trains/object_pose.py:213-214)
    assert list(object_pose.LOSS_STATS) == ["loss", "hm_loss", "hp_loss", "hm_hp_loss", "hp_offset_loss", "wh_loss", "off_loss",
                                            "obj_scale_loss", "tracking_loss", "tracking_hp_loss"]
    assert set(object_pose.LOSS_STATS) == set(hip.POSE_LOSS_STATS)


def test_optimizer_is_repointed_at_the_training_module():
    """A HipPoseNet from create_model, as the reference's main passes it: the caller's optimizer steps the module's
    parameters, in HipPoseNet.parameters() key order, with a loaded state re-keyed; load_module hands the weights back."""
    from centerpose_amd import synth
    from centerpose_amd.lib.models.model import create_model

    opt = make_opt(pre_img=False, pre_hm=False, pre_hm_hp=False)
    model = create_model("dla_34", synth.HEADS_POSE, 64, opt)
    model.load_state_dict(synth.make_state_dict("dla_34", synth.HEADS_POSE, head_conv=64))
    optimizer = torch.optim.Adam(model.parameters(), 1e-3)  # built BEFORE load_state_dict replaced the tensors, as main does
    held = optimizer.param_groups[0]["params"]
    optimizer.state[held[0]] = {"step": torch.tensor(3.), "exp_avg": torch.full_like(held[0], 2.), "exp_avg_sq": torch.ones_like(held[0])}
    optimizer.state[held[-1]] = {"step": torch.tensor(3.), "exp_avg": torch.full_like(held[-1], 5.), "exp_avg_sq": torch.ones_like(held[-1])}
    trainer = Trainer(opt, model, optimizer)
    net = trainer.model_with_loss.model
    keys = [k for k, v in model.state_dict().items() if v.is_floating_point() and "running_" not in k]
    named = dict(net.named_parameters())
    params = optimizer.param_groups[0]["params"]
    assert len(params) == len(keys) and all(p is named[k] for p, k in zip(params, keys))
    assert len(optimizer.state) == 2
    assert float(optimizer.state[named[keys[0]]]["exp_avg"].flatten()[0]) == 2. and float(optimizer.state[named[keys[-1]]]["exp_avg"].flatten()[0]) == 5.
    assert sorted(optimizer.state_dict()["state"]) == [0, len(keys) - 1]
    optimizer.param_groups[0]["lr"] = 0.5  # the caller's edit is the one the step reads
    assert trainer.optimizer.param_groups[0]["lr"] == 0.5
    with pytest.raises(ValueError, match="model.parameters"):
        Trainer(opt, model, torch.optim.Adam(list(model.parameters())[:3], 1e-3))


def test_logger_average_meter(tmp_path):
    from centerpose_amd.lib.logger import Logger
    from centerpose_amd.lib.utils.utils import AverageMeter

    opt = SimpleNamespace(save_dir=str(tmp_path / "exp"), debug_dir=str(tmp_path / "exp" / "debug"), lr=1e-3, c="chair")
    logger = Logger(opt)
    logger.write("epoch: 1 | ")
    logger.write("train_loss 1.000000 | ")
    logger.write("\n")
    logger.scalar_summary("train_loss", 1.0, 1)
    logger.img_summary("train", [], 1)
    logger.close()
    text = (tmp_path / "exp" / "log.txt").read_text()
    assert text.count("epoch: 1 | train_loss 1.000000 | \n") == 1 and text[:2] == "20"  # one time stamp per line
    assert "  lr: 0.001\n" in (tmp_path / "exp" / "opt.txt").read_text()
    m = AverageMeter()
    m.update(2.0, 3)
    m.update(4.0, 1)
    assert (m.val, m.sum, m.count, m.avg) == (4.0, 10.0, 4, 2.5)


@pytest.mark.skipif(not PC.reference_available(), reason="the reference tree is not present")
def test_reference_entry_points_resolve_in_the_mirror():
    """main_CenterPose.py and test.py of the reference, imported as modules with centerpose_amd/ first on sys.path:
    every lib.* module they pull in comes from this repository."""
    before, path = set(sys.modules), list(sys.path)
    stale = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "lib" or k.startswith("lib.")}
    try:
        sys.path.insert(0, os.path.join(REPO, "centerpose_amd"))
        pulled = {}
        for script in ("main_CenterPose.py", "test.py"):
            spec = importlib.util.spec_from_file_location("reference_" + script[:-3], os.path.join(PC.REF, "src", script))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            assert callable(mod.main)
            pulled[script] = mod
        libs = {k: m for k, m in sys.modules.items() if k == "lib" or k.startswith("lib.")}
        for name in ("lib.opts", "lib.logger", "lib.models.model", "lib.models.data_parallel", "lib.datasets.dataset_factory",
                     "lib.datasets.dataset_combined", "lib.trains.train_factory", "lib.trains.base_trainer", "lib.utils.utils"):
            assert name in libs, name
        inside = os.path.join(REPO, "centerpose_amd", "lib") + os.sep
        for name, m in libs.items():
            assert os.path.abspath(m.__file__).startswith(inside), (name, m.__file__)
        assert pulled["test.py"].train_factory["object_pose"].__module__ == "lib.trains.object_pose"
    finally:
        for name in set(sys.modules) - before:
            del sys.modules[name]
        sys.modules.update(stale)
        sys.path[:] = path
