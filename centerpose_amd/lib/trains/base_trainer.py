"""The training loop with the reference's trainer contract (trains/base_trainer.py): ``ModelWithLoss``,
``BaseTrainer(opt, model, optimizer)``, ``set_device``, ``train`` / ``val`` -> ``(ret, results, writer_imgs)``.

An iteration is the hand-written loop of INTEGRATION.md: the loader's collated records are expanded on the device
(``TrainInputs`` -> ``input`` / ``pre_img``, ``PoseTargets`` or ``TrackPoseTargets`` -> the targets), the network and
``ObjectPoseLoss`` run, and in 'train' ``zero_grad``, ``backward``, ``step`` follow.

**The loop asks the device nothing.**  The reference reads about fifteen scalars back per iteration
(``loss_stats[l].mean().item()``, :106-111).  Here the running sums of the statistics live on the device, in one
float64 vector over ``loss_stats`` (``acc += stats.double() * n``), and are read back only when a progress line is
printed (``opt.print_iter > 0 and iter_id % opt.print_iter == 0``) and once at the end of the epoch.  The per-iteration
code of this module calls no ``.item()``, ``.cpu()``, ``.tolist()``, ``.numpy()`` and no ``torch.cuda.synchronize()``.

One consequence for the printed line: ``Data`` and ``Net`` are host-side wall-clock times around calls that only
enqueue work, so they measure the time to ENQUEUE an iteration, not to compute it (they converge to the device's time per
iteration once the launch queue is full and the host is throttled by it).  ``ret['time']`` is taken after the final
read-back, which waits for the device, and is the true duration of the epoch in minutes.
"""
import copy
import time
import warnings

import torch

from centerpose_amd.data_parallel import DataParallel as _HipDataParallel

from ..models.data_parallel import MULTI_GPU_MESSAGE
from ..utils.utils import AverageMeter


class ModelWithLoss(torch.nn.Module):
    def __init__(self, model, loss):
        super().__init__()
        self.model = model
        self.loss = loss

    def forward(self, batch, phase):
        previous = [batch.get(k) for k in ('pre_img', 'pre_hm', 'pre_hm_hp')]
        # the single-frame families (hourglass, resdcn_N) take the image alone
        outputs = self.model(batch['input'], *previous) if any(p is not None for p in previous) else self.model(batch['input'])
        # the loss reads NCHW-contiguous heads and overwrites hm / hm_hp in place, which autograd allows on a tensor of its
        # own only: PoseNetGRU and the hourglass return channels_last heads or views of a shared buffer, and get copies
        outputs = [{h: v if v.is_contiguous() and not v._is_view() else v.clone(memory_format=torch.contiguous_format)
                    for h, v in z.items()} for z in outputs]
        loss, loss_stats, choice_list = self.loss(outputs, batch, phase)
        return outputs[-1], loss, loss_stats, choice_list


def _scalar(t):
    """A statistic as a 0-d float32 tensor without a graph (the mean over the replicas where it has a dimension)."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.dim() == 0 else t.mean()


def _training_module(model):
    """The nn.Module that trains ``model``: itself, or for a lib.models HipPoseNet the module of its family holding the
    model's parameters and buffers."""
    if isinstance(model, torch.nn.Module):
        return model, None
    arch = getattr(model, 'arch', None)
    if not isinstance(arch, str) or not hasattr(model, 'load_module'):
        raise TypeError("BaseTrainer: model must be an nn.Module or a HipPoseNet of lib.models.model.create_model, got %r"
                        % type(model).__name__)
    if arch.startswith('dlav1'):
        from centerpose_amd.pose_net_gru import PoseNetGRU
        return PoseNetGRU.from_model(model), model
    if arch == 'hourglass':
        from centerpose_amd.pose_net_hourglass import PoseNetHourglass
        return PoseNetHourglass.from_model(model), model
    if arch.startswith('resdcn'):
        from centerpose_amd.pose_net_resdcn import PoseNetResDCN
        return PoseNetResDCN.from_model(model), model
    return model.train_module(), model


def _repoint(optimizer, owner, net):
    """Makes the optimizer a caller built over ``owner.parameters()`` (a HipPoseNet's tensors) step ``net``'s parameters
    instead: group by group, position by position in HipPoseNet.parameters()' key order, with any state it already
    holds (a resumed checkpoint) re-keyed the same way.  The optimizer object, its groups and their options stay the
    caller's, so ``param_groups[i]['lr'] = ...`` and ``state_dict()`` keep their meaning."""
    keys = [k for k, v in owner.state_dict().items() if v.is_floating_point() and 'running_' not in k]
    named = dict(net.named_parameters())
    missing = [k for k in keys if k not in named]
    if missing:
        raise RuntimeError("BaseTrainer: the training module has no parameter %s" % missing[:5])
    held = sum(len(g['params']) for g in optimizer.param_groups)
    if held != len(keys):
        raise ValueError("BaseTrainer: the optimizer holds %d parameters, model.parameters() has %d: build it over "
                         "model.parameters()" % (held, len(keys)))
    state, at = {}, 0
    for group in optimizer.param_groups:
        new = [named[k] for k in keys[at:at + len(group['params'])]]
        at += len(new)
        for old, p in zip(group['params'], new):
            if old in optimizer.state:
                state[p] = optimizer.state[old]
        group['params'] = new
    optimizer.state.clear()
    optimizer.state.update(state)
    if hasattr(optimizer, '_groups'):  # centerpose_amd.optim.Adam: its device tables are laid out again at the next step
        optimizer._groups = None


class BaseTrainer(object):
    """``inputs`` / ``targets``: the two expanders, ``inputs(frames, ti_records, device=...)`` -> float32 images and
    ``targets(batch)`` (``targets(batch, pre_img=...)`` for the tracking task) -> {name: tensor}; by default
    ``TrainInputs(opt)`` and ``PoseTargets`` / ``TrackPoseTargets`` on a copy of ``opt`` with ``debug = 0``, built when
    the first batch arrives.  ``detector``: the dlav1_34 model of ``TrackPoseTargets(opt, detector=...)`` for
    ``opt.data_generation_mode_ratio > 0``."""

    def __init__(self, opt, model, optimizer=None, inputs=None, targets=None, detector=None):
        self.opt = opt
        self.optimizer = optimizer
        self.loss_stats, self.loss = self._get_losses(opt)
        net, self.owner = _training_module(model)
        if self.owner is not None and optimizer is not None:
            _repoint(optimizer, self.owner, net)
        self.model_with_loss = ModelWithLoss(net, self.loss)
        self.inputs, self.targets, self.detector = inputs, targets, detector
        self.device = None
        self._warned_debug = False

    # ---- devices ----
    def set_device(self, gpus, chunk_sizes, device):
        if len(gpus) > 1:
            raise NotImplementedError(MULTI_GPU_MESSAGE)
        self.device = torch.device(device)
        if not isinstance(self.model_with_loss.model, _HipDataParallel):  # a wrapped module was moved before it was wrapped
            self.model_with_loss = self.model_with_loss.to(self.device)
        if self.optimizer is not None:
            for state in self.optimizer.state.values():
                for k, v in state.items():
                    if isinstance(v, torch.Tensor):
                        state[k] = v.to(device=self.device, non_blocking=True)
            if hasattr(self.optimizer, '_groups'):
                self.optimizer._groups = None

    # ---- the batch ----
    def _expanders(self):
        opt = self.opt
        if self.inputs is None:
            from centerpose_amd.train_inputs import TrainInputs
            self.inputs = TrainInputs(opt)
        if self.targets is None:
            topt = copy.copy(opt)
            topt.debug = 0  # meta / gt_det are not produced
            if getattr(opt, 'tracking_task', False):
                from centerpose_amd.pose_targets_track import TrackPoseTargets
                self.targets = TrackPoseTargets(topt, detector=self.detector)
            else:
                from centerpose_amd.pose_targets import PoseTargets
                self.targets = PoseTargets(topt)
        return self.inputs, self.targets

    def expand(self, batch):
        """The collated records -> the reference's batch, on the device and on the current stream."""
        inputs, targets = self._expanders()
        if getattr(self.opt, 'tracking_task', False):
            both = inputs(list(batch['frame']) + list(batch['frame_pre']),
                          torch.cat([torch.as_tensor(batch['ti_image']), torch.as_tensor(batch['ti_image_pre'])]),
                          device=self.device)
            half = both.shape[0] // 2  # train_inputs.split_tracking
            batch['input'], pre_img = both[:half], both[half:]
            batch.update(targets(batch, pre_img=pre_img))
            if getattr(self.opt, 'pre_img', False):
                batch['pre_img'] = pre_img
        else:
            batch['input'] = inputs(batch['frame'], batch['ti_image'], device=self.device)
            batch.update(targets(batch))
        return batch

    # ---- the epoch ----
    def _line(self, phase, epoch, iter_id, num_iters, start, acc, counts, data_time, batch_time):
        """One progress line in the reference's format.  Reads the accumulator back: the one host transfer of a printed
        iteration.  ``Data`` / ``Net`` are enqueue times (see the module text)."""
        opt = self.opt
        sums = acc.cpu().tolist()
        text = '{phase}: [{0}][{1}/{2}]|Tot: {3:.0f}s '.format(epoch, iter_id, num_iters, time.time() - start, phase=phase)
        for l, total, n in zip(self.loss_stats, sums, counts):
            text += '|{} {:.4f} '.format(l, total / n if n else 0.)
        if not opt.hide_data_time:
            text += '|Data {dt.val:.3f}s({dt.avg:.3f}s) |Net {bt.avg:.3f}s'.format(dt=data_time, bt=batch_time)
        print('{}/{}| {}'.format(opt.task, opt.exp_id, text))

    def run_epoch(self, phase, epoch, data_loader):
        opt = self.opt
        model_with_loss = self.model_with_loss
        net = model_with_loss.model
        parallel = net if isinstance(net, _HipDataParallel) else None
        if phase == 'train':
            model_with_loss.train()
        else:
            model_with_loss.eval()
        clip = phase == 'train' and not any(g.get('max_grad_norm') for g in self.optimizer.param_groups)
        if opt.debug > 0 and not self._warned_debug:
            self._warned_debug = True
            warnings.warn("lib.trains: opt.debug = %d: the training debug pictures (trains/object_pose.py:218-401) are not "
                          "built; writer_imgs stays empty" % opt.debug)
        results, writer_imgs = {}, []
        data_time, batch_time = AverageMeter(), AverageMeter()
        num_iters = len(data_loader) if opt.num_iters < 0 else opt.num_iters
        names = list(self.loss_stats)
        acc, counts = None, [0] * len(names)
        start = end = time.time()
        for iter_id, batch in enumerate(data_loader):
            if batch is None:  # every sample of it was unreadable
                continue
            if iter_id >= num_iters:
                break
            data_time.update(time.time() - end)
            batch = self.expand(batch)
            output, loss, loss_stats, choice_list = model_with_loss(batch, phase)
            if loss.dim():  # one value per replica in the reference; a 0-d loss is its own mean
                loss = loss.mean()
            if phase == 'train':
                self.optimizer.zero_grad()
                loss.backward()
                if parallel is not None:
                    parallel.reduce_gradients()
                if clip:
                    torch.nn.utils.clip_grad_norm_(net.parameters(), 100.)
                self.optimizer.step()
            if parallel is not None and parallel.world > 1:
                loss_stats = parallel.reduce_stats({l: loss_stats[l] for l in names if torch.is_tensor(loss_stats[l])})
            # the meter: one small accumulate on the device, nothing read back
            n = batch['input'].size(0)
            if acc is None:
                acc = torch.zeros(len(names), dtype=torch.float64, device=loss.device)
                zero = torch.zeros((), dtype=torch.float32, device=loss.device)
            present = [torch.is_tensor(loss_stats.get(l)) for l in names]  # a head that is off may be reported as a number
            stats = torch.stack([_scalar(loss_stats[l]) if on else zero for l, on in zip(names, present)])
            acc += stats.double() * n
            counts = [c + n if on else c for c, on in zip(counts, present)]
            batch_time.update(time.time() - end)
            end = time.time()
            if opt.print_iter > 0 and iter_id % opt.print_iter == 0:
                self._line(phase, epoch, iter_id, num_iters, start, acc, counts, data_time, batch_time)
            del output, loss, loss_stats, batch
        sums = acc.cpu().tolist() if acc is not None else [0.] * len(names)  # waits for the epoch's last launch
        ret = {l: (total / n if n else 0.) for l, total, n in zip(names, sums, counts)}
        ret['time'] = (time.time() - start) / 60.
        if phase == 'train' and self.owner is not None:  # the caller's model (and its save_model) sees the trained weights
            self.owner.load_module(parallel.module if parallel is not None else net)
        return ret, results, writer_imgs

    def debug(self, batch, output, iter_id, choice_list=None):
        raise NotImplementedError("lib.trains: the training debug pictures (trains/object_pose.py:218-401) are not built")

    def save_result(self, output, batch, results):
        raise NotImplementedError("lib.trains: save_result is not built (the evaluation runs through the detectors)")

    def _get_losses(self, opt):
        raise NotImplementedError

    def val(self, epoch, data_loader):
        with torch.no_grad():
            return self.run_epoch('val', epoch, data_loader)

    def train(self, epoch, data_loader):
        return self.run_epoch('train', epoch, data_loader)
