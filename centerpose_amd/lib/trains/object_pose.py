"""ObjectPoseTrainer: BaseTrainer with the fused device loss (centerpose_amd.pose_loss.ObjectPoseLoss) and the
reference's ``loss_stats`` names (trains/object_pose.py:212-216).  The debug pictures of the reference's trainer
(:218-401) and ``save_result`` are not built: BaseTrainer refuses them by name."""
from centerpose_amd import hip
from centerpose_amd.pose_loss import ObjectPoseLoss

from .base_trainer import BaseTrainer

LOSS_STATS = tuple(dict.fromkeys(hip.POSE_LOSS_STATS + ('loss',)))  # 'loss' first, as the reference lists them


class ObjectPoseTrainer(BaseTrainer):
    def __init__(self, opt, model, optimizer=None, **kw):
        super().__init__(opt, model, optimizer=optimizer, **kw)

    def _get_losses(self, opt):
        # looked up at call time, as the reference does: a caller may have replaced the module's ObjectPoseLoss
        return list(LOSS_STATS), globals()['ObjectPoseLoss'](opt)
