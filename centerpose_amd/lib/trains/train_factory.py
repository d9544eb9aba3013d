from .object_pose import ObjectPoseTrainer

train_factory = {'object_pose': ObjectPoseTrainer}
