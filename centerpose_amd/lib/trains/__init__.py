"""Mirror of the reference's ``lib.trains``: the trainer contract (base_trainer), ObjectPoseTrainer (object_pose) and
``train_factory``."""
