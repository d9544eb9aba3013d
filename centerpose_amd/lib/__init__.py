"""Drop-in mirror of the reference's ``lib`` package for the inference hot path.

Put ``centerpose_amd/`` on ``sys.path`` (instead of the reference's ``src/``) and the reference's
``demo.py`` imports — ``lib.opts.opts``, ``lib.detectors.detector_factory.detector_factory``,
``lib.models.model.create_model/load_model``, ``lib.models.decode.object_pose_decode``,
``lib.utils.pnp.cuboid_pnp_shell.pnp_shell`` — resolve here, with the compute routed to
libcenterpose_hip.so.  Only what the inference hot path needs is mirrored: detectors (incl. the CenterPoseTrack
per-frame loop with ``lib.utils.tracker.Tracker`` / ``Tracker_baseline``), opts, model factory, decode, PnP packaging,
``lib.utils.debugger``.  The reference's own ``src/demo.py`` runs unmodified against it (tests/test_demo_dropin.py).

The training side is mirrored by name as well, so that ``main_CenterPose.py`` / ``main_CenterPoseTrack.py`` and
``test.py`` import against this package: ``lib.datasets`` (``ObjectPoseDataset`` with the reference's discovery and
random stream, whose samples are a decoded frame plus the small records the device expands; ``collate_fn_filtered``),
``lib.trains`` (``train_factory``, ``BaseTrainer`` / ``ObjectPoseTrainer``: the training step of the library's operators,
with the loss statistics summed on the device), ``lib.logger``, ``lib.utils.utils.AverageMeter`` and
``lib.models.data_parallel`` (a name that points at one process per GPU).  Not mirrored: the trainer's debug pictures
and ``save_result``, the dataset's ``meta`` / ``gt_det`` record, ``new_data_augmentation``, a detector constructed
inside the dataset ("Training with the reference's loop").
"""
import os as _os
import sys as _sys

# Works both as ``centerpose_amd.lib`` and as top-level ``lib`` (drop-in mode, ``centerpose_amd/`` on sys.path):
# the compute bindings are always imported by their absolute name.
_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.append(_root)
