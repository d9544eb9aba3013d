"""The loader's collate function (datasets/dataset_factory.py of the reference) and the dataset table."""
from torch.utils.data.dataloader import default_collate

from .dataset_combined import ObjectPoseDataset

dataset_factory = {"objectron": ObjectPoseDataset}

FRAME_KEYS = ("frame", "frame_pre")  # decoded frames: Objectron mixes portrait and landscape, so they stay a list


def collate_fn_filtered(batch):
    """Drops the samples a dataset answered with None (an unreadable image) and returns None for a batch that has none
    left, as the reference's does.  The decoded frames stay Python lists of uint8 HWC arrays, one per sample
    (train_inputs.pack_frames takes lists); every other field is default-collated."""
    batch = [sample for sample in batch if sample is not None]
    if not batch:
        return None
    if not isinstance(batch[0], dict):
        return default_collate(batch)
    out = default_collate([{k: v for k, v in sample.items() if k not in FRAME_KEYS} for sample in batch])
    for k in FRAME_KEYS:
        if k in batch[0]:
            out[k] = [sample[k] for sample in batch]
    return out
