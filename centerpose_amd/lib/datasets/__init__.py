"""Mirror of the reference's ``lib.datasets``: ObjectPoseDataset (dataset_combined) and the loader's collate function
(dataset_factory)."""
