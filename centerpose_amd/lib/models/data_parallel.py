"""The name the reference's entry points import (``from lib.models.data_parallel import DataParallel``).  The reference's
class scatters one process's batch over several GPUs; this project trains with one process per GPU, so the name only
points the caller there."""

MULTI_GPU_MESSAGE = ("more than one GPU in one process is not built: start one process per GPU and wrap the network in "
                     "centerpose_amd.data_parallel.DataParallel (INTEGRATION.md, 'Training across GPUs')")


class DataParallel(object):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("lib.models.data_parallel.DataParallel: " + MULTI_GPU_MESSAGE)
