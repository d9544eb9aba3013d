"""The Objectron box metrics on the device (cp_box_iou, cp_box_eval)."""
import torch

from . import _abi

BOX_EVAL_STRIDE = 9  # CP_BOX_EVAL_STRIDE
BOX_EVAL_FIELDS = ("iou", "add", "adds", "azimuth", "polar", "pixel", "best3d", "best2d", "flags")
BOX_FLAG_SINGULAR_RAY, BOX_FLAG_SINGULAR_MO2C, BOX_FLAG_CLIP_OVERFLOW = 1, 2, 4


def _box_upload(arrays, device):
    """(array, shape, dtype) host arrays (numpy or CPU tensors) -> typed views of ONE device byte buffer, filled by one
    host-to-device copy: each array's bytes go in at a 16-byte aligned offset and come back out as a tensor of its own
    dtype (``Tensor.view(dtype)`` reinterprets, it does not convert).  Device tensors are used in place."""
    import numpy as np

    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out, host, total = [None] * len(arrays), [], 0
    for i, (a, shape, dt) in enumerate(arrays):
        if isinstance(a, torch.Tensor) and a.is_cuda:
            t = a.to(getattr(torch, np.dtype(dt).name)).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError("box metrics: expected shape %s, got %s" % (shape, tuple(t.shape)))
            out[i] = t
            continue
        h = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dt)
        if h.shape != shape:
            raise ValueError("box metrics: expected shape %s, got %s" % (shape, h.shape))
        host.append((i, h, total))
        total += (h.nbytes + 15) // 16 * 16
    if host:
        buf = np.zeros(total, np.uint8)
        for _, h, o in host:
            buf[o:o + h.nbytes] = h.reshape(-1).view(np.uint8)
        dbuf = torch.from_numpy(buf).to(dev)
        for i, h, o in host:
            out[i] = dbuf[o:o + h.nbytes].view(getattr(torch, h.dtype.name)).view(h.shape)
    return out, dev


def box_iou(a, b, device=None):
    """cp_box_iou: IoU3D.IoU(Box(a[i]), Box(b[i])).iou() of the reference evaluator for every pair; a, b [N,9,3] float64
    (numpy or tensors) -> numpy float64 [N]."""
    import numpy as np

    n = int(np.shape(a)[0])
    if n == 0:
        return np.zeros(0)
    f8 = np.float64
    (da, db), dev = _box_upload([(a, (n, 9, 3), f8), (b, (n, 9, 3), f8)], device)
    iou = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _abi._check(_abi.lib().cp_box_iou(_abi._stream(), _abi._ptr(da), _abi._ptr(db), n, _abi._ptr(iou)), "cp_box_iou")
        return iou.cpu().numpy()


def box_eval(pred3d, gt3d, pred2d, mo2c, proj, single_rotation=None, num_symmetry=1, device=None):
    """cp_box_eval: evaluate_3d + evaluate_2d of the reference evaluator for N matched pairs in one launch.
    pred3d, gt3d [N,9,3], pred2d [N,9,2], mo2c, proj [N,4,4] float64; single_rotation [N] (nonzero: index 0 only, the mug
    break).  Returns numpy float64 [N, BOX_EVAL_STRIDE], columns BOX_EVAL_FIELDS."""
    import numpy as np

    n = int(np.shape(pred3d)[0])
    if n == 0:
        return np.zeros((0, BOX_EVAL_STRIDE))
    if num_symmetry < 1:
        raise ValueError("box_eval: num_symmetry must be >= 1")
    single = np.zeros(n, np.int32) if single_rotation is None else np.asarray(single_rotation).astype(np.int32)
    if single.shape != (n,):
        raise ValueError("box_eval: single_rotation must have shape (%d,)" % n)
    f8 = np.float64
    bufs, dev = _box_upload([(pred3d, (n, 9, 3), f8), (gt3d, (n, 9, 3), f8), (pred2d, (n, 9, 2), f8),
                             (mo2c, (n, 4, 4), f8), (proj, (n, 4, 4), f8), (single, (n,), np.int32)], device)
    out = torch.empty((n, BOX_EVAL_STRIDE), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _abi._check(_abi.lib().cp_box_eval(_abi._stream(), *_abi._ptrs(*bufs), n, int(num_symmetry), _abi._ptr(out)), "cp_box_eval")
        return out.cpu().numpy()
