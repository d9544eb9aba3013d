"""What the training layers share (``conv.py``, ``stem.py``, ``deconv.py``, ``norm.py``, ``sync_norm.py``, ``group_norm.py``,
``pool.py``, ``upsample.py``, ``conv_gru.py``): the NHWC view of a logical NCHW tensor, the device gate, the "same on both axes"
rule of the geometry arguments, the in-place re-class walk behind every ``use_hip_*``, and the name check and the walk
behind every ``set_backward_precision`` (``conv.py``, ``deconv.py``, ``pose_heads.py``, ``DCNv2/dcn_v2.py``).
"""
from .hip import _abi

_on_device = _abi._on_device  # raises unless every tensor lives on the HIP device (there is no CPU path)


def _nhwc(t):
    """Logical [B,C,H,W] tensor -> its values as a contiguous [B,H,W,C] tensor (no copy when it is channels_last already)."""
    return _abi._nhwc_view(t).permute(0, 2, 3, 1)


def _same(v):
    """Is ``v`` one number, or a pair with the same number on both axes?"""
    return not isinstance(v, (tuple, list)) or (len(v) == 2 and v[0] == v[1])


def _one(v, op, what):
    """The geometry argument ``what`` of the operator ``op`` -- a number, or a pair that is the same on both axes -- as an int."""
    if isinstance(v, str):
        raise NotImplementedError("%s: string %s is not built" % (op, what))
    if not _same(v):
        raise NotImplementedError("%s: %s must be the same on both axes, got %r" % (op, what, tuple(v)))
    return int(v[0] if isinstance(v, (tuple, list)) else v)


def _precision_name(name):
    """``name`` if it is a precision a backward pass can run in ("f32", "f16x3"); ValueError otherwise."""
    if name not in _abi.PRECISIONS:
        raise ValueError("backward_precision must be one of %s, got %r" % (sorted(_abi.PRECISIONS), name))
    return name


def _set_backward_precision(module, name, targets):
    """The walk of every ``set_backward_precision``: check ``name``, then for each module ``m`` under ``module`` (itself
    included) set ``name`` on every ``(object, attribute)`` pair that ``targets(m)`` yields.  Returns how many were set."""
    name = _precision_name(name)
    n = 0
    for m in module.modules():
        for obj, attr in targets(m):
            setattr(obj, attr, name)
            n += 1
    return n


def _reclass(module, sources, target, refusal, also=(), of="", unbuilt=(), converted_hook=None):
    """The walk of every ``use_hip_*``: re-class each module under ``module`` (itself included) whose exact type is one of
    ``sources`` to ``target`` in place, unless ``refusal(m)`` gives a reason.  Returns ``(converted, skipped)``: the converted
    modules' names and ``{name: reason}`` for the layers of that kind left alone -- the refused ones, the subclasses of
    ``sources`` and ``also`` (they keep their own forward; ``of`` names the base class in the reason) and the instances of a
    class in ``unbuilt`` ((class, reason) pairs).  A module that already is a ``target`` appears in neither, and no other kind
    of module is mentioned or touched.  ``converted_hook(m)`` runs on each module right after its re-class."""
    converted, skipped = [], {}
    for name, m in module.named_modules():
        if isinstance(m, target):
            continue
        if type(m) in sources:
            why = refusal(m)
            if why:
                skipped[name] = why
                continue
            m.__class__ = target
            if converted_hook:
                converted_hook(m)
            converted.append(name)
        elif isinstance(m, tuple(sources) + tuple(also)):
            skipped[name] = "subclass %s%s keeps its own forward" % (type(m).__name__, of)
        else:
            skipped.update({name: why for cls, why in unbuilt if isinstance(m, cls)})
    return converted, skipped
