"""Writes tests/golden/hip_public_surface.json: every public name of ``centerpose_amd.hip`` with what a caller can see of
it -- the signature of a function and of a class's public methods, the value of a constant, the ``_fields_`` of a
ctypes.Structure, the members of KernelSel.  tests/test_binding_table_cpu.py recomputes ``surface()`` and compares.  Run
it on the commit whose surface is to be kept (no device, no built library needed).

  python tools/make_hip_surface_golden.py
"""
import ctypes
import enum
import inspect
import json
import os
import sys
import types
from collections import OrderedDict

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

PATH = os.path.join(REPO, "tests", "golden", "hip_public_surface.json")


def _value(v):
    if isinstance(v, OrderedDict):
        return {"ordered": [[k, _value(x)] for k, x in v.items()]}
    if isinstance(v, dict):
        return {"dict": [[k, _value(x)] for k, x in v.items()]}
    if isinstance(v, (tuple, list)):
        return [_value(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError("hip surface: a public constant of type %s" % type(v).__name__)


def _class(c):
    d = {"bases": [b.__name__ for b in c.__bases__]}
    if issubclass(c, ctypes.Structure):
        d["fields"] = [[n, t.__name__] for n, t in c._fields_]
    if issubclass(c, enum.Enum):
        d["members"] = [[m.name, int(m.value)] for m in c]
        return d
    for n, v in sorted(vars(c).items()):
        if n.startswith("_") and n not in ("__init__", "__call__"):
            continue
        if isinstance(v, types.FunctionType):
            d.setdefault("methods", {})[n] = str(inspect.signature(v))
        elif not isinstance(v, (staticmethod, classmethod, property)) and not hasattr(v, "__get__"):
            d.setdefault("attributes", {})[n] = _value(v)
    return d


def surface(hip):
    """{"functions": {name: signature}, "classes": {name: ...}, "constants": {name: value}} of the module ``hip``.  Left
    out: modules and names defined elsewhere (the ctypes / collections names the binding imports).  LIB_PATH is given
    relative to the repository."""
    out = {"functions": {}, "classes": {}, "constants": {}}
    for n in sorted(vars(hip)):
        v = getattr(hip, n)
        if n.startswith("_") or isinstance(v, types.ModuleType):
            continue
        if isinstance(v, (type, types.FunctionType)):
            if not v.__module__.startswith(hip.__name__):
                continue
            if isinstance(v, type):
                out["classes"][n] = _class(v)
            else:
                out["functions"][n] = str(inspect.signature(v))
        else:
            out["constants"][n] = os.path.relpath(v, REPO).replace(os.sep, "/") if n == "LIB_PATH" else _value(v)
    return out


def main():
    from centerpose_amd import hip

    s = surface(hip)
    with open(PATH, "w") as f:
        json.dump(s, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d bytes, %s" % (PATH, os.path.getsize(PATH), ", ".join("%d %s" % (len(v), k) for k, v in sorted(s.items()))))


if __name__ == "__main__":
    main()
