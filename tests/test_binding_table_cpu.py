"""The binding package against what it must not drift from (no device, no built library): its signature table against the
text of the two headers, its public surface against tests/golden/hip_public_surface.json (recorded from the one-module
binding it replaced, tools/make_hip_surface_golden.py), and its single copy of the mutable state and of the stub point."""
import ctypes
import json
import os
import re
from collections import OrderedDict

import pytest
import torch

from centerpose_amd import hip

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
           "int64_t": ctypes.c_int64}


def _declarations():
    """{name: (return text, [parameter text])} of every ``cp_name(args);`` in the two headers."""
    out = {}
    for header in ("centerpose_hip.h", "centerpose_hip_testing.h"):
        text = open(os.path.join(REPO, "include", header)).read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        text = re.sub(r"^\s*#.*$", ";", text, flags=re.M)
        for ret, name, args in re.findall(r"(?:^|[;{}])\s*([\w \t\n\*]+?)\s*\b(cp_[a-z0-9_]+)\s*\(([^()]*)\)\s*(?=;)", text):
            assert name not in out, name
            args = " ".join(args.split())
            out[name] = (" ".join(ret.split()), [] if args == "void" else [a.strip() for a in args.split(",")])
    return out


def _header_kind(text, parameter):
    """The kind of a parameter (its name is the last word) or of a return type, by the rules of the binding."""
    if "*" in text or "[" in text or "cp_stream_t" in text:
        return "pointer"
    words = [w for w in text.split() if w != "const"]
    words = words[:-1] if parameter else words
    assert len(words) == 1 and (words[0] in SCALARS or (words[0] == "void" and not parameter)), "no rule for %r" % text
    return words[0]


def _table_kind(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    kinds = [k for k, c in SCALARS.items() if c is t]
    assert len(kinds) == 1, "no rule for %r" % (t,)
    return kinds[0]


def test_signature_table_agrees_with_the_headers():
    declared, table = _declarations(), hip._abi.SIGNATURES
    assert len(declared) >= 101 and set(declared) == set(table), sorted(set(declared) ^ set(table))
    assert hip.exported_symbols() == list(table)
    for name, (ret, params) in declared.items():
        restype, argtypes = table[name]
        assert _table_kind(restype) == _header_kind(ret, False), name
        assert len(argtypes) == len(params), "%s: %d arguments bound, %d declared" % (name, len(argtypes), len(params))
        for i, (t, p) in enumerate(zip(argtypes, params)):
            assert _table_kind(t) == _header_kind(p, True), "%s: argument %d (%s)" % (name, i, p)


def test_a_kind_the_rules_do_not_know_fails():
    with pytest.raises(AssertionError, match="no rule"):
        _header_kind("long n", True)
    with pytest.raises(AssertionError, match="no rule"):
        _header_kind("void x", True)
    with pytest.raises(AssertionError, match="no rule"):
        _table_kind(ctypes.c_long if ctypes.c_long is not ctypes.c_int64 else ctypes.c_short)
    assert _header_kind("const unsigned char* image", True) == _header_kind("cp_stream_t stream", True) == "pointer"
    assert _header_kind("const char*", False) == "pointer" and _header_kind("void", False) == "void"


def test_public_surface_is_the_recorded_one():
    from tools.make_hip_surface_golden import PATH, surface

    want = json.load(open(PATH))
    if os.environ.get("CENTERPOSE_HIP_LIB"):
        want["constants"]["LIB_PATH"] = os.path.relpath(os.environ["CENTERPOSE_HIP_LIB"], REPO).replace(os.sep, "/")
    got = json.loads(json.dumps(surface(hip)))
    assert sum(len(v) for v in want.values()) == 127
    for kind in ("functions", "classes", "constants"):
        assert sorted(got[kind]) == sorted(want[kind]), (kind, sorted(set(got[kind]) ^ set(want[kind])))
        for name in want[kind]:
            assert got[kind][name] == want[kind][name], name
    assert os.path.basename(hip.LIB_PATH) == "libcenterpose_hip.so" or os.environ.get("CENTERPOSE_HIP_LIB")
    assert os.path.dirname(hip.LIB_PATH) == os.path.join(REPO, "centerpose_amd") or os.environ.get("CENTERPOSE_HIP_LIB")


def test_the_package_file_only_re_exports():
    import ast

    tree = ast.parse(open(os.path.join(REPO, "centerpose_amd", "hip", "__init__.py")).read())
    assert all(isinstance(n, (ast.ImportFrom, ast.Expr)) for n in tree.body)   # (the one expression is the docstring)
    assert not os.path.exists(os.path.join(REPO, "centerpose_amd", "hip.py"))


class _Reached(Exception):
    pass


def test_one_deterministic_flag(monkeypatch):
    """set_deterministic() is seen by deterministic() and by dcn_v2_backward, whose resolve_deterministic gets it as own_flag."""
    seen = []

    def record(requested, fast, own_flag, *rest):
        seen.append((requested, fast, own_flag))
        raise _Reached()

    monkeypatch.setattr(hip._abi, "lib", lambda: None)
    monkeypatch.setattr(hip._abi, "_dev", lambda t: t)
    monkeypatch.setattr(hip.ops, "resolve_deterministic", record)
    B, C, Co, H, W = 1, 16, 4, 5, 6
    args = (torch.zeros(B, C, H, W), torch.zeros(Co, C, 3, 3), torch.zeros(Co), torch.zeros(B, 18, H, W), torch.zeros(B, 9, H, W),
            torch.zeros(B, Co, H, W), 3, 3, 1, 1, 1, 1, 1, 1, 1)
    assert hip.deterministic() is False
    prev = hip.set_deterministic(True)
    try:
        assert prev is False and hip.deterministic() is True and hip.ops.deterministic() is True
        with pytest.raises(_Reached):
            hip.dcn_v2_backward(*args)
        with pytest.raises(_Reached):
            hip.dcn_v2_backward(*args, deterministic=False)
    finally:
        assert hip.set_deterministic(prev) is True
    with pytest.raises(_Reached):
        hip.dcn_v2_backward(*args)
    assert seen == [(None, True, True), (False, True, True), (None, True, False)] and hip.deterministic() is False


def test_one_stub_point(monkeypatch):
    """Replacing ``lib`` and ``_stream`` in ``hip._abi`` is what a LazyHeads built through ``hip.LazyHeads`` calls."""
    class Lib(object):
        calls = 0

        def cp_model_dense_heads(self, h, stream, ptrs):
            assert stream == "the stub's stream"
            Lib.calls += 1
            return 0

    class Model(object):
        _det_gen, _h = 1, None

    monkeypatch.setattr(hip._abi, "lib", Lib)
    monkeypatch.setattr(hip._abi, "_stream", lambda: "the stub's stream")
    shapes = OrderedDict([("hm", (1, 1, 2, 2)), ("wh", (1, 2, 2, 2))])
    z = hip.LazyHeads(Model(), 1, shapes, {"hm": torch.zeros(1, 1, 2, 2)}, {}, torch.zeros(1, 9, 1),
                      torch.zeros(1, 9, 1, dtype=torch.int32))
    assert Lib.calls == 0 and z["wh"].shape == (1, 2, 2, 2) and Lib.calls == 1
    assert hip.lib is not Lib   # the package's re-export is the real loader: stubbing happens in _abi alone
