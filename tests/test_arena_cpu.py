"""The engine's work-space arena (centerpose_amd/csrc/engine_arena.h: Arena and Block, free of HIP includes) compiled for the
host by tests/native/arena_host.cpp and driven with random allocate / release scripts against a brute-force model: one flag
per 256-byte unit, a block goes to the lowest run of free units that holds it.

Checked after every operation: the offset is the model's (so live blocks never overlap) and 256-aligned; the free list is
exactly the model's maximal free runs in order (free neighbours coalesce, no empty or touching entries); ``peak`` is the
highest end reached; ``overflow`` is set exactly from the first block that ends beyond ``cap`` on.  A dry replay of the script
(null base, as cp_model_workspace_bytes runs it) hands out the same offsets and reports the same peak, and never sets
``overflow``: that is why the size a pass needs can be asked before it runs."""
import ctypes
import os
import subprocess
from ctypes import POINTER, byref, c_int, c_size_t, c_void_p

import numpy as np
import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
UNIT = 256
OPEN_END = 1 << 62   # the arena's free space is one run of 2^62 bytes from offset 0


@pytest.fixture(scope="module")
def host():
    out = os.path.join(REPO, "tests", "_build", "libcp_arena_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(REPO, "tests", "native", "arena_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", out])
    lib = ctypes.CDLL(out)
    lib.arena_host_new.restype, lib.arena_host_new.argtypes = c_void_p, [c_int, c_size_t]
    lib.arena_host_delete.restype, lib.arena_host_delete.argtypes = None, [c_void_p]
    lib.arena_host_alloc.restype, lib.arena_host_alloc.argtypes = c_int, [c_void_p, c_size_t, POINTER(c_size_t)]
    lib.arena_host_release.restype, lib.arena_host_release.argtypes = None, [c_void_p, c_int]
    lib.arena_host_state.restype = None
    lib.arena_host_state.argtypes = [c_void_p, POINTER(c_size_t), POINTER(c_int), POINTER(c_size_t), POINTER(c_int)]
    lib.arena_host_free_list.restype, lib.arena_host_free_list.argtypes = c_int, [c_void_p, POINTER(c_size_t), c_int]
    lib.arena_host_align_up.restype, lib.arena_host_align_up.argtypes = c_size_t, [c_size_t, c_size_t]
    return lib


class Model(object):
    """Brute force: used[i] says whether bytes [256 i, 256 (i + 1)) belong to a live block."""

    def __init__(self):
        self.used, self.peak = [], 0

    def alloc(self, nbytes):
        u = -(-nbytes // UNIT)
        start = 0
        while True:   # the lowest offset with u free units in a row (beyond the list everything is free)
            run = 0
            while run < u and (start + run >= len(self.used) or not self.used[start + run]):
                run += 1
            if run == u:
                break
            start += run + 1
        self.used.extend([False] * (start + u - len(self.used)))
        assert not any(self.used[start:start + u])
        self.used[start:start + u] = [True] * u
        self.peak = max(self.peak, (start + u) * UNIT)
        return start * UNIT, u * UNIT

    def release(self, off, nbytes):
        a, u = off // UNIT, nbytes // UNIT
        assert all(self.used[a:a + u])
        self.used[a:a + u] = [False] * u

    def free_runs(self):
        runs, i, n = [], 0, len(self.used)
        while i < n:
            if self.used[i]:
                i += 1
                continue
            j = i
            while j < n and not self.used[j]:
                j += 1
            runs.append([i * UNIT, (j - i) * UNIT if j < n else None])
            i = j
        if not runs or runs[-1][1] is not None:
            runs.append([n * UNIT, None])
        return runs


def _script(rng, n_ops):
    """[("a", bytes) | ("r", index of the allocating operation)]: sizes from 1 byte to 32 KiB, odd ones and exact multiples of
    256; releases in random order, so that holes open, fill and merge on both sides"""
    ops, live = [], []
    for i in range(n_ops):
        if live and rng.rand() < 0.47:
            ops.append(("r", live.pop(rng.randint(len(live)))))
        else:
            kind = rng.randint(4)
            size = int([rng.randint(1, 257), UNIT * rng.randint(1, 9), rng.randint(1, 20000), rng.randint(1, 1 << 15)][kind])
            ops.append(("a", size))
            live.append(i)
    return ops


def _state(host, h):
    peak, ovf, cap, base = c_size_t(), c_int(), c_size_t(), c_int()
    host.arena_host_state(h, byref(peak), byref(ovf), byref(cap), byref(base))
    buf = (c_size_t * 4096)()
    n = host.arena_host_free_list(h, buf, 2048)
    assert n <= 2048
    return peak.value, bool(ovf.value), [[buf[2 * i], buf[2 * i + 1]] for i in range(n)]


def _replay(host, ops, real, cap, check):
    """Runs the script -> (offsets per allocating operation, peak, overflow); with ``check`` every step is held to the model"""
    h = host.arena_host_new(int(real), cap)
    model, ids, blocks, offs, over = Model(), {}, {}, {}, False
    try:
        for i, (op, arg) in enumerate(ops):
            if op == "a":
                off = c_size_t()
                ids[i] = host.arena_host_alloc(h, arg, byref(off))
                offs[i] = off.value
                want_off, size = model.alloc(arg)
                blocks[i] = (want_off, size)
                over = over or (real and want_off + size > cap)
                if check:
                    assert off.value == want_off and off.value % UNIT == 0, (i, arg, off.value, want_off)
                    assert size == host.arena_host_align_up(arg, UNIT)
            else:
                host.arena_host_release(h, ids.pop(arg))
                model.release(*blocks.pop(arg))
            if check:
                peak, ovf, free = _state(host, h)
                want = model.free_runs()
                assert [f[0] for f in free] == [w[0] for w in want], (i, free[:6], want[:6])
                for f, w in zip(free, want):   # (the open end: what is left of the 2^62 bytes)
                    assert f[1] == (w[1] if w[1] is not None else OPEN_END - w[0]), (i, f, w)
                assert peak == model.peak, (i, peak, model.peak)
                assert ovf == over, "operation %d: overflow %s, a block ended beyond cap: %s" % (i, ovf, over)
        peak, ovf, _ = _state(host, h)
        return offs, peak, ovf
    finally:
        host.arena_host_delete(h)


@pytest.mark.parametrize("seed", range(6))
def test_random_scripts_against_the_interval_model(host, seed):
    rng = np.random.RandomState(100 + seed)
    ops = _script(rng, 300)
    _, dry_peak, dry_ovf = _replay(host, ops, False, 0, check=True)
    assert not dry_ovf and dry_peak > 0
    # a real pass over exactly the dry peak never overflows; one block short of it does, from the block that crosses on
    offs, peak, ovf = _replay(host, ops, True, dry_peak, check=True)
    assert (peak, ovf) == (dry_peak, False)
    offs_short, peak_short, ovf_short = _replay(host, ops, True, dry_peak - UNIT, check=True)
    assert ovf_short and peak_short == dry_peak and offs_short == offs   # offsets beyond cap are handed out all the same
    _, _, ovf_half = _replay(host, ops, True, dry_peak // 2, check=True)
    assert ovf_half
    assert _replay(host, ops, False, 0, check=False)[0] == offs          # the dry pass places every block where the real one does


def test_everything_released_leaves_one_free_run(host):
    """The engine resets the arena per pass, but a pass releases every tensor before it ends: the free list is whole again."""
    rng = np.random.RandomState(7)
    ops = _script(rng, 300)
    ops += [("r", i) for i in sorted({i for i, o in enumerate(ops) if o[0] == "a"} - {o[1] for o in ops if o[0] == "r"})]
    h = host.arena_host_new(1, 1 << 30)
    ids = {}
    for i, (op, arg) in enumerate(ops):
        if op == "a":
            ids[i] = host.arena_host_alloc(h, arg, byref(c_size_t()))
        else:
            host.arena_host_release(h, ids.pop(arg))
    _, ovf, free = _state(host, h)
    host.arena_host_delete(h)
    assert free == [[0, OPEN_END]] and not ovf
