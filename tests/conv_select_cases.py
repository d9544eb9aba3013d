"""The grid of tests/golden/conv_select_grid.json, its codec and the host helper that answers it: shared by
tools/make_conv_select_golden.py (which writes the fixture from the PARENT commit's library) and tests/test_conv_select_cpu.py (which
replays it against the current one).

A row is one ConvParams as tests/native/conv_select_host.cpp fills it, named by five indices into the axes below; its answer is what
the library's selectors say about it.  The axes take the smallest values on each side of every threshold the selectors read:
B x map gives 2 ... 8192 8 x 16 patches (dcn16p's 64 blocks, dcn16t's 1024, the wide tile's 256, dcn16s's 4096 items, strm16's 1024
jobs); the channel pairs give the N tiles 16 / 32 / 64 / 128, CoutPad % 128 both ways, an offset convolution (64 -> 27), a <= 16-wide
head packed to 32 columns and unaligned input channels for the float32 stems."""
import ctypes
import os
import subprocess

import numpy as np

from centerpose_amd import hip

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
S = hip.KernelSel
F_OFFMASK, F_W16, F_W16F, F_GN, F_PJ = 1, 2, 4, 8, 16
ACT_NONE, ACT_RELU, ACT_SIGMOID_FROM = 0, 1, 3

BATCHES = [1, 2, 64]
MAPS = [16, 32, 64, 128]
# (Cin, Cout, least CoutPad, activation)
PAIRS = [(64, 27, 0, ACT_SIGMOID_FROM), (64, 16, 32, ACT_NONE), (64, 16, 0, ACT_RELU), (64, 32, 0, ACT_RELU), (64, 64, 0, ACT_RELU),
         (128, 64, 0, ACT_RELU), (64, 128, 0, ACT_RELU), (128, 128, 0, ACT_RELU), (256, 256, 0, ACT_RELU), (64, 192, 0, ACT_RELU),
         (32, 64, 0, ACT_RELU), (12, 16, 0, ACT_RELU), (12, 32, 0, ACT_RELU), (12, 64, 0, ACT_RELU), (12, 128, 0, ACT_RELU)]
# (kernel, stride, sources, flags): 1x1 s1, 3x3 s1, 3x3 s2, each over one source and over a virtual concat of two; the GroupNorm'd 1x1;
# the DCN and the fused projection on the one geometry their launchers accept
CONFIGS = [(1, 1, 1, 0), (1, 1, 2, 0), (1, 1, 1, F_GN), (3, 1, 1, 0), (3, 1, 2, 0), (3, 1, 1, F_OFFMASK), (3, 1, 1, F_PJ), (3, 2, 1, 0),
           (3, 2, 2, 0)]
# (fragment-ordered weights, tile_m = tile_n = 64, split-K slices)
WEIGHTS_TILING = [(1, 0, 1), (1, 1, 1), (1, 1, 4), (1, 0, 4), (0, 0, 1), (0, 1, 1)]
# 0, every single switch igemm.hip, igemm16.hip, dcn16p.hip, halo16.hip, pw16.hip or strm16.hip reads, and the two combinations of
# tests/engine_plan_cases.py
SELS = [0, S.HALO_NEVER, S.HALO_ALWAYS, S.HALO_LDS_WEIGHTS, S.STRM16_NEVER, S.STRM16_ALWAYS, S.PW16_NEVER, S.PW16_FRAG_A,
        S.DCN16P_NEVER, S.DCN16P_ALWAYS, S.DCN16P_NOT_WIDE, S.DCN16S_NEVER, S.DCN16S_ALWAYS, S.DCN16T_ALWAYS, S.DCN16T_NEVER,
        S.SPLITK_ELEMENTWISE, S.DCN16P_ALWAYS | S.DCN16T_ALWAYS, S.PW16_FRAG_A | S.LEVEL1_ROWS_NEVER]
SELS = [int(s) for s in SELS]
AXES = dict(batch=BATCHES, map=MAPS, pair=[list(p) for p in PAIRS], config=[list(c) for c in CONFIGS],
            weights_tiling=[list(w) for w in WEIGHTS_TILING], sel=SELS)
OUT_FIELDS = ["conv_variant", "conv16_supported", "conv16_variant", "conv16_project_supported", "tiles_f32", "ksteps_f32",
              "tiles_f16x3", "ksteps_f16x3"]
FULL_SEL_AT = (2, 64)  # every switch set against every configuration here; elsewhere only the switches the configuration's kernels read

_ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz-_"
ROW_CHARS = 6  # pair, config, weights_tiling, sel, answer (two digits, most significant first)


def _cout_pad(cout, least):
    bn = 16 if cout <= 16 else 32 if cout <= 32 else 128 if cout % 128 == 0 else 64
    return max((cout + bn - 1) // bn * bn, least)


def _has_w16(pair):
    cin, cout, least, _ = pair
    return cin % 32 == 0 and _cout_pad(cout, least) >= 32  # (the packer's rule for making split-f16 weights)


def _sels_read(config):
    k, stride, _, flags = config
    if flags & F_OFFMASK:
        names = [S.DCN16P_NEVER, S.DCN16P_ALWAYS, S.DCN16P_NOT_WIDE, S.DCN16S_NEVER, S.DCN16S_ALWAYS, S.DCN16T_ALWAYS, S.DCN16T_NEVER,
                 S.DCN16P_ALWAYS | S.DCN16T_ALWAYS]
    elif k == 3 and stride == 1:
        names = [S.HALO_NEVER, S.HALO_ALWAYS, S.HALO_LDS_WEIGHTS, S.STRM16_NEVER, S.STRM16_ALWAYS]
    elif k == 3:
        names = [S.HALO_ALWAYS]
    else:
        names = [S.PW16_NEVER, S.PW16_FRAG_A, S.PW16_FRAG_A | S.LEVEL1_ROWS_NEVER]
    return [0] + [int(n) for n in names]


def grid(batch, hw):
    """-> the (pair, config, weights_tiling, sel) index rows of one (B, map).  Pruned: what cannot matter is not crossed -- pairs
    without split-f16 weights (only the float32 selector looks at them) meet neither tiling, switches, GroupNorm nor projection;
    64 x 64 tiles need CoutPad % 64 == 0 (the planner's rule); the split-K crossings are made with fragment-ordered weights only."""
    rows = []
    for ip, pair in enumerate(PAIRS):
        w16 = _has_w16(pair)
        for ic, config in enumerate(CONFIGS):
            if not w16 and config[3] & (F_GN | F_PJ):
                continue
            sels = SELS if (batch, hw) == FULL_SEL_AT else _sels_read(config)
            for iw, (w16f, tile64, splitk) in enumerate(WEIGHTS_TILING):
                if not w16 and iw != WEIGHTS_TILING.index((0, 0, 1)):
                    continue
                if tile64 and _cout_pad(pair[1], pair[2]) % 64 != 0:
                    continue
                for sel in (sels if w16 else [0]):
                    rows.append((ip, ic, iw, SELS.index(sel)))
    return rows


def params(batch, hw, row):
    """-> the helper's input ints of one row"""
    cin, cout, least, act = PAIRS[row[0]]
    k, stride, nsrc, flags = CONFIGS[row[1]]
    w16f, tile64, splitk = WEIGHTS_TILING[row[2]]
    if _has_w16(PAIRS[row[0]]):
        flags |= F_W16 | (F_W16F if w16f else 0)
    return [batch, hw, cin, cout, least, k, stride, nsrc, act, flags, tile64, splitk, SELS[row[3]]]


def describe(batch, hw, row):
    cin, cout, least, act = PAIRS[row[0]]
    k, stride, nsrc, flags = CONFIGS[row[1]]
    w16f, tile64, splitk = WEIGHTS_TILING[row[2]]
    return ("B=%d map=%dx%d %d->%d (CoutPad >= %d, act %d) %dx%d s%d nsrc=%d%s%s%s w16=%d w16f=%d tile64=%d splitk=%d sel=0x%08x"
            % (batch, hw, hw, cin, cout, least, act, k, k, stride, nsrc, " offmask" if flags & F_OFFMASK else "",
               " gn_in_a/d" if flags & F_GN else "", " pj_src" if flags & F_PJ else "", _has_w16(PAIRS[row[0]]), w16f, tile64, splitk,
               SELS[row[3]]))


def encode(rows, answers):
    return "".join("".join(_ALPHABET[i] for i in row) + _ALPHABET[a // 64] + _ALPHABET[a % 64] for row, a in zip(rows, answers))


def decode(text):
    """-> (rows, answer indices) of one group's string"""
    assert len(text) % ROW_CHARS == 0
    d = [_ALPHABET.index(c) for c in text]
    rows = [tuple(d[i:i + 4]) for i in range(0, len(d), ROW_CHARS)]
    return rows, [d[i + 4] * 64 + d[i + 5] for i in range(0, len(d), ROW_CHARS)]


def helper(lib_path):
    """tests/native/conv_select_host.cpp built for the host against the library at `lib_path` -> evaluate(list of input rows) ->
    int array [rows, len(OUT_FIELDS)]"""
    out = os.path.join(REPO, "tests", "_build", "libcp_conv_select_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(REPO, "tests", "native", "conv_select_host.cpp")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib_dir = os.path.dirname(os.path.abspath(lib_path))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-shared",
                           "-fPIC", src, "-o", out, os.path.abspath(lib_path), "-Wl,-rpath," + lib_dir])
    lib = ctypes.CDLL(out)
    n_in, n_out = ctypes.c_int(), ctypes.c_int()
    lib.conv_select_row_ints(ctypes.byref(n_in), ctypes.byref(n_out))
    assert n_out.value == len(OUT_FIELDS)
    lib.conv_select_eval.restype = None

    def evaluate(rows):
        a = np.ascontiguousarray(rows, dtype=np.int32)
        assert a.ndim == 2 and a.shape[1] == n_in.value
        res = np.empty((a.shape[0], n_out.value), dtype=np.int32)
        lib.conv_select_eval(a.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(a.shape[0]), res.ctypes.data_as(ctypes.c_void_p))
        return res

    return evaluate
