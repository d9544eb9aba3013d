"""CPU tests of the training input images (no GPU): the host build of train_inputs_common.h against the numpy
restatement tests/train_inputs_ref.py on every case, draw_color_aug's random stream and the restatement against the
reference's own color_aug (where that tree is present) and against the reference-built goldens, the record layout in
its three statements, the C ABI's refusals with no device, and the Python layer's refusal and frame packing."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from centerpose_amd import hip
from centerpose_amd.train_inputs import (EIG_VAL, EIG_VEC, FRAME_ALIGN, MEAN, STD, TrainInputs, draw_color_aug,
                                         pack_frames, pack_input)
from tests import train_input_cases as TC
from tests import train_inputs_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(REPO, "tests", "golden", "train_inputs_ref.npz")
I = hip.TI_IMG
# Colour images against the float64 restatement: each step is one or two float32 roundings on magnitudes below 16 (three
# alphas of at most 1.4 on values of at most 1, a lighting shift, a division by a std of at least 0.27); about a dozen
# roundings give roughly 12 * 16 * 2^-24 = 1.2e-5.
COLOR_TOL = 4e-5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", sorted(TC.BATCHES))
def test_host_build_equals_restatement(name):
    frames, recs, side = TC.batch(name)
    host, means = TC.host_batch(frames, recs, side)
    f32, f64 = R.batch(frames, recs, side, "f32"), R.batch(frames, recs, side, "f64")
    assert host.shape == f32.shape == (5, 3, side, side) and f32.dtype == np.float32 and f64.dtype == np.float64
    for n in range(5):
        if recs[n, I["color"]]:
            err_host, err_f32 = np.abs(host[n] - f64[n]).max(), np.abs(f32[n] - f64[n]).max()
            print("%s/%d colour: host %.3g, float32 restatement %.3g against float64" % (name, n, err_host, err_f32))
            assert err_f32 < COLOR_TOL, (n, err_f32)  # the bound holds for numpy's own float32 evaluation
            assert err_host < COLOR_TOL, (n, err_host)
        else:
            assert means[n] == 0
            assert np.array_equal(bits(host[n]), bits(f32[n])), n  # bit for bit


def test_cases_cover_what_they_name():
    frames, recs, side = TC.batch("border48")
    assert TC.border_share(frames, recs, side, 0) > 1 / 3 and TC.border_share(frames, recs, side, 4) > 1 / 3
    sing = R.image(frames[2], recs[2], side)
    assert all(len(np.unique(sing[c])) == 1 for c in range(3))  # the constant source pixel (0, 0) gives
    assert np.array_equal(R.warp_u8(frames[2], recs[2], side)[5, 7], frames[2][0, 0])
    assert recs[1, I["flipped"]] == 1 and recs[3, I["flipped"]] == 1
    orders = set()
    for name in TC.BATCHES:
        _, r, _ = TC.batch(name)
        orders |= {int(v[I["order"]]) for v in r if v[I["color"]]}
        assert len({tuple(f.shape) for f in TC.batch(name)[0]}) == 3, name  # three frame sizes in every batch
    assert orders == set(range(6))
    frames, recs, side = TC.batch("mixed48")
    assert sorted(recs[:, I["color"]].tolist()) == [0, 1, 1, 1, 1]
    inp = R.warp_u8(frames[2], recs[2], side).astype(np.float32) / 255.
    gs = R.grey(inp)
    assert (gs == gs[0, 0]).all() and TC.host_batch(frames, recs, side)[1][2] == gs[0, 0]  # gs == gs_mean everywhere
    # an order code names the operations as run: the host build and the binding agree
    L = TC.host_lib()
    for code, s in enumerate(hip.TI_ORDERS):
        assert "".join("bcs"[L.ti_host_order_op(code, i)] for i in range(3)) == s


def test_draw_color_aug_keeps_the_reference_stream():
    if not TC.reference_available():
        pytest.skip("the reference tree is not present")
    seen = set()
    with TC.reference_modules() as (image, _):
        for seed in range(12):
            rng_a, rng_b = np.random.RandomState(seed), np.random.RandomState(seed)
            py_b = random.Random(seed)
            random.seed(seed)
            inp = np.random.RandomState(100 + seed).randint(0, 256, (20, 24, 3)).astype(np.float32) / 255.
            ref = inp.copy()
            image.color_aug(rng_a, ref, EIG_VAL, EIG_VEC)
            col = draw_color_aug(rng_b, py_b)
            assert random.getstate() == py_b.getstate()
            sa, sb = rng_a.get_state(), rng_b.get_state()
            assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
            rec = pack_input(np.eye(2, 3), 20, 24, False, col)["ti_image"]
            mine = inp.copy()
            R.color(mine, rec)
            # numpy's pairwise float32 mean is the only possible difference: 2 float32 ulps of 16
            assert np.abs(mine - ref).max() <= 2 * 2.0 ** -19, seed
            seen.add(col["order"])
    assert len(seen) >= 4  # the shuffle is followed, not a fixed order


def test_restatement_equals_goldens():
    gold = np.load(GOLD)
    assert os.path.getsize(GOLD) < 400 * 1024
    for key in TC.GOLDEN_CASES:
        f, rec, out = gold[key + "/frame"], gold[key + "/ti_image"], gold[key + "/out"]
        mine = R.image(f, rec, 36)
        assert mine.dtype == out.dtype == np.float32 and mine.shape == out.shape == (3, 36, 36)
        if rec[I["color"]]:  # numpy's promotion of the scalar blend differs between its major versions
            assert np.abs(mine - out).max() < COLOR_TOL, key
        else:
            assert np.array_equal(bits(mine), bits(out)), key
    assert sum(int(gold[k + "/ti_image"][I["color"]]) for k in TC.GOLDEN_CASES) == 2
    assert sum(int(gold[k + "/ti_image"][I["flipped"]]) for k in TC.GOLDEN_CASES) >= 1


def test_symbols_and_record_layout():
    names = ["cp_train_inputs_workspace_bytes", "cp_train_inputs"]
    assert all(n in hip.exported_symbols() for n in names)
    hdr = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    for n in names:
        assert re.search(r"\b%s\(" % n, hdr), n
    common = open(os.path.join(REPO, "centerpose_amd", "csrc", "train_inputs_common.h")).read()
    for src in (hdr, common):
        assert "#define CP_TI_STRIDE %d" % hip.TI_STRIDE in src
        for k, v in hip.TI_IMG.items():
            assert "#define CP_TI_%s %d" % (k.upper(), v) in src, k
    assert max(hip.TI_IMG.values()) + 3 <= hip.TI_STRIDE
    assert hip.train_inputs_means_offset(5) == 1024 and hip.train_inputs_means_offset(32) == 6144
    assert "#define CP_ABI_VERSION %d" % hip.ABI_VERSION in hdr and hip.ABI_VERSION == 7
    L = hip.lib()
    assert L.cp_train_inputs_workspace_bytes(5, 36, 36) == 1024 + 256 + 5 * 2 * 8  # records, means, 2 slabs per image
    assert L.cp_train_inputs_workspace_bytes(0, 36, 36) == 0 and L.cp_train_inputs_workspace_bytes(1, 0, 36) == 0


def _call(recs, frames_bytes=1 << 20, frames=4096, mean=True, out=4096, N=None, side=(36, 36), ws=4096, ws_bytes=None):
    """cp_train_inputs with pointers that are never dereferenced: every call below is refused on the host."""
    L = hip.lib()
    f3 = (ctypes.c_float * 3)(0.4, 0.4, 0.4)
    N = recs.shape[0] if N is None else N
    need = L.cp_train_inputs_workspace_bytes(max(N, 1), max(side[0], 1), max(side[1], 1))
    rc = L.cp_train_inputs(None, frames, frames_bytes, recs.ctypes.data if recs is not None else None, N,
                           f3 if mean else None, f3, out, side[0], side[1], ws, need if ws_bytes is None else ws_bytes)
    return rc, L.cp_last_error().decode()


def _recs(n=2):
    r = np.stack([pack_input(np.eye(2, 3), 40, 56, False, {"order": 3, "alphas": [1.1, 0.9, 1.2], "light": np.zeros(3)}
                             )["ti_image"] for _ in range(n)])
    r[:, I["offset"]] = np.arange(n) * 40 * 56 * 3
    return r


@pytest.mark.parametrize("case, msg", [
    ("nullframes", "null pointer"), ("nullmean", "null pointer"), ("nullout", "null pointer"), ("N0", "N must be >= 1"),
    ("side0", "out_h and out_w"), ("H0", "height 0"), ("Wfrac", "width 56.5"), ("order6", "order code 6"),
    ("order-1", "order code -1"), ("orderfrac", "order code 2.5"), ("nan", "non-finite record value at 4"),
    ("inf", "non-finite record value at 13"), ("extent", "outside the frames buffer"), ("negoffset", "outside the frames buffer"),
    ("misaligned", "16-byte aligned"), ("nullws", "null workspace"), ("smallws", "workspace too small")])
def test_c_abi_refusals_without_device(case, msg):
    r, kw = _recs(), {}
    if case == "nullframes":
        kw["frames"] = None
    elif case == "nullmean":
        kw["mean"] = False
    elif case == "nullout":
        kw["out"] = None
    elif case == "N0":
        kw["N"] = 0
    elif case == "side0":
        kw["side"] = (36, 0)
    elif case == "H0":
        r[1, I["height"]] = 0
    elif case == "Wfrac":
        r[0, I["width"]] = 56.5
    elif case == "order6":
        r[1, I["order"]] = 6
    elif case == "order-1":
        r[0, I["order"]] = -1
    elif case == "orderfrac":
        r[0, I["order"]] = 2.5
    elif case == "nan":
        r[1, I["trans"] + 1] = np.nan
    elif case == "inf":
        r[0, I["alpha"] + 1] = np.inf
    elif case == "extent":
        kw["frames_bytes"] = 2 * 40 * 56 * 3 - 1
    elif case == "negoffset":
        r[0, I["offset"]] = -1
    elif case == "misaligned":
        kw["out"] = 4096 + 8
    elif case == "nullws":
        kw["ws"] = None
    elif case == "smallws":
        kw["ws_bytes"] = hip.lib().cp_train_inputs_workspace_bytes(2, 36, 36) - 1
    rc, err = _call(r, **kw)
    assert rc == hip.CP_ERR_INVALID
    assert msg in err, err


def test_null_records_refused():
    L = hip.lib()
    f3 = (ctypes.c_float * 3)(0.4, 0.4, 0.4)
    assert L.cp_train_inputs(None, 4096, 1 << 20, None, 2, f3, f3, 4096, 36, 36, 4096, 1 << 20) == hip.CP_ERR_INVALID


def test_python_refusal_and_frame_packing():
    with pytest.raises(NotImplementedError, match="new_data_augmentation"):
        TrainInputs(TC.SimpleNamespace(new_data_augmentation=True, input_res=64))
    ti = TrainInputs(TC.SimpleNamespace(new_data_augmentation=False, input_res=64))
    assert ti.res == 64 and np.array_equal(ti.mean, MEAN) and np.array_equal(ti.std, STD)
    frames, recs, _ = TC.batch("border48")
    buf, packed = pack_frames(frames, recs)
    assert buf.dtype == torch.uint8 and buf.dim() == 1
    end = 0
    for n, f in enumerate(frames):
        off = int(packed[n, I["offset"]])
        assert off % FRAME_ALIGN == 0 and off >= end  # no overlap
        assert np.array_equal(buf[off:off + f.size].numpy().reshape(f.shape), f)
        end = off + f.size
    assert buf.numel() >= end and (recs[:, I["offset"]] == 0).all()  # the caller's records are not written
    with pytest.raises(ValueError, match="its record says"):
        pack_frames(frames[::-1], recs)
    with pytest.raises(ValueError, match="one per frame"):
        pack_frames(frames[:3], recs)
    # no colour: the flag and every colour field stay clear; a colour record carries the lighting shift as float64
    rec = pack_input(np.eye(2, 3), 40, 56, True)["ti_image"]
    assert rec[I["flipped"]] == 1 and rec[I["color"]] == 0 and not rec[I["order"]:].any()
    light = np.array([0.1, -0.2, 0.05])
    rec = pack_input(np.eye(2, 3), 40, 56, False, {"order": 4, "alphas": [0.7, 1.2, 1.0], "light": light})["ti_image"]
    assert rec[I["color"]] == 1 and rec[I["order"]] == 4 and rec[I["alpha"]:I["alpha"] + 3].tolist() == [0.7, 1.2, 1.0]
    assert np.array_equal(rec[I["shift"]:I["shift"] + 3], np.dot(EIG_VEC, EIG_VAL * light))
