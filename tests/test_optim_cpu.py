"""CPU tests (no GPU) of the optimizer step: declarations and refusals of cp_adam_*, the table cp_adam_table_build lays out,
the constructor and state_dict of centerpose_amd.optim.Adam against torch.optim.Adam, the resume branch of
lib.models.model.load_model, and the float32 error the GPU test's limit is set against (tests/optim_ref.py)."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from centerpose_amd import hip
from centerpose_amd.optim import Adam
from tests import optim_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("cp_adam_table_bytes", "cp_adam_table_build", "cp_adam_state_bytes", "cp_adam_workspace_bytes", "cp_adam_step")


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def test_symbols_declared_exported_and_listed(built):
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and hasattr(built, name) and name in hip.exported_symbols(), name
    assert "base_trainer.py:91-99" in header and "test.py:41" in header
    assert built.cp_abi_version() == 7 == hip.ABI_VERSION and "#define CP_ABI_VERSION 7" in header
    for name, value in (("CHUNK", hip.optim.ADAM_CHUNK), ("TENSOR_BYTES", hip.optim.ADAM_TENSOR_BYTES),
                        ("CHUNK_BYTES", hip.optim.ADAM_CHUNK_BYTES), ("VEC", hip.optim.ADAM_VEC),
                        ("SKIP_NONFINITE", hip.optim.ADAM_SKIP_NONFINITE), ("STATE_NORM", hip.optim.ADAM_STATE_NORM),
                        ("STATE_COEF", hip.optim.ADAM_STATE_COEF), ("STATE_SKIPPED", hip.optim.ADAM_STATE_SKIPPED),
                        ("STATE_STEPS", hip.optim.ADAM_STATE_STEPS)):
        assert re.search(r"#define CP_ADAM_%s %d\n" % (name, value), header), name
    for n in (1, 2, 3, 250):
        assert built.cp_adam_state_bytes(n) == hip.optim.adam_state_bc_offset(n) + 16 * n and hip.optim.adam_state_bc_offset(n) % 8 == 0
        assert hip.optim.adam_state_bc_offset(n) >= 16 + 4 * n
    assert not hasattr(hip, "adam_step")   # the recorded surface of `hip` stays as it is: callers use hip.optim.adam_step


def _arrays(lengths, addresses=None, active=None):
    a = hip.optim.AdamArrays(len(lengths))
    for i, n in enumerate(lengths):
        a.lengths[i] = n
        a.active[i] = 1 if active is None else active[i]
        for j, arr in enumerate((a.p, a.g, a.m, a.v)):
            arr[i] = addresses[i][j] if addresses is not None else 0x10000 * (4 * i + j + 1)
    return a


def test_refusals_without_a_device(built):
    p = ctypes.c_void_p(0x1000)

    def step(table=p, n_tensors=3, n_chunks=5, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, max_norm=100.0, flags=0, state=p,
             ws=p, ws_bytes=4096):
        return built.cp_adam_step(None, table, n_tensors, n_chunks, lr, beta1, beta2, eps, wd, max_norm, flags, state, ws, ws_bytes)

    def refused(text, **kw):
        assert step(**kw) == hip.CP_ERR_INVALID and text in built.cp_last_error(), (kw, built.cp_last_error())

    for kw in (dict(table=None), dict(state=None), dict(ws=None)):
        refused(b"null argument", **kw)
    refused(b"n_tensors must be >= 1", n_tensors=0)
    refused(b"n_chunks must be >= 0", n_chunks=-1)
    refused(b"8-byte aligned", state=ctypes.c_void_p(0x1004))
    refused(b"lr must be >= 0", lr=-1e-3)
    for kw in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=1.5)):
        refused(b"betas must lie in [0, 1)", **kw)
    refused(b"eps must be >= 0", eps=-1e-8)
    refused(b"weight_decay must be >= 0", wd=-1e-2)
    for name in ("lr", "beta1", "beta2", "eps", "wd", "max_norm"):
        for bad in (float("nan"), float("inf")):
            refused(b"non-finite hyper-parameter", **{name: bad})
    refused(b"unknown flag", flags=2)
    assert built.cp_adam_workspace_bytes(5) >= 5 * 8 and built.cp_adam_workspace_bytes(-1) == 0 and built.cp_adam_state_bytes(0) == 0
    refused(b"workspace too small", ws_bytes=built.cp_adam_workspace_bytes(5) - 1)
    refused(b"workspace too small", n_chunks=1000, ws_bytes=4096)

    # the table: lengths, totals, pointers, the buffer
    n_chunks = ctypes.c_int(-7)
    for lengths, text in (((5, -1), b"length -1"), ((1 << 31, 1), b"2^31 elements"), (((1 << 31) + 1,), b"2^31 elements")):
        a = _arrays(lengths)
        assert built.cp_adam_table_bytes(a.n, a.lengths, a.active, ctypes.byref(n_chunks)) == 0 and text in built.cp_last_error()
        with pytest.raises(ValueError):
            hip.optim.adam_table_bytes(a)
    a = _arrays((1 << 31,))   # exactly 2^31 elements are accepted
    assert hip.optim.adam_table_bytes(a) == (48 + 16 * (1 << 19), 1 << 19)
    a = _arrays((5, 6))
    assert built.cp_adam_table_bytes(0, a.lengths, a.active, ctypes.byref(n_chunks)) == 0 and b"n_tensors" in built.cp_last_error()
    assert built.cp_adam_table_bytes(2, None, a.active, ctypes.byref(n_chunks)) == 0 and b"null" in built.cp_last_error()
    assert built.cp_adam_table_bytes(2, a.lengths, a.active, None) == 0 and b"null" in built.cp_last_error()
    nbytes, _ = hip.optim.adam_table_bytes(a)
    assert nbytes == 2 * 48 + 2 * 16
    buf = torch.zeros(nbytes, dtype=torch.uint8)
    with pytest.raises(ValueError, match="table buffer too small"):
        hip.optim.adam_table_build(buf[:nbytes - 1], a)
    with pytest.raises(ValueError, match="null or misaligned"):
        hip.optim.adam_table_build(buf, _arrays((5, 6), addresses=[(16, 32, 48, 64), (16, 0, 48, 64)]))
    with pytest.raises(ValueError, match="null or misaligned"):
        hip.optim.adam_table_build(buf, _arrays((5, 6), addresses=[(16, 32, 48, 66), (16, 32, 48, 64)]))
    args = (ctypes.c_void_p(buf.data_ptr()), nbytes, 2, a.p, a.g, a.m, a.v, a.lengths, a.active, ctypes.byref(n_chunks))
    for i in (0, 3, 4, 5, 6, 7, 9):
        bad = list(args)
        bad[i] = None
        assert built.cp_adam_table_build(*bad) == hip.CP_ERR_INVALID and b"null" in built.cp_last_error(), i
    # an inactive tensor's pointers are not looked at; an empty tensor's neither
    assert hip.optim.adam_table_build(buf, _arrays((5, 0), addresses=[(16, 32, 48, 64), (0, 0, 0, 0)])) == 1
    assert hip.optim.adam_table_build(buf, _arrays((5, 6), addresses=[(16, 32, 48, 64), (0, 0, 0, 0)], active=(1, 0))) == 1


def _parse(buf, n_tensors, n_chunks):
    raw = buf.numpy()
    tensors = raw[:48 * n_tensors].view(np.int64).reshape(n_tensors, 6)
    chunks = raw[48 * n_tensors:48 * n_tensors + 16 * n_chunks].view(np.int32).reshape(n_chunks, 4)
    return tensors, chunks


def test_table_covers_every_element_once(built):
    c = R.case()
    lengths = [c.params[k].numel() for k in c.names]
    active = [0 if k == "no_grad" else 1 for k in c.names]
    # synthetic addresses: 256-byte aligned, except one array each of four tensors (a different array each time) and all
    # four arrays of a fifth, by 4, 8 or 12 bytes
    addresses, odd = [], {}
    for i, n in enumerate(lengths):
        row = [0x100000 * (4 * i + j + 1) for j in range(4)]
        if c.names[i] in ("len5", "len1025", "len4097", "len12289"):
            j = len(odd)
            row[j] += (4, 8, 12, 4)[j]
            odd[i] = True
        if c.names[i] == "unaligned":
            row = [x + 4 for x in row]
            odd[i] = True
        addresses.append(row)
    assert len(odd) == 5
    a = _arrays(lengths, addresses, active)
    nbytes, n_chunks = hip.optim.adam_table_bytes(a)
    buf = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8)
    assert hip.optim.adam_table_build(buf[:nbytes], a) == n_chunks
    assert bool((buf[nbytes:] == 0xAB).all())   # nothing written past the table
    tensors, chunks = _parse(buf, len(lengths), n_chunks)
    for i, n in enumerate(lengths):
        assert list(tensors[i, :4]) == addresses[i] and tensors[i, 4] == n and tensors[i, 5] == active[i], i
    covered = [np.zeros(n, dtype=np.int32) for n in lengths]
    last = (-1, -1)
    for t, start, count, flags in chunks:
        start = int(np.uint32(start))
        assert 0 <= t < len(lengths) and active[t] and 1 <= count <= hip.optim.ADAM_CHUNK and start % hip.optim.ADAM_CHUNK == 0
        assert start + count <= lengths[t]                       # no chunk crosses its tensor's end
        assert (t, start) > last                                 # tensor order, ascending within a tensor
        last = (t, start)
        assert flags == (0 if t in odd else hip.optim.ADAM_VEC), (c.names[t], flags)
        covered[t][start:start + count] += 1
    for i, n in enumerate(lengths):
        assert bool((covered[i] == active[i]).all()), c.names[i]   # every element of an active tensor exactly once
    per_tensor = np.bincount(chunks[:, 0], minlength=len(lengths))
    assert per_tensor[c.names.index("empty")] == 0 and per_tensor[c.names.index("no_grad")] == 0
    assert per_tensor[c.names.index("len4096")] == 1 and per_tensor[c.names.index("len4097")] == 2
    assert per_tensor[c.names.index("len12289")] == 4 and n_chunks == int(per_tensor.sum())
    # with every tensor 16-byte aligned every chunk takes the vector path
    a = _arrays(lengths, None, active)
    assert hip.optim.adam_table_build(buf[:nbytes], a) == n_chunks
    assert bool((_parse(buf, len(lengths), n_chunks)[1][:, 3] == hip.optim.ADAM_VEC).all())


def test_no_cpu_path(built):
    t = torch.zeros(256, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.optim.adam_step(t, 1, 1, t, 1e-3, 0.9, 0.999, 1e-8, 0.0, 100.0)
    p = torch.nn.Parameter(torch.zeros(5))
    p.grad = torch.ones(5)
    opt = Adam([p], lr=0.1, max_grad_norm=100.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        opt.step()
    assert bool((p == 0).all()) and len(opt.state) == 0 and opt.last_grad_norm is None


def test_constructor_refusals():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for name in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=name):
            Adam(p, **{name: True})
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match="float32"):
            Adam([torch.nn.Parameter(torch.zeros(3, dtype=dtype))])
    with pytest.raises(NotImplementedError, match="non-dense"):
        Adam([torch.nn.Parameter(torch.zeros(8, 8)[:, :3])])
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0),
               dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            Adam(p, **kw)
    with pytest.raises(TypeError):
        Adam(p, nesterov=True)
    with pytest.raises(ValueError):
        Adam([])
    opt = Adam(p, lr=1.25e-4, max_grad_norm=100.0)
    assert isinstance(opt, torch.optim.Optimizer) and opt.layout_copies == 0
    ours, theirs = opt.param_groups[0], torch.optim.Adam(p, lr=1.25e-4).param_groups[0]
    assert list(ours)[:len(theirs)] == list(theirs) and list(ours)[len(theirs):] == ["max_grad_norm", "skip_nonfinite"]
    assert all(ours[k] == theirs[k] for k in theirs if k != "params") and ours["max_grad_norm"] == 100.0 and ours["skip_nonfinite"] is False
    # amsgrad arriving through a loaded state dict is refused as well
    sd = torch.optim.Adam(p, amsgrad=True).state_dict()
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.load_state_dict(sd)


def _cpu_params(seed):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(5, 3, generator=g)), torch.nn.Parameter(torch.randn(7, generator=g)),
          torch.nn.Parameter(torch.randn(2, 3, 4, 5, generator=g).contiguous(memory_format=torch.channels_last)),
          torch.nn.Parameter(torch.randn(4, generator=g))]
    return ps


def _assert_same_state_dict(a, b):
    assert a["param_groups"][0]["params"] == b["param_groups"][0]["params"]
    assert list(a["state"]) == list(b["state"])
    for i in a["state"]:
        assert list(a["state"][i]) == list(b["state"][i]) == ["step", "exp_avg", "exp_avg_sq"]
        for k in a["state"][i]:
            x, y = a["state"][i][k], b["state"][i][k]
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (i, k)


def test_state_dict_round_trip_with_torch():
    ps = _cpu_params(1)
    theirs = torch.optim.Adam(ps, lr=0.01, betas=(0.8, 0.95), eps=1e-7, weight_decay=1e-3)
    for s in range(3):
        for i, p in enumerate(ps[:3]):   # the last parameter never gets a gradient: no state, as in torch
            p.grad = torch.randn(p.shape, generator=torch.Generator().manual_seed(10 * s + i)).contiguous(
                memory_format=torch.channels_last if p.dim() == 4 else torch.contiguous_format)
        theirs.step()
    want = copy.deepcopy(theirs.state_dict())   # (load_state_dict keeps the tensors it is given where dtype and device fit)
    assert list(want["state"]) == [0, 1, 2]
    ours = Adam(ps, lr=0.5, max_grad_norm=100.0, skip_nonfinite=True)
    ours.load_state_dict(copy.deepcopy(want))
    got = ours.state_dict()
    _assert_same_state_dict(got, want)
    g = got["param_groups"][0]
    assert all(g[k] == v for k, v in want["param_groups"][0].items())   # lr, betas, eps, ... are the checkpoint's
    assert g["max_grad_norm"] == 100.0 and g["skip_nonfinite"] is True   # what the checkpoint does not have stays
    assert float(got["state"][0]["step"]) == 3.0
    # the other way round: what we write loads into torch.optim.Adam, which then continues as the original does
    back = torch.optim.Adam(ps, lr=0.5)
    back.load_state_dict(copy.deepcopy(got))
    _assert_same_state_dict(back.state_dict(), want)
    assert all(back.param_groups[0][k] == v for k, v in want["param_groups"][0].items() if k != "params")
    assert "max_grad_norm" in back.state_dict()["param_groups"][0]   # extra keys torch carries along and ignores
    clones = [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in ps]
    cont = torch.optim.Adam(clones, lr=0.5)
    cont.load_state_dict(copy.deepcopy(want))
    for a, b in zip(ps, clones):
        b.grad = None if a.grad is None else a.grad.clone(memory_format=torch.preserve_format)
    back.step()
    cont.step()
    for a, b in zip(ps, clones):
        assert torch.equal(a, b)
    # state_dict() holds the live moments, as torch's does, and a copy of the step
    assert got["state"][0]["exp_avg"] is ours.state[ps[0]]["exp_avg"] and got["state"][0]["step"] is not ours.state[ps[0]]["step"]


def test_load_model_resumes_the_optimizer(tmp_path, capsys):
    from centerpose_amd.lib.models.model import load_model, save_model

    torch.manual_seed(3)
    model = torch.nn.Linear(4, 3)
    opt = torch.optim.Adam(model.parameters(), 1.25e-4)
    for _ in range(2):
        opt.zero_grad()
        model(torch.randn(5, 4)).sum().backward()
        opt.step()
    saved = {k: v.clone() for k, v in model.state_dict().items()}
    for make in (lambda ps: torch.optim.Adam(ps, 7.0), lambda ps: Adam(ps, 7.0, max_grad_norm=100.0)):
        for epoch, k in ((1, 0), (2, 1), (5, 2)):
            path = str(tmp_path / ("model_%d.pth" % epoch))
            save_model(path, epoch, model, opt)
            fresh = torch.nn.Linear(4, 3)
            fresh_opt = make(fresh.parameters())
            out = load_model(fresh, path, fresh_opt, resume=True, lr=1.25e-4, lr_step=[2, 4])
            assert isinstance(out, tuple) and out[0] is fresh and out[1] is fresh_opt and out[2] == epoch
            assert all(torch.equal(fresh.state_dict()[n], saved[n]) for n in saved)
            assert [g["lr"] for g in fresh_opt.param_groups] == pytest.approx([1.25e-4 * 0.1 ** k], rel=1e-12)
            assert "Resumed optimizer with start lr" in capsys.readouterr().out
            _assert_same_state_dict(fresh_opt.state_dict(), opt.state_dict())
        # resume=False leaves the optimizer alone
        fresh = torch.nn.Linear(4, 3)
        fresh_opt = make(fresh.parameters())
        m, o, start = load_model(fresh, path, fresh_opt, resume=False, lr=1.25e-4, lr_step=[2, 4])
        assert m is fresh and o is fresh_opt and start == 0 and fresh_opt.param_groups[0]["lr"] == 7.0 and len(fresh_opt.state) == 0
        assert "Resumed" not in capsys.readouterr().out
    # a checkpoint without an optimizer: said, nothing loaded
    path = str(tmp_path / "bare.pth")
    save_model(path, 3, model)
    fresh = torch.nn.Linear(4, 3)
    fresh_opt = torch.optim.Adam(fresh.parameters(), 7.0)
    assert load_model(fresh, path, fresh_opt, resume=True, lr=1.25e-4, lr_step=[2, 4])[2] == 0
    assert "No optimizer parameters in checkpoint." in capsys.readouterr().out and fresh_opt.param_groups[0]["lr"] == 7.0
    # optimizer=None returns the model alone, as before
    assert load_model(torch.nn.Linear(4, 3), path).__class__ is torch.nn.Linear


def test_float32_error_is_far_below_the_gpu_limit():
    """torch's own float32 path on the CPU against the float64 reference, every variant: what R.TOL is ten times of."""
    assert R.TOL == 10 * R.MEASURED_F32
    seen = 0.0
    for variant in R.VARIANTS:
        ref = R.reference(variant)
        params, opt, norms = R.torch_float32(variant)
        m, v, step = R.state_of(opt, params)
        errs, norm_err = R.errors(ref, {k: p.detach() for k, p in params.items()}, m, v, norms)
        print("optim float32 CPU %-14s worst %.3e (norm %.3e)" % (variant, R.worst(errs, norm_err), norm_err))
        assert step == {k: float(s) for k, s in ref.step.items() if s} and "no_grad" not in step and step["empty"] == R.STEPS
        seen = max(seen, R.worst(errs, norm_err))
    assert 0 < seen <= 0.1 * R.TOL, seen
    # the case is what the issue asks for
    c = R.case()
    assert [c.params["len%d" % n].numel() for n in R.LENGTHS] == list(R.LENGTHS) and R.STEPS == 5
    assert c.params["channels_last"].is_contiguous(memory_format=torch.channels_last) and not c.params["channels_last"].is_contiguous()
    hp = c.variants()
    assert hp["clip_active"]["max_grad_norm"] < c.min_norm and hp["clip_inactive"]["max_grad_norm"] >= 100 * c.max_norm
    assert hp["clip_off"]["max_grad_norm"] is None and hp["weight_decay"]["weight_decay"] == 1e-2 and hp["betas"]["betas"] == (0.5, 0.9)
    assert hp["reference_lr"]["lr"] == 1.25e-4 and hp["clip_active"]["lr"] == 0.05
