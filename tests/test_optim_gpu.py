"""GPU tests of ``centerpose_amd.optim.Adam`` (pytest -m gpu): the clip + Adam step of csrc/optim.hip against the float64
reference and the case list of tests/optim_ref.py, within its TOL (ten times the float32 error of torch's own CPU path), then
on the whole dla_34 network at the geometry of tests/test_pose_net_det_gpu.py.

Measured on an MI355X: see DESIGN.md section 3.13.
"""
import copy
from collections import OrderedDict

import pytest
import torch

from centerpose_amd import hip
from centerpose_amd.optim import Adam
from tests import optim_ref as R

pytestmark = pytest.mark.gpu


def _run(variant, device, steps=R.STEPS, order=None, grads=None, check_grads=False, **kw):
    """``steps`` steps of the case with our optimizer: (params by name, optimizer, the norm after every step)."""
    c = R.case()
    grads = grads or c.grads
    params = R.materialize(c, device, order)
    opt = Adam(list(params.values()), **dict(c.variants()[variant], **kw))
    norms = []
    for s in range(steps):
        R.set_grads(params, grads[s], device)
        assert opt.step() is None
        norms.append(opt.last_grad_norm.clone())
        if check_grads:   # .grad is read, never written
            for k, p in params.items():
                assert (p.grad is None) == (grads[s][k] is None) and (p.grad is None or torch.equal(p.grad.cpu(), grads[s][k])), k
    return params, opt, norms


def _errors(variant, params, opt, norms, steps=R.STEPS):
    ref = R.reference(variant, steps)
    m, v, step = R.state_of(opt, params)
    errs, norm_err = R.errors(ref, {k: p.detach() for k, p in params.items()}, m, v, [float(n) for n in norms])
    assert step == {k: float(s) for k, s in ref.step.items() if s}
    return errs, norm_err


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_parity_with_float64(device, variant):
    c = R.case()
    params, opt, norms = _run(variant, device, check_grads=True)
    measured = variant != "clip_off"   # without clipping (and without skip_nonfinite) the norm is not measured: NaN
    if not measured:
        assert all(bool(torch.isnan(n)) for n in norms)
    errs, norm_err = _errors(variant, params, opt, norms if measured else [])
    print("optim %-14s worst %.3e (norm %.3e) of TOL %.1e" % (variant, R.worst(errs, norm_err), norm_err, R.TOL))
    assert norm_err <= R.TOL
    bad = [(k, n, e) for k, es in errs.items() for n, e in es.items() if not e <= R.TOL]
    assert not bad, bad[:10]
    # the parameter that never had a gradient: untouched, no state
    assert torch.equal(params["no_grad"].detach().cpu(), c.params["no_grad"]) and len(opt.state.get(params["no_grad"], {})) == 0
    assert float(opt.state[params["empty"]]["step"]) == R.STEPS and opt.layout_copies == 0
    assert opt.last_grad_norm.dim() == 0 and opt.last_step_skipped.dtype == torch.bool and not bool(opt.last_step_skipped)
    assert opt.state_dict()["state"][0]["step"].device.type == "cuda" and float(opt.state_dict()["state"][0]["step"]) == R.STEPS


def test_layouts(device):
    """The channels_last and the unaligned parameter run in their own memory (moments in the parameter's layout, no copy); a
    gradient with other strides than its parameter is copied into the parameter's layout, counted, and gives the same result."""
    c = R.case()
    params, opt, norms = _run("clip_active", device)
    errs, _ = _errors("clip_active", params, opt, norms)
    for k in ("channels_last", "unaligned", "weight4d"):
        assert all(e <= R.TOL for e in errs[k].values()), (k, errs[k])
        assert opt.state[params[k]]["exp_avg"].stride() == params[k].stride()
    assert params["unaligned"].data_ptr() % 16 == 4 and params["channels_last"].stride() == c.params["channels_last"].stride()
    assert opt.layout_copies == 0
    # the same steps with the 4-D gradients in the other memory format
    swapped = []
    for gs in c.grads:
        gs = OrderedDict(gs)
        gs["weight4d"] = gs["weight4d"].contiguous(memory_format=torch.channels_last)
        gs["channels_last"] = gs["channels_last"].contiguous()
        assert gs["weight4d"].stride() != c.params["weight4d"].stride() and gs["channels_last"].stride() != c.params["channels_last"].stride()
        swapped.append(gs)
    params2, opt2, norms2 = _run("clip_active", device, grads=swapped)
    assert opt2.layout_copies == 2 * R.STEPS
    assert params2["weight4d"].grad.stride() == swapped[0]["weight4d"].stride()   # .grad itself is not replaced
    for k in params:
        assert torch.equal(params[k], params2[k]), k
    assert all(torch.equal(a, b) for a, b in zip(norms, norms2))


def _assert_identical(a, b, norms=True):
    (pa, oa, na), (pb, ob, nb) = a, b
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
        sa, sb = oa.state.get(pa[k], {}), ob.state.get(pb[k], {})
        assert list(sa) == list(sb)
        for name in sa:
            assert torch.equal(sa[name], sb[name]), (k, name)
    if norms:
        assert all(torch.equal(x, y) for x, y in zip(na, nb))


@pytest.mark.parametrize("variant", ["clip_active", "weight_decay"])
def test_reproducible(device, variant):
    first = _run(variant, device)
    _assert_identical(first, _run(variant, device))
    # registered in reverse order: every tensor's chunks sum as before and the float64 sum of the partials rounds to the
    # same float32 norm here, so p, m and v are bitwise the same; the norm's summation order follows the table
    rev = _run(variant, device, order=list(reversed(R.case().names)))
    _assert_identical(first, (OrderedDict((k, rev[0][k]) for k in first[0]), rev[1], rev[2]), norms=False)


def _torch_steps(variant, device, grads):
    """clip_grad_norm_ + torch.optim.Adam on the device over ``grads``: params by name."""
    c = R.case()
    hp = dict(c.variants()[variant])
    max_norm = hp.pop("max_grad_norm")
    params = R.materialize(c, device)
    opt = torch.optim.Adam(list(params.values()), **hp)
    for gs in grads:
        R.set_grads(params, gs, device)
        torch.nn.utils.clip_grad_norm_([p for p in params.values() if p.grad is not None], max_norm)
        opt.step()
    return params, opt


def _poisoned(step, value):
    gs = OrderedDict(R.case().grads[step])
    g = gs["len1025"].clone()
    g[17] = value
    gs["len1025"] = g
    return gs


@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_gradient_by_default_is_torchs(device, value):
    """One inf (the norm is inf, the coefficient 0, inf x 0 = NaN at that element) or one NaN (everything is NaN): the
    parameters after the step are torch's own, NaN for NaN, the finite ones within TOL."""
    c = R.case()
    grads = [c.grads[0], _poisoned(1, value)]
    params, opt, norms = _run("clip_active", device, steps=2, grads=grads)
    want, _ = _torch_steps("clip_active", device, grads)
    assert not bool(torch.isfinite(norms[1])) and not bool(opt.last_step_skipped)
    n_bad = 0
    for k in params:
        a, b = params[k].detach(), want[k].detach()
        assert torch.equal(torch.isfinite(a), torch.isfinite(b)) and torch.equal(torch.isnan(a), torch.isnan(b)), k
        ok = torch.isfinite(b)
        n_bad += int((~ok).sum())
        if bool(ok.any()):
            assert float((a[ok] - b[ok]).abs().max()) <= R.TOL * float(b[ok].abs().max()), k
    assert n_bad == (1 if value == float("inf") else sum(p.numel() for k, p in params.items() if k != "no_grad"))


@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_skip_nonfinite(device, value):
    c = R.case()
    before = _run("clip_active", device, steps=1, skip_nonfinite=True)
    params, opt, norms = _run("clip_active", device, steps=2, grads=[c.grads[0], _poisoned(1, value)], skip_nonfinite=True)
    assert bool(opt.last_step_skipped) and not bool(torch.isfinite(norms[1]))
    _assert_identical((params, opt, norms[:1]), before)   # p, m, v and the step counts as after the first step, bit for bit
    # the next finite step equals that of a run that never saw the bad one
    R.set_grads(params, c.grads[1], device)
    opt.step()
    assert not bool(opt.last_step_skipped)
    clean = _run("clip_active", device, steps=2, skip_nonfinite=True)
    _assert_identical((params, opt, [opt.last_grad_norm]), (clean[0], clean[1], clean[2][1:]))
    # the flag alone, without clipping, still measures the norm
    _, opt3, norms3 = _run("clip_off", device, steps=1, skip_nonfinite=True)
    assert abs(float(norms3[0]) - R.reference("clip_off", 1).norms[0]) <= R.TOL * float(norms3[0]) and not bool(opt3.last_step_skipped)


def test_one_call_and_no_synchronisation(device, monkeypatch):
    c = R.case()
    calls = []
    real = hip.optim.adam_step

    def counted(*a, **kw):
        calls.append(a[1:3])
        return real(*a, **kw)

    monkeypatch.setattr(hip.optim, "adam_step", counted)
    params = R.materialize(c, device)
    opt = Adam(list(params.values()), **c.variants()["clip_active"])
    R.set_grads(params, c.grads[0], device)
    opt.step()
    assert len(calls) == 1 and calls[0][0] == len(c.names)   # one call for the whole case list
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    # fresh gradients (new addresses: the table is rebuilt and uploaded) and a fresh optimizer (state allocation), both under
    # the switch that turns every synchronising torch call into an error
    R.set_grads(params, c.grads[1], device)
    params2 = R.materialize(c, device)
    opt2 = Adam(list(params2.values()), **c.variants()["clip_active"])
    R.set_grads(params2, c.grads[0], device)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
        opt2.step()
        opt.zero_grad(set_to_none=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert len(calls) == 3
    errs, norm_err = _errors("clip_active", params, opt, [], steps=2)
    assert all(e <= R.TOL for es in errs.values() for e in es.values())


def test_wrapper_refuses_short_table_and_state(device):
    """hip.optim.adam_step knows the sizes of the two device blocks the library only gets addresses of."""
    n, chunks = 3, 5
    table = torch.zeros(n * hip.optim.ADAM_TENSOR_BYTES + chunks * hip.optim.ADAM_CHUNK_BYTES, dtype=torch.uint8, device=device)
    state = torch.zeros(hip.optim.adam_state_bytes(n), dtype=torch.uint8, device=device)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 100.0)
    with pytest.raises(ValueError, match="table is smaller"):
        hip.optim.adam_step(table[:-1], n, chunks, state, *hyper)
    with pytest.raises(ValueError, match="state is smaller"):
        hip.optim.adam_step(table, n, chunks, state[:-1], *hyper)
    with pytest.raises(ValueError, match="n_tensors must be >= 1"):   # the library's own refusals still come through
        hip.optim.adam_step(table, 0, chunks, state, *hyper)
    with pytest.raises(ValueError, match="workspace too small"):
        hip.optim.adam_step(table, n, chunks, state, *hyper, workspace=torch.zeros(8, dtype=torch.uint8, device=device))
    assert not bool(state.any())   # nothing ran


def test_interchange_with_torch(device):
    """Two steps here, the state_dict into a device torch.optim.Adam, the third step there: three steps of the reference."""
    c = R.case()
    params, opt, _ = _run("clip_active", device, steps=2)
    hp = dict(c.variants()["clip_active"])
    max_norm = hp.pop("max_grad_norm")
    theirs = torch.optim.Adam(list(params.values()), lr=123.0)
    theirs.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert theirs.param_groups[0]["lr"] == hp["lr"] and theirs.param_groups[0]["betas"] == hp["betas"]
    R.set_grads(params, c.grads[2], device)
    torch.nn.utils.clip_grad_norm_([p for p in params.values() if p.grad is not None], max_norm)
    theirs.step()
    errs, _ = _errors("clip_active", params, theirs, [], steps=3)
    assert all(e <= R.TOL for es in errs.values() for e in es.values()), errs
    # and back: their state after three steps into ours, steps four and five here
    ours = Adam(list(params.values()), lr=123.0)
    ours.load_state_dict(copy.deepcopy(theirs.state_dict()))
    ours.param_groups[0]["max_grad_norm"] = max_norm
    for s in (3, 4):
        R.set_grads(params, c.grads[s], device)
        ours.step()
    errs, _ = _errors("clip_active", params, ours, [], steps=5)
    assert all(e <= R.TOL for es in errs.values() for e in es.values()), errs


def test_sparse_gradient_is_refused_as_in_torch(device):
    p = torch.nn.Parameter(torch.zeros(4, 3, device=device))
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3)).to(device)
    with pytest.raises(RuntimeError, match="does not support sparse gradients"):
        Adam([p]).step()


# ---- the whole network: PoseNet (dla_34), B = 2, 3 x 64 x 96, linear loss, as tests/test_pose_net_det_gpu.py ----

def _pose_net(device):
    from centerpose_amd import synth
    from centerpose_amd.pose_net import PoseNet
    from tests import pose_net_ref as PR
    from tests import test_pose_net_gpu as TP

    hip.set_default_precision("f32")
    net = PoseNet(synth.HEADS_POSE, head_conv=PR.HEAD_CONV, opt=TP._Opt(pre_img=False, pre_hm=False, pre_hm_hp=False))
    net.load_state_dict(PR.case_state_dict(False), strict=True)
    x, _, _, lin = PR.case_inputs(False)
    return net.to(device).train(), x.to(device), OrderedDict((h, v.to(device)) for h, v in lin.items())


def _backward(net, x, lin):
    z = net(x)[0]
    sum((z[h] * lin[h]).sum() for h in z).backward()


@pytest.fixture
def deterministic():
    prev = hip.set_deterministic(True)
    yield
    hip.set_deterministic(prev)


def test_pose_net_training_steps_are_bit_identical(device, deterministic):
    """Three full steps (zero_grad, forward, backward, clip + Adam at the reference's lr and max norm) twice from the same
    state: parameters, buffers and optimizer state bit for bit."""
    runs = []
    for _ in range(2):
        net, x, lin = _pose_net(device)
        opt = Adam(net.parameters(), 1.25e-4, max_grad_norm=100.)
        norms = []
        for _ in range(3):
            opt.zero_grad()
            _backward(net, x, lin)
            opt.step()
            norms.append(opt.last_grad_norm.clone())
        runs.append((net, opt, norms))
    (na, oa, norms_a), (nb, ob, norms_b) = runs
    print("pose_net optimizer: layout_copies %d in 3 steps, grad norms %s" % (oa.layout_copies, [float(n) for n in norms_a]))
    assert all(torch.equal(a, b) for a, b in zip(norms_a, norms_b)) and all(bool(torch.isfinite(n)) for n in norms_a)
    sa, sb = na.state_dict(), nb.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    stepped = 0
    for (k, pa), pb in zip(na.named_parameters(), nb.parameters()):
        assert list(oa.state.get(pa, {})) == list(ob.state.get(pb, {})), k
        for name, t in oa.state.get(pa, {}).items():
            assert torch.equal(t, ob.state[pb][name]), (k, name)
            assert name != "step" or float(t) == 3.0
        stepped += bool(oa.state.get(pa))
    assert stepped > 200 and oa.layout_copies == ob.layout_copies


def test_pose_net_step_matches_torch(device, deterministic):
    """One step on the network's real gradients against clip_grad_norm_ + torch.optim.Adam on a float64 clone of the
    parameters and gradients, max |delta p| per tensor relative to lr (one Adam step moves a weight by at most about lr).
    lr = 0.5 for this one step, so that the measure resolves the update: max |p| of this case is 4.35, where float32 rounds
    the updated parameter itself by up to 2.4e-7, which is 4.8e-7 of this lr and would be 1.9e-3 of the reference's 1.25e-4."""
    lr = 0.5
    net, x, lin = _pose_net(device)
    _backward(net, x, lin)
    named = [(k, p) for k, p in net.named_parameters()]
    clones = [torch.nn.Parameter(p.detach().double()) for _, p in named]
    for (_, p), q in zip(named, clones):
        q.grad = None if p.grad is None else p.grad.double()
    opt = Adam(net.parameters(), lr, max_grad_norm=100.)
    opt.step()
    with_grad = [q for q in clones if q.grad is not None]
    norm = torch.nn.utils.clip_grad_norm_(with_grad, 100.)
    torch.optim.Adam(clones, lr).step()
    print("pose_net optimizer: one step, grad norm %.6g (float64 %.6g), layout_copies %d" % (float(opt.last_grad_norm), float(norm),
                                                                                            opt.layout_copies))
    assert abs(float(opt.last_grad_norm) - float(norm)) <= R.TOL * float(norm)
    worst, bad = 0.0, []
    for (k, p), q in zip(named, clones):
        e = float((p.detach().double() - q.detach()).abs().max()) / lr if p.numel() else 0.0
        worst = max(worst, e)
        if q.grad is None:
            assert e == 0.0 and not opt.state.get(p), k
        elif not e <= R.TOL:
            bad.append((k, e))
    print("pose_net optimizer: worst max |delta p| / lr %.3e of TOL %.1e" % (worst, R.TOL))
    assert not bad, bad[:10]
