"""GPU tests of the training operators beyond the caps of their launch plans (pytest -m gpu; cases and plans:
tests/plan_cases.py, pinned to the library by tests/test_plan_caps_cpu.py).

The operators' own suites stay below the caps: a stem workgroup owns one tile, a max-pool thread makes one pass, a conv stage
lane sums one pixel, a BatchNorm or depth-wise slab has eight steps.  The cases here are the smallest that make the workgroup
loop -- what the workload (dla_34, B = 32, 512 x 512) does in its first layers.  Every test asserts its regime before it
launches, and reuses the operator's own reference and tolerance: exact on dyadic inputs (stems, convolution), bitwise CPU
torch (max-pool), 1e-4 x max |reference| against float64 autograd (BatchNorm, depth-wise deconv).  One launch sequence per
case."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import batchnorm_ref as BR
from tests import conv_backward_ref as CR
from tests import deconv_backward_ref as DR
from tests import plan_cases as P

pytestmark = pytest.mark.gpu
GATED = pytest.mark.parametrize("gated", [True, False], ids=["gated", "plain"])


def _release():
    torch.cuda.empty_cache()


# ---- stems ----
@functools.lru_cache(maxsize=None)
def _stem_inputs(t):
    return CR.dyadic_inputs(500 + list(P.STEM_CAP_CASES).index(t), P.stem_case(t))   # shared, never modified


def _stem_device(device, c, inp, gated):
    from centerpose_amd import hip

    gw, gb = hip.conv2d_stem_backward(inp.x.to(device), CR.nhwc(inp.go).to(device), stride=c.stride,
                                      y=CR.nhwc(inp.y).to(device) if gated else None, need_bias_grad=True)
    return gw.cpu(), gb.cpu()


@GATED
@pytest.mark.parametrize("t", list(P.STEM_CAP_CASES), ids=P.stem_id)
def test_stem_runs_of_tiles(device, t, gated):
    """A workgroup walks two or three tiles: the patch is re-staged per tile and the accumulators are carried across tiles,
    tile rows and images."""
    c = P.stem_case(t)
    p = P.stem_plan(c.B, c.H, c.W, c.stride)
    assert p == P.STEM_CAP_CASES[t] and p.tiles_per_wg >= 2
    inp = _stem_inputs(t)
    _, gw_ref, gb_ref = CR.reference(inp.x, inp.w, inp.go, c.stride, c.pad, y=inp.y if gated else None)
    gw, gb = _stem_device(device, c, inp, gated)
    for name, a, e in (("grad_w", gw, gw_ref), ("grad_bias", gb, gb_ref)):
        print("%s gated=%d %s: %d of %d differ" % (P.stem_id(t), gated, name, int((a.double() != e).sum()), e.numel()))
    assert torch.equal(gw.double(), gw_ref)
    assert torch.equal(gb.double(), gb_ref)
    gw2, gb2 = _stem_device(device, c, inp, gated)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)   # call to call
    _release()


def test_stem_workspace_canary_beyond_the_cap(device):
    """347 slabs of three tiles stay inside the queried workspace, and a NULL grad_bias is not touched."""
    from centerpose_amd import hip

    t = list(P.STEM_CAP_CASES)[0]
    c = P.stem_case(t)
    assert P.stem_plan(c.B, c.H, c.W, c.stride).tiles_per_wg >= 2
    inp = _stem_inputs(t)
    _, gw_ref, _ = CR.reference(inp.x, inp.w, inp.go, c.stride, c.pad, y=inp.y)
    L = hip.lib()
    geo = (c.B, c.H, c.W, c.Cin, c.Cout, c.stride)
    nbytes = L.cp_conv2d_stem_backward_workspace_bytes(*geo)
    assert nbytes == P.stem_workspace_bytes(*geo)
    words = 1024
    ws = torch.full((nbytes // 4 + words,), 0x5A5A5A5A, dtype=torch.int32, device=device)
    x, go, y = inp.x.to(device), CR.nhwc(inp.go).to(device), CR.nhwc(inp.y).to(device)
    gw = torch.full((c.Cout, c.Cin, 7, 7), 7.25, device=device)
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    rc = L.cp_conv2d_stem_backward(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(x), p(go), p(y), p(gw), None, p(ws),
                                   nbytes, *geo)
    assert rc == 0, L.cp_last_error()
    torch.cuda.synchronize()
    assert bool((ws[nbytes // 4:] == 0x5A5A5A5A).all())
    assert torch.equal(gw.cpu().double(), gw_ref)
    del ws, x, go, y, gw
    _release()


# ---- max-pool ----
@functools.lru_cache(maxsize=None)
def _pool_reference(geo):
    """(x, grad_out, y, grad_x) by CPU torch float32, logical NCHW; shared by both layouts, never modified."""
    g = torch.Generator().manual_seed(100 * geo[0] + geo[2])
    x = torch.relu(torch.randn(P.POOL_B, P.POOL_C, P.POOL_H, P.POOL_W, generator=g))
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, *geo)
    go = torch.randn(y.shape, generator=g)
    gx, = torch.autograd.grad(y, xr, go)
    return x, go, y.detach(), gx


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("geo", list(P.POOL_CAP_CASES), ids=lambda g: "x".join(str(i) for i in g))
def test_pool_second_grid_pass(device, geo, layout):
    """More float4 items than the grid has threads: the grid-stride loops take a second pass (the backward a fifth), with the
    floor / pad edges of an odd H and W inside the later passes."""
    from centerpose_amd import pool

    fwd_items, bwd_items = P.pool_items(P.POOL_B, P.POOL_C, P.POOL_H, P.POOL_W, geo)
    assert (fwd_items, bwd_items) == P.POOL_CAP_CASES[geo] and min(fwd_items, bwd_items) > P.POOL_GRID_ITEMS
    x, go, y_ref, gx_ref = _pool_reference(geo)
    assert bool((x == 0).any())   # ties exist
    xd = x.to(device)
    if layout == "channels_last":
        xd = xd.contiguous(memory_format=torch.channels_last)
    god = go.to(device)
    outs = []
    for _ in range(2):   # the second call: call-to-call identity
        xg = xd.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y = pool.max_pool2d(xg, *geo)
        assert y.is_contiguous(memory_format=torch.channels_last)
        gx, = torch.autograd.grad(y, xg, god)
        outs.append((y.detach().cpu(), gx.cpu()))
        del xg, y, gx
    assert tuple(outs[0][0].shape) == tuple(y_ref.shape)
    print("pool %s %s: forward %d of %d differ, grad_x %d of %d differ" % (geo, layout, int((outs[0][0] != y_ref).sum()), y_ref.numel(),
                                                                         int((outs[0][1] != gx_ref).sum()), gx_ref.numel()))
    assert torch.equal(outs[0][0], y_ref)
    assert torch.equal(outs[0][1], gx_ref)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    del xd, god
    _release()


# ---- conv backward ----
@functools.lru_cache(maxsize=None)
def _conv_inputs(c):
    return CR.dyadic_inputs(sum(c), c)   # shared, never modified


@GATED
@pytest.mark.parametrize("c", list(P.CONV_CAP_CASES), ids=CR.case_id)
def test_conv_stage_lane_sums_several_pixels(device, c, gated):
    """More than 512 x 64 output pixels: a stage slab has more than 64 pixels, so a pixel lane of stage_kernel sums more than
    one step into the bias partials."""
    s = P.conv_stage_plan(c)
    assert s == P.CONV_CAP_CASES[c] and s.st_px > 64
    inp = _conv_inputs(c)
    got = CR.device_backward(device, c, inp, gated)
    exp = CR.reference(inp.x, inp.w, inp.go, c.stride, c.pad, inp.y if gated else None)
    for name, a, e in zip(("grad_x", "grad_w", "grad_bias"), got, exp):
        bad = int((a.double() != e).sum())
        print("%s gated=%d %s: %d of %d differ" % (CR.case_id(c), gated, name, bad, e.numel()))
        assert a.shape == e.shape and torch.equal(a.double(), e), (name, gated, bad)
    _release()


# ---- BatchNorm ----
@functools.lru_cache(maxsize=1)
def _bn_inputs(c, mean):
    return BR.inputs(sum(c), c, mean=mean)   # shared by the two modes of a case, never modified; one case held at a time


def _bn_check(device, c, residual, act, mean=0.0):
    p = P.bn_plan(*c)
    assert p == P.BN_CAP_CASES[c] and p.red_px // p.S > 8 and p.red_slabs < p.red_bound
    inp = _bn_inputs(c, mean)
    what = "%s%s res=%d act=%d" % ("mean %g " % mean if mean else "", BR.case_id(c), residual, act)
    fwd = BR.device_forward(device, inp, residual, act)
    bwd = BR.device_backward(device, inp, fwd, residual, act)
    BR.check(fwd[0], BR.reference_forward(inp, residual, act), what)
    BR.check(bwd, BR.reference_backward(inp, residual, fwd[0]["y"] if act else None), what)
    del fwd, bwd
    _release()


@pytest.mark.parametrize("residual,act", [(True, 1), (False, 0)], ids=["res_relu", "plain"])
@pytest.mark.parametrize("c", list(P.BN_CAP_CASES), ids=BR.case_id)
def test_batchnorm_nine_steps_per_slab(device, c, residual, act):
    """More row steps than eight per slab at the slab cap: the reductions' lanes walk nine steps, and fewer slabs are launched
    than the workspace bound."""
    _bn_check(device, c, residual, act)


def test_batchnorm_large_mean_many_slabs(device):
    """x = 1000 + N(0, 1) over 918 slabs of two channel passes: the many-way Chan merge of finalize_kernel."""
    _bn_check(device, P.BN_LARGE_MEAN_CASE, True, 1, mean=1000.0)
    _bn_inputs.cache_clear()


# ---- depth-wise deconv backward ----
@pytest.mark.parametrize("c", list(P.DW_CAP_CASES), ids=DR.case_id)
def test_depthwise_deconv_nine_rounds_per_slab(device, c):
    """More pixel-lane rounds than 8 x 1024: a slab has nine rounds, so the per-lane tap accumulators run past the eight the
    older cases give them.  grad_out is about 135 MB: the cap times the smallest round."""
    from centerpose_amd import hip

    p = P.dw_plan(c.B, c.H, c.W, c.Cin, c.stride)
    assert p == P.DW_CAP_CASES[c] and p.rounds_per_slab > 8
    inp = DR.inputs(1, c)
    ref = DR.reference.__wrapped__(1, c)   # not through the cache: nothing else uses this case, and it is a gigabyte
    ref = dict(grad_x=ref["grad_x"], grad_w=ref["grad_w"])
    x, go = DR.nhwc(inp.x).to(device), DR.nhwc(inp.go).to(device)
    gx, gw = hip.conv_transpose2d_backward(x, inp.w.to(device), go, c.stride, c.pad, c.groups)
    DR.check(dict(grad_x=DR.nchw(gx), grad_w=gw), ref, DR.case_id(c))
    del x, go, gx, gw, inp, ref
    _release()
