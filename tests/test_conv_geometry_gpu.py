"""conv2d over its whole accepted geometry on the device (pytest -m gpu): conv.conv2d / Conv2d / use_hip_convs and
cp_conv2d_backward_nhwc at rectangular and even kernels, stride 3 and 4, pad above k // 2, more than 32 taps and unaligned
channel counts (tests/conv_geometry_cases.py), forward and backward, against torch.nn.functional.conv2d under float64 CPU
autograd.  Dyadic inputs must match EXACTLY, in float32 and under "f16x3" (the generator's premise: every partial sum is an
integer below 2^24; integers in [-2, 2] times a power of two have an exact binary16 hi half and a zero lo half).  Gaussian
inputs: forward within 2e-5 x max |reference| (tests/test_gpu_parity.py), gradients within 1e-4 x max |reference|
(tests/test_conv_backward_gpu.py)."""
import copy
import ctypes

import pytest
import torch
from torch import nn

from centerpose_amd import conv, hip
from centerpose_amd.hip import _abi
from tests import conv_geometry_cases as G

pytestmark = pytest.mark.gpu
NAMES = ("out", "grad_x", "grad_w", "grad_bias")
F16_CASES = [c for c in G.CASES if G.f16x3_eligible(c)]
FWD_TOL, GRAD_TOL = 2e-5, 1e-4


@pytest.fixture(autouse=True)
def f32_before_and_after():
    """Every test starts in "f32" and leaves the library there, whatever it switched to in between."""
    hip.set_default_precision("f32")
    yield
    hip.set_default_precision("f32")


def _x_on(device, x, channels_last):
    x = x.to(device)
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()


def _functional(device, c, inp, relu, has_bias, channels_last=False, backward=True):
    """conv.conv2d on the case -> (out, grad_x, grad_w, grad_bias | None) on the CPU (out alone without ``backward``)."""
    xd = _x_on(device, inp.x, channels_last).requires_grad_(True)
    wd = inp.w.to(device).requires_grad_(True)
    bd = inp.bias.to(device).requires_grad_(True) if has_bias else None
    out = conv.conv2d(xd, wd, bd, c.stride, c.pad, relu=relu)
    assert out.is_contiguous(memory_format=torch.channels_last)
    if not backward:
        return out.detach().cpu()
    grads = torch.autograd.grad(out, (xd, wd) + ((bd,) if has_bias else ()), inp.go.to(device))
    return (out.detach().cpu(),) + tuple(g.cpu() for g in grads) + (() if has_bias else (None,))


def _equal(got, exp, what):
    """Every device tensor EQUALS its float64 reference (a missing grad_bias is skipped)."""
    for name, a, e in zip(NAMES, got, exp):
        if a is None:
            continue
        assert a.shape == e.shape, (what, name, tuple(a.shape), tuple(e.shape))
        bad = int((a.double() != e).sum())
        assert bad == 0, "%s %s: %d of %d differ, max err %.3g" % (what, name, bad, e.numel(), float((a.double() - e).abs().max()))


def _close(got, exp, what):
    for name, a, e in zip(NAMES, got, exp):
        if a is None:
            continue
        assert a.shape == e.shape, (what, name)
        tol = FWD_TOL if name == "out" else GRAD_TOL
        scale = float(e.abs().max())
        err = float((a.double() - e.double()).abs().max())
        print("%s %s: max err %.3g, max |ref| %.3g (bound %.3g)" % (what, name, err, scale, tol * scale))
        assert scale > 0 and err <= tol * scale, "%s %s: max err %.3g vs max |ref| %.3g" % (what, name, err, scale)


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_dyadic_forward_and_gradients_are_exact(device, c):
    for relu in (False, True):
        for has_bias in (False, True):
            inp, exp = G.dyadic_reference(c, relu, has_bias)
            for channels_last in (False, True):
                what = "%s relu=%d bias=%d channels_last=%d" % (G.case_id(c), relu, has_bias, channels_last)
                got = _functional(device, c, inp, relu, has_bias, channels_last)
                _equal(got, exp, what)
                # the module, with and without a gradient for its input
                mod = conv.Conv2d(c.Cin, c.Cout, (c.KH, c.KW), c.stride, c.pad, bias=has_bias).to(device)
                mod.relu = relu
                with torch.no_grad():
                    mod.weight.copy_(inp.w)
                    if has_bias:
                        mod.bias.copy_(inp.bias)
                for x_grad in (True, False):
                    xm = _x_on(device, inp.x, channels_last).requires_grad_(x_grad)
                    mod.zero_grad()
                    om = mod(xm)
                    om.backward(inp.go.to(device))
                    assert (xm.grad is not None) == x_grad
                    _equal((om.detach().cpu(), xm.grad.cpu() if x_grad else None, mod.weight.grad.cpu(),
                            mod.bias.grad.cpu() if has_bias else None), exp, what + " module x_grad=%d" % x_grad)


@pytest.mark.parametrize("c", F16_CASES, ids=G.case_id)
def test_dyadic_forward_is_exact_f16x3(device, c):
    hip.set_default_precision("f16x3")
    for relu in (False, True):
        for has_bias in (False, True):
            inp, exp = G.dyadic_reference(c, relu, has_bias)
            for channels_last in (False, True):
                what = "f16x3 %s relu=%d bias=%d channels_last=%d" % (G.case_id(c), relu, has_bias, channels_last)
                # (the gradients are float32 kernels in either mode; they are fed by this mode's forward output when relu gates)
                _equal(_functional(device, c, inp, relu, has_bias, channels_last), exp, what)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_all_zero_output_channel_is_exactly_the_bias(device, precision):
    """One whole output channel of w is zero: its per-channel |max| is 0, the clamped-exponent branch of the f16x3 weight scale."""
    c = G.RECT_F16_CASES[4]
    inp, _ = G.dyadic_reference(c, False, True)
    ch = int(inp.bias.abs().argmax())   # a channel whose bias is not 0
    assert float(inp.bias[ch]) != 0
    w = inp.w.clone()
    w[ch] = 0
    inz = inp._replace(w=w)
    exp = G.reference(inz.x, inz.w, inz.bias, inz.go, c.stride, c.pad)
    hip.set_default_precision(precision)
    got = _functional(device, c, inz, False, True)
    assert torch.equal(got[0][:, ch], inp.bias[ch].expand_as(got[0][:, ch]))
    _equal(got, exp, "%s zeroed channel %d" % (precision, ch))


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_gaussian_inputs(device, c):
    inp = G.gaussian_inputs(sum(c) + 1, c)
    exp = G.reference(inp.x, inp.w, inp.bias, inp.go, c.stride, c.pad)
    got = _functional(device, c, inp, False, True, channels_last=True)
    _close(got, exp, G.case_id(c))
    if G.f16x3_eligible(c):
        hip.set_default_precision("f16x3")
        out16 = _functional(device, c, inp, False, True, channels_last=True, backward=False)
        hip.set_default_precision("f32")
        _close((out16,), exp, "f16x3 " + G.case_id(c))
        assert not torch.equal(out16, got[0]), "the split-f16 kernel did not run: its output is bit-equal to the float32 one"


def _hand_padded(xh, w, bias, stride, pad, relu):
    """``hip.conv2d_nhwc`` the way the layers called it while the library refused a ``shift`` shorter than its N tile: weight and
    bias padded with zero channels to the tile of the width, the output sliced.  xh NHWC -> NHWC."""
    cout = w.shape[0]
    tile = 16 if cout <= 16 else 32 if cout <= 32 else 128 if cout % 128 == 0 else 64
    cpad = (cout + tile - 1) // tile * tile
    wp = torch.cat([w, w.new_zeros((cpad - cout,) + tuple(w.shape[1:]))])
    bp = torch.cat([bias, bias.new_zeros(cpad - cout)])
    return hip.conv2d_nhwc(xh, wp, shift=bp, stride=stride, pad=pad, act=1 if relu else 0)[..., :cout]


def _biased_inputs(device, seed, B, Cin, Cout, H, W, K):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) / (Cin * K * K) ** 0.5
    return x.to(device), w.to(device), torch.randn(Cout, generator=g).to(device)


BIASED_GEOMETRIES = [((2, 16, 32), 3, 1, 1),    # whole 8 x 16 patches
                     ((1, 9, 13), 3, 1, 1),     # ragged
                     ((2, 16, 32), 1, 2, 0)]


def test_bias_of_any_width_equals_the_hand_padded_call(device):
    """cp_conv2d_nhwc stages ``shift`` into its workspace itself: conv.conv2d and stem.stem_conv2d with a bias of a width that is
    no multiple of the N tile are bit-equal to the call on hand-padded weight and bias, whose N tile is the same."""
    from centerpose_amd import stem

    for precision in ("f32", "f16x3"):
        hip.set_default_precision(precision)
        for (B, H, W), K, stride, pad in BIASED_GEOMETRIES:
            for Cin in (4, 32):
                for Cout in (1, 8, 27, 48, 160):
                    x, w, bias = _biased_inputs(device, Cout + Cin + K, B, Cin, Cout, H, W, K)
                    xh = x.permute(0, 2, 3, 1).contiguous()
                    for relu in (False, True):
                        got = conv.conv2d(x, w, bias, stride, pad, relu=relu)
                        old = _hand_padded(xh, w, bias, stride, pad, relu).permute(0, 3, 1, 2)
                        assert got.shape == old.shape and got.shape[1] == Cout
                        assert torch.equal(got, old), (precision, (B, H, W), K, stride, Cin, Cout, relu)
        for Cout in (16, 48):
            x, w, bias = _biased_inputs(device, Cout, 2, 3, Cout, 32, 48, 7)
            x4 = torch.cat([x, x.new_zeros(2, 1, 32, 48)], 1).permute(0, 2, 3, 1).contiguous()
            w4 = torch.cat([w, w.new_zeros(Cout, 1, 7, 7)], 1)
            for stride in (1, 2):
                for relu in (False, True):
                    got = stem.stem_conv2d(x, w, bias, stride, relu=relu)
                    old = _hand_padded(x4, w4, bias, stride, 3, relu).permute(0, 3, 1, 2)
                    assert got.shape == old.shape and torch.equal(got, old), (precision, "stem", Cout, stride, relu)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_bias_of_width_100_runs_on_the_64_wide_tile(device, precision):
    """The one family of widths whose N tile differs between the routes: 65 .. 127 that are no multiple of 64 ran on the 128-wide
    tile when padded by hand and run on the 64-wide tile now.  Both are within the forward bound of the float64 reference."""
    x, w, bias = _biased_inputs(device, 100, 2, 32, 100, 16, 32, 3)
    exp = torch.nn.functional.conv2d(x.cpu().double(), w.cpu().double(), bias.cpu().double(), 1, 1)
    hip.set_default_precision(precision)
    new = conv.conv2d(x, w, bias, 1, 1).cpu()
    old = _hand_padded(x.permute(0, 2, 3, 1).contiguous(), w, bias, 1, 1, False).permute(0, 3, 1, 2).cpu()
    _close((new,), (exp,), "%s Cout=100, true width (64-wide tile)" % precision)
    _close((old,), (exp,), "%s Cout=100, hand-padded to 128" % precision)


def _swapped(c, inp):
    """The case and its inputs with the spatial axes exchanged (KH <-> KW, H <-> W)."""
    t = lambda a: a.transpose(2, 3).contiguous()
    return c._replace(H=c.W, W=c.H, KH=c.KW, KW=c.KH), inp._replace(x=t(inp.x), w=t(inp.w), go=t(inp.go), y=t(inp.y))


@pytest.mark.parametrize("c", [G.RECT_F16_CASES[4], G.RECT_F16_CASES[5], G.RECT_F32_CASES[0], G.UNALIGNED_CASES[2]], ids=G.case_id)
def test_transposed_problem_gives_the_transposed_result(device, c):
    assert c.KH != c.KW
    inp, _ = G.dyadic_reference(c, True, True)
    ct, inpt = _swapped(c, inp)
    assert (ct.KH, ct.KW) == (c.KW, c.KH) and G.out_size(ct) == G.out_size(c)[::-1]
    for precision in ("f32", "f16x3") if G.f16x3_eligible(c) else ("f32",):
        hip.set_default_precision(precision)
        a = _functional(device, c, inp, True, True)
        b = _functional(device, ct, inpt, True, True)
        hip.set_default_precision("f32")
        for name, p, q in zip(NAMES[:3], a, b):
            assert torch.equal(p.transpose(2, 3), q), (precision, name)
        assert torch.equal(a[3], b[3]), precision


def _device_backward(device, c, inp, gated=True, need_x_grad=True, need_bias_grad=True):
    gx, gw, gb = hip.conv2d_backward(G.nhwc(inp.x).to(device), inp.w.to(device), G.nhwc(inp.go).to(device), stride=c.stride,
                                     pad=c.pad, y=G.nhwc(inp.y).to(device) if gated else None, need_x_grad=need_x_grad,
                                     need_bias_grad=need_bias_grad)
    return (gx.permute(0, 3, 1, 2).cpu() if gx is not None else None, gw.cpu(), gb.cpu() if gb is not None else None)


@pytest.mark.parametrize("c", [G.RECT_F16_CASES[3], G.UNALIGNED_CASES[2]], ids=G.case_id)
def test_two_backward_calls_are_bit_identical(device, c):
    assert c.KH != c.KW
    inp = G.gaussian_inputs(5, c)
    a = _device_backward(device, c, inp)
    b = _device_backward(device, c, inp)
    for name, p, q in zip(NAMES[1:], a, b):
        assert torch.equal(p, q), name


GUARD = 256   # floats on either side of an output (1 KiB: the outputs stay 16-byte aligned)


def _in_canary(n, device):
    buf = torch.full((n + 2 * GUARD,), 7.25, device=device)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    return bool((buf[:GUARD] == 7.25).all()) and bool((buf[-GUARD:] == 7.25).all())


@pytest.mark.parametrize("c", [G.RECT_F16_CASES[5], G.SQUARE_CASES[3]], ids=G.case_id)
def test_c_abi_writes_inside_its_outputs_and_honours_null(device, c):
    assert c.KH != c.KW or c.KH % 2 == 0
    inp = G.gaussian_inputs(6, c)
    full = _device_backward(device, c, inp)
    L = hip.lib()
    x, w, go, y = (t.to(device) for t in (G.nhwc(inp.x), inp.w, G.nhwc(inp.go), G.nhwc(inp.y)))
    geo = (c.B, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for need_x, need_b in ((True, True), (False, False)):
        bx, gx = _in_canary(x.numel(), device)
        bw, gw = _in_canary(w.numel(), device)
        bb, gb = _in_canary(c.Cout, device)
        nbytes = L.cp_conv2d_backward_workspace_bytes(*geo, int(need_x))
        assert nbytes > 0
        bws = torch.full((nbytes + 2 * GUARD,), 0x5a, dtype=torch.uint8, device=device)
        ws = bws[GUARD:GUARD + nbytes]
        rc = L.cp_conv2d_backward_nhwc(stream, p(x), p(w), p(y), p(go), p(gx) if need_x else None, p(gw), p(gb) if need_b else None,
                                       *geo, p(ws), nbytes)
        assert rc == 0, L.cp_last_error()
        torch.cuda.synchronize()
        assert _guards_intact(bx) and _guards_intact(bw) and _guards_intact(bb), (need_x, need_b)
        assert bool((bws[:GUARD] == 0x5a).all()) and bool((bws[-GUARD:] == 0x5a).all()), (need_x, need_b)
        assert torch.equal(gw.view_as(w).cpu(), full[1]), (need_x, need_b)
        if need_x:
            assert torch.equal(gx.view_as(x).permute(0, 3, 1, 2).cpu(), full[0]) and torch.equal(gb.cpu(), full[2])
        else:   # NULL outputs: the buffers that were not handed in are untouched, whole
            assert bool((bx == 7.25).all()) and bool((bb == 7.25).all())


def test_expanded_grad_out(device):
    """out.sum().backward() hands the backward a grad_out of stride 0 on every axis."""
    c = G.RECT_F16_CASES[3]
    inp, _ = G.dyadic_reference(c, True, True)
    ones = torch.ones_like(inp.go)
    exp = G.reference(inp.x, inp.w, inp.bias, ones, c.stride, c.pad, relu=True)
    xd = inp.x.to(device).requires_grad_(True)
    wd, bd = inp.w.to(device).requires_grad_(True), inp.bias.to(device).requires_grad_(True)
    out = conv.conv2d(xd, wd, bd, c.stride, c.pad, relu=True)
    out.sum().backward()
    _equal((out.detach().cpu(), xd.grad.cpu(), wd.grad.cpu(), bd.grad.cpu()), exp, "expanded grad_out")


def test_x_is_a_channel_slice(device):
    """x = big[:, 4:4+Cin]: neither NCHW-contiguous nor channels_last; the gradient lands in the slice and nowhere else."""
    c = G.UNALIGNED_CASES[2]
    inp, exp = G.dyadic_reference(c, False, True)
    assert c.B > 1   # (with one image a channel slice of an NCHW tensor is still one contiguous block)
    for channels_last in (False, True):
        big = torch.full((c.B, c.Cin + 8, c.H, c.W), 2.0)
        big[:, 4:4 + c.Cin] = inp.x
        big = _x_on(device, big, channels_last).requires_grad_(True)
        x = big[:, 4:4 + c.Cin]
        assert not x.is_contiguous() and not x.is_contiguous(memory_format=torch.channels_last)
        wd, bd = inp.w.to(device).requires_grad_(True), inp.bias.to(device).requires_grad_(True)
        out = conv.conv2d(x, wd, bd, c.stride, c.pad)
        out.backward(inp.go.to(device))
        gbig = big.grad.cpu()
        _equal((out.detach().cpu(), gbig[:, 4:4 + c.Cin], wd.grad.cpu(), bd.grad.cpu()), exp, "channel slice cl=%d" % channels_last)
        assert not gbig[:, :4].any() and not gbig[:, 4 + c.Cin:].any()


def test_use_hip_convs_rectangular_and_patchify_sgd_step(device):
    torch.manual_seed(4)
    ref = nn.Sequential(nn.Conv2d(32, 32, (1, 7), padding=0), nn.Conv2d(32, 32, (7, 1)), nn.Conv2d(32, 64, 4, 4)).double()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 32, 14, 18, generator=g)
    target = torch.randn(2, 64, 2, 3, generator=g)
    lr = 0.1
    dnet = copy.deepcopy(ref).float().to(device)
    params = dict(dnet.named_parameters())
    converted, skipped = conv.use_hip_convs(dnet)
    assert converted == ["0", "1", "2"] and not skipped and all(type(m) is conv.Conv2d for m in dnet)
    assert all(p is params[n] for n, p in dnet.named_parameters())
    opt = torch.optim.SGD(dnet.parameters(), lr=lr)
    opt.zero_grad()
    out = dnet(x.to(device))
    assert out.shape == target.shape
    ((out - target.to(device)) ** 2).mean().backward()
    dev_grads = {n: p.grad.detach().cpu() for n, p in dnet.named_parameters()}
    opt.step()
    p0 = {n: p.detach().clone() for n, p in ref.named_parameters()}
    ((ref(x.double()) - target.double()) ** 2).mean().backward()
    for n, p in ref.named_parameters():
        gc = p.grad
        scale = float(gc.abs().max())
        err = float((dev_grads[n].double() - gc).abs().max())
        print("%s: grad err %.3g, max |ref| %.3g" % (n, err, scale))
        assert scale > 0 and err <= 1e-3 * scale, n
        stepped = p0[n] - lr * gc
        assert float((params[n].detach().cpu().double() - stepped).abs().max()) <= 1e-3 * lr * scale + 1e-6, n


def test_refused_geometry_raises_before_any_launch(device, monkeypatch):
    """What the backward refuses, the forward refuses: NotImplementedError, and neither a workspace nor a kernel was asked for."""
    calls = []
    real_ws, real_fwd = _abi._workspace, hip.conv2d_nhwc
    monkeypatch.setattr(_abi, "_workspace", lambda *a, **k: calls.append("workspace") or real_ws(*a, **k))
    monkeypatch.setattr(hip, "conv2d_nhwc", lambda *a, **k: calls.append("forward") or real_fwd(*a, **k))
    x = torch.ones(1, 32, 12, 12, device=device, requires_grad=True)
    w = lambda kh, kw: torch.ones(8, 32, kh, kw, device=device, requires_grad=True)
    for weight, stride, pad in ((w(8, 3), 1, 0), (w(3, 8), 1, 0), (w(3, 3), 5, 1), (w(3, 1), 1, 1), (w(1, 3), 1, 1), (w(2, 2), 1, 2),
                                (w(3, 3), 0, 1)):
        with pytest.raises(NotImplementedError, match="conv2d: geometry outside"):
            conv.conv2d(x, weight, None, stride, pad)
    with pytest.raises(NotImplementedError, match="conv2d: in_channels = 6"):
        conv.conv2d(torch.ones(1, 6, 12, 12, device=device), torch.ones(8, 6, 3, 3, device=device), None, 1, 1)
    assert calls == []
    # the spies do see an accepted call, forward and backward
    conv.conv2d(x, w(3, 1), None, 1, 0).sum().backward()
    assert calls.count("forward") == 1 and calls.count("workspace") >= 2
