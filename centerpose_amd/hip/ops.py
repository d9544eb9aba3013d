"""The stand-alone operators: DCNv2 forward / backward, the pose heads, conv2d, batch and group norm, the GRU gate, the
transposed convolutions, max-pool and the stem's gradient.  Each wrapper checks shapes, allocates results and the
workspace, and hands device pointers and the current stream to one entry point."""
from ctypes import c_int, c_void_p

import torch

from . import _abi


def _conv_out(H, W, kh, kw, sh, sw, ph, pw, dh=1, dw=1):
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def _precision(op, name):
    """The C ABI's value of a backward pass's ``precision`` argument (``op``: the operator named in the refusal)."""
    if name not in _abi.PRECISIONS:
        raise ValueError("%s: precision must be one of %s, got %r" % (op, sorted(_abi.PRECISIONS), name))
    return _abi.PRECISIONS[name]


def _precision_mask(what, op, symbol, precision, *ints):
    """The three ``*_precision_mask`` queries: ``symbol(*ints, precision)``, a negative answer being a refusal of ``what``."""
    rc = getattr(_abi.lib(), symbol)(*map(int, ints), _precision(op, precision))
    if rc < 0:
        _abi._refuse(what)
    return rc


def dcn_v2_forward(input, weight, bias, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group):
    """Same 14-argument signature as the reference's ``_ext.dcn_v2_forward`` (DCNv2/src/vision.cpp:5)."""
    L = _abi.lib()
    input, weight, bias, offset, mask = map(_abi._dev, (input, weight, bias, offset, mask))
    B, C, H, W = input.shape
    Co = weight.shape[0]
    Ho, Wo = _conv_out(H, W, kh, kw, sh, sw, ph, pw, dh, dw)  # dcn_v2_cuda.cu:75-76
    if Ho < 1 or Wo < 1:
        raise RuntimeError("dcn_v2_forward: empty output")
    _abi._check_shapes("dcn_v2_forward", (  # the reference's AT_ASSERTM shape checks (dcn_v2_cuda.cu:60-66)
        ("weight", weight, (Co, C, kh, kw)), ("bias", bias, (Co,)),
        ("offset", offset, (B, deformable_group * 2 * kh * kw, Ho, Wo)), ("mask", mask, (B, deformable_group * kh * kw, Ho, Wo))))
    out = torch.empty(B, Co, Ho, Wo, device=input.device, dtype=torch.float32)
    ws = _abi._workspace(L.cp_dcnv2_workspace_bytes(B, C, H, W, Co), input.device)
    rc = L.cp_dcnv2_forward(_abi._stream(), *_abi._ptrs(input, weight, bias, offset, mask, out),
                            B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, _abi._ptr(ws), ws.numel())
    _abi._check(rc, "cp_dcnv2_forward")
    return out


_deterministic = False
_warned_nondeterministic = False


def set_deterministic(flag):
    """Process-wide default of ``dcn_v2_backward``'s ``deterministic`` argument (False at import): with it every gradient
    of a training step is bitwise reproducible from run to run.  Returns the previous value."""
    global _deterministic
    prev, _deterministic = _deterministic, bool(flag)
    return prev


def deterministic():
    return _deterministic


def dcn_backward_is_fast(C, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group):
    """The geometry cp_dcnv2_backward_det covers (dcn_bwd.hip: cp_dcn_backward_fast)."""
    return (kh, kw, sh, sw, ph, pw, dh, dw, deformable_group) == (3, 3, 1, 1, 1, 1, 1, 1, 1) and C % 16 == 0


def resolve_deterministic(requested, fast, own_flag, torch_flag, torch_warn_only, what=""):
    """Which DCNv2 backward runs (pure: no device, no globals).  ``requested``: the call's ``deterministic`` argument (None:
    ``own_flag or torch_flag``); ``fast``: the geometry is one the deterministic kernels cover.  Returns (use the
    deterministic path, warn that the atomic path runs instead).  A deterministic request for any other geometry raises
    RuntimeError, as torch does for an operator without a deterministic implementation -- unless it came from torch's flag
    alone and torch's warn_only is set."""
    want = (own_flag or torch_flag) if requested is None else bool(requested)
    if not want:
        return False, False
    if fast:
        return True, False
    if requested is None and not own_flag and torch_warn_only:
        return False, True
    raise RuntimeError("dcn_v2_backward does not have a deterministic implementation for %s: the deterministic path covers "
                       "3x3 / stride 1 / pad 1 / dilation 1 / deformable_group 1 / C %% 16 == 0.  Pass deterministic=False, or "
                       "turn off hip.set_deterministic / torch.use_deterministic_algorithms." % (what or "this geometry"))


def dcn_backward_precision_mask(B, C, H, W, Co, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, deformable_group=1,
                                deterministic=False, precision="f16x3"):
    """What ``dcn_v2_backward(..., precision=precision)`` runs in f16x3 for a shape (cp_dcnv2_backward_prec_mask; host
    arithmetic, no device): bit 0 = the weight gradient, bit 1 = grad_col.  0 for "f32" and outside the fast geometry."""
    return _precision_mask("dcn_backward_precision_mask", "dcn_v2_backward", "cp_dcnv2_backward_prec_mask", precision,
                           B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, bool(deterministic))


def dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group,
                    workspace=None, deterministic=None, precision="f32"):
    """Same 15-argument signature as the reference's ``_ext.dcn_v2_backward`` (DCNv2/src/vision.cpp:6, dcn_v2.h:48-80):
    returns [grad_input, grad_offset, grad_mask, grad_weight, grad_bias], float32 on the input's device.  ``workspace`` (a
    uint8 device tensor of at least the queried size) may be passed to skip the allocation; a smaller one is an error.
    ``deterministic``: True runs cp_dcnv2_backward_det (grad_input summed in a fixed order, no float atomics: all five
    gradients bitwise reproducible; a larger workspace), False cp_dcnv2_backward, None (default) resolves at call time to
    ``hip.deterministic() or torch.are_deterministic_algorithms_enabled()`` -- see resolve_deterministic.
    ``precision``: "f32" (the two calls above, bit for bit) or "f16x3": on the fast geometry, with either ``deterministic``
    value, the weight gradient and grad_col run in split binary16 (cp_dcnv2_backward_prec; ``dcn_backward_precision_mask``
    tells what a shape gets); any other geometry runs float32."""
    global _warned_nondeterministic
    prec = _precision("dcn_v2_backward", precision)
    L = _abi.lib()
    input, weight, bias, offset, mask, grad_output = map(_abi._dev, (input, weight, bias, offset, mask, grad_output))
    B, C, H, W = input.shape
    Co = weight.shape[0]
    Ho, Wo = _conv_out(H, W, kh, kw, sh, sw, ph, pw, dh, dw)  # dcn_v2_cuda.cu:242-243
    if Ho < 1 or Wo < 1:
        raise RuntimeError("dcn_v2_backward: empty output")
    _abi._check_shapes("dcn_v2_backward", (
        ("weight", weight, (Co, C, kh, kw)), ("bias", bias, (Co,)),
        ("offset", offset, (B, deformable_group * 2 * kh * kw, Ho, Wo)), ("mask", mask, (B, deformable_group * kh * kw, Ho, Wo)),
        ("grad_output", grad_output, (B, Co, Ho, Wo))))
    geo = (kh, kw, sh, sw, ph, pw, dh, dw, deformable_group)
    det, warn = resolve_deterministic(
        deterministic, dcn_backward_is_fast(C, *geo), _deterministic, torch.are_deterministic_algorithms_enabled(),
        torch.is_deterministic_algorithms_warn_only_enabled(),
        "kernel %dx%d, stride (%d, %d), padding (%d, %d), dilation (%d, %d), deformable_group %d, C = %d" % (*geo, C))
    if warn and not _warned_nondeterministic:
        import warnings

        _warned_nondeterministic = True
        warnings.warn("dcn_v2_backward has no deterministic implementation for this geometry; running the float-atomic path "
                      "(torch.use_deterministic_algorithms(True, warn_only=True))")
    grads = [torch.empty_like(t) for t in (input, offset, mask, weight, bias)]
    if prec == _abi.PRECISIONS["f32"]:
        query, call = ((L.cp_dcnv2_backward_det_workspace_bytes, L.cp_dcnv2_backward_det) if det else
                       (L.cp_dcnv2_backward_workspace_bytes, L.cp_dcnv2_backward))
        tail = ()
    else:
        query, call, tail = L.cp_dcnv2_backward_prec_workspace_bytes, L.cp_dcnv2_backward_prec, (int(det), prec)
    workspace = _abi._workspace(query(B, C, H, W, Co, *geo, *tail), input.device, "dcn_v2_backward", last_error=False, given=workspace)
    rc = call(_abi._stream(), *_abi._ptrs(input, weight, offset, mask, grad_output, *grads), B, C, H, W, Co, *geo, *tail,
              _abi._ptr(workspace), workspace.numel() * workspace.element_size())
    _abi._check(rc, "cp_dcnv2_backward_prec" if tail else "cp_dcnv2_backward_det" if det else "cp_dcnv2_backward")
    return grads


def dcn_v2_backward_f32(input, weight, bias, offset, mask, grad_output, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group,
                        workspace=None, deterministic=None):
    """``dcn_v2_backward`` without the ``precision`` argument: what the package exports as ``hip.dcn_v2_backward`` (its
    recorded signature); ``hip.ops.dcn_v2_backward`` is the operator with the argument."""
    return dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group,
                           workspace=workspace, deterministic=deterministic, precision="f32")


def _heads_args(feat, params):
    """Shape checks and the pointer tables of a pose_heads call.  ``params``: per head (w0 [hid,Cin,3,3], b0 [hid],
    w1 [classes,hid,1,1], b1 [classes])."""
    B, Cin, H, W = feat.shape
    if len(params) < 1:
        raise RuntimeError("pose_heads: at least one head is needed")
    hid = params[0][0].shape[0]
    flat, classes = [], []
    for i, (w0, b0, w1, b1) in enumerate(params):
        w0, b0, w1, b1 = map(_abi._dev, (w0, b0, w1, b1))
        c = w1.shape[0]
        _abi._check_shapes("pose_heads", (("head %d w0" % i, w0, (hid, Cin, 3, 3)), ("head %d b0" % i, b0, (hid,)),
                                          ("head %d w1" % i, w1, (c, hid, 1, 1)), ("head %d b1" % i, b1, (c,))))
        flat.append((w0, b0, w1, b1))
        classes.append(int(c))
    n = len(flat)
    tables = [(c_void_p * n)(*[p[k].data_ptr() for p in flat]) for k in range(4)]
    return flat, tables, (c_int * n)(*classes), classes, (B, H, W, Cin, hid)


def pose_heads_chunk_images(B, H, W, hid):
    """Images whose hidden layer pose_heads_backward materialises at a time (cp_pose_heads_chunk_images)."""
    return int(_abi.lib().cp_pose_heads_chunk_images(int(B), int(H), int(W), int(hid)))


def pose_heads_forward(feat, params):
    """The prediction-head block conv3x3 -> ReLU -> conv1x1 of every head on one feature map (cp_pose_heads_forward).
    ``feat`` [B,Cin,H,W] (NCHW-contiguous or channels_last; the kernels read NHWC), ``params`` a list of (w0, b0, w1, b1)
    per head -> list of [B,classes_i,H,W] raw logits."""
    L = _abi.lib()
    feat = _abi._nhwc_view(feat)
    flat, tables, cls_arr, classes, (B, H, W, Cin, hid) = _heads_args(feat, params)
    outs = [torch.empty(B, c, H, W, device=feat.device, dtype=torch.float32) for c in classes]
    optr = (c_void_p * len(outs))(*[t.data_ptr() for t in outs])
    ws = _abi._workspace(L.cp_pose_heads_forward_workspace_bytes(B, H, W, Cin, hid, len(outs), cls_arr), feat.device,
                         "pose_heads_forward")
    rc = L.cp_pose_heads_forward(_abi._stream(), _abi._ptr(feat), len(outs), *tables, cls_arr, optr, B, H, W, Cin, hid,
                                 _abi._ptr(ws), ws.numel())
    _abi._check(rc, "cp_pose_heads_forward")
    return outs


def pose_heads_backward(feat, params, grad_outs, need_feat_grad=True, grad_feat=None):
    """Gradients of pose_heads_forward (cp_pose_heads_backward).  ``grad_outs``: per head a [B,classes_i,H,W] tensor or None (a
    head the loss does not use: zero parameter gradients, nothing added to grad_feat).  Returns (grad_feat, grads) with
    grads[i] = (grad_w0, grad_b0, grad_w1, grad_b1); grad_feat is a [B,Cin,H,W] channels_last tensor, or None when
    ``need_feat_grad`` is false (the data-gradient contraction is then not launched).  ``grad_feat``: an optional
    channels_last buffer to write into.  Float32 and bitwise reproducible.  ``ops.pose_heads_backward_prec`` is the same
    operator with a ``precision`` argument."""
    return pose_heads_backward_prec(feat, params, grad_outs, need_feat_grad=need_feat_grad, grad_feat=grad_feat, precision="f32")


def pose_heads_backward_prec(feat, params, grad_outs, need_feat_grad=True, grad_feat=None, precision="f32"):
    """``pose_heads_backward`` with the arithmetic of its matrix products as an argument.  ``precision``: "f32" (exact float32:
    cp_pose_heads_backward, the bits of ``pose_heads_backward``) or "f16x3" (cp_pose_heads_backward_prec: the recomputed hidden
    layer, the 3x3 weight gradient and the data gradient of every head on split-binary16 matrix instructions, float32-class
    accuracy and bitwise reproducible; the gate, grad_w1 and the bias gradients stay float32 --
    ``pose_heads_backward_precision_mask`` tells what a shape gets).  Reached as ``hip.ops.pose_heads_backward_prec``: the
    ``hip`` package's own list of names and the signature of ``hip.pose_heads_backward`` are kept as they were."""
    L = _abi.lib()
    prec = _precision("pose_heads_backward", precision)
    feat = _abi._nhwc_view(feat)
    flat, tables, cls_arr, classes, (B, H, W, Cin, hid) = _heads_args(feat, params)
    n = len(flat)
    if len(grad_outs) != n:
        raise RuntimeError("pose_heads_backward: %d gradients for %d heads" % (len(grad_outs), n))
    gos = []
    for i, g in enumerate(grad_outs):
        g = _abi._dev_opt(g)
        _abi._check_shapes("pose_heads_backward", [("grad_out %d" % i, g, (B, classes[i], H, W))])
        gos.append(g)
    grads = [tuple(torch.empty_like(t) for t in p) for p in flat]
    gtab = [(c_void_p * n)(*[g[k].data_ptr() for g in grads]) for k in range(4)]
    goptr = (c_void_p * n)(*[g.data_ptr() if g is not None else None for g in gos])
    if need_feat_grad and grad_feat is None:
        grad_feat = torch.empty_like(feat, memory_format=torch.channels_last)
    if need_feat_grad and not (grad_feat.is_cuda and grad_feat.dtype == torch.float32 and grad_feat.shape == feat.shape and
                               grad_feat.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("pose_heads_backward: grad_feat must be a float32 channels_last tensor of feat's shape")
    gfp = _abi._ptr(grad_feat) if need_feat_grad else c_void_p(0)
    query, call, tail = (("cp_pose_heads_backward_prec_workspace_bytes", "cp_pose_heads_backward_prec", (prec,)) if prec else
                         ("cp_pose_heads_backward_workspace_bytes", "cp_pose_heads_backward", ()))
    ws = _abi._workspace(getattr(L, query)(B, H, W, Cin, hid, n, cls_arr, *tail), feat.device, "pose_heads_backward")
    rc = getattr(L, call)(_abi._stream(), _abi._ptr(feat), n, *tables, cls_arr, goptr, *gtab, gfp, B, H, W, Cin, hid, *tail,
                          _abi._ptr(ws), ws.numel())
    _abi._check(rc, call)
    return (grad_feat if need_feat_grad else None), grads


def pose_heads_backward_precision_mask(B, H, W, Cin, hid, precision="f16x3"):
    """What ``pose_heads_backward_prec(..., precision=precision)`` runs in f16x3 for a shape (cp_pose_heads_backward_prec_mask;
    host arithmetic): bit 0 = the 3x3 weight gradient, bit 1 = the data gradient, bit 2 = the recomputed hidden layer.  0 for
    "f32".  Raises RuntimeError for a shape the operator refuses."""
    return _precision_mask("pose_heads_backward_precision_mask", "pose_heads_backward", "cp_pose_heads_backward_prec_mask", precision,
                           B, H, W, Cin, hid)


def conv2d_nhwc(x, w, scale=None, shift=None, residual=None, stride=1, pad=0, act=0):
    """x [B,H,W,Cin] NHWC, w [Cout,Cin,KH,KW] -> [B,Ho,Wo,Cout] NHWC (unit-test entry of the igemm kernel)."""
    L = _abi.lib()
    x, w = _abi._dev(x), _abi._dev(w)
    B, H, W, Cin = x.shape
    Cout, _, KH, KW = w.shape
    Ho, Wo = _conv_out(H, W, KH, KW, stride, stride, pad, pad)
    out = torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=torch.float32)
    ws = _abi._workspace(L.cp_conv2d_workspace_bytes(Cin, Cout, KH, KW), x.device)
    scale, shift, residual = map(_abi._dev_opt, (scale, shift, residual))
    rc = L.cp_conv2d_nhwc(_abi._stream(), *_abi._ptrs(x, w, scale, shift, residual, out),
                          B, H, W, Cin, Cout, KH, KW, stride, pad, act, _abi._ptr(ws), ws.numel())
    _abi._check(rc, "cp_conv2d_nhwc")
    return out


def conv2d_backward(x, w, grad_out, stride=1, pad=0, y=None, need_x_grad=True, need_bias_grad=True):
    """Gradients of ``conv2d_nhwc(x, w, shift=bias)`` (cp_conv2d_backward_nhwc): x [B,H,W,Cin] NHWC, w [Cout,Cin,KH,KW],
    grad_out [B,Ho,Wo,Cout] NHWC -> (grad_x [B,H,W,Cin] | None, grad_w [Cout,Cin,KH,KW], grad_bias [Cout] | None).  ``y``: the
    activated forward output when the layer ended in a ReLU (grad_out is gated by y > 0).  Float32 and bitwise reproducible.
    ``ops.conv2d_backward_prec`` is the same operator with a ``precision`` argument."""
    return conv2d_backward_prec(x, w, grad_out, stride=stride, pad=pad, y=y, need_x_grad=need_x_grad, need_bias_grad=need_bias_grad,
                                precision="f32")


def conv2d_backward_prec(x, w, grad_out, stride=1, pad=0, y=None, need_x_grad=True, need_bias_grad=True, precision="f32"):
    """``conv2d_backward`` with the arithmetic of its matrix products as an argument.  ``precision``: "f32" (exact float32:
    cp_conv2d_backward_nhwc, the bits of ``conv2d_backward``) or "f16x3" (cp_conv2d_backward_prec_nhwc: the MFMA path's weight
    and data gradient on split-binary16 matrix instructions, float32-class accuracy and bitwise reproducible; the other paths
    stay float32 -- ``conv2d_backward_precision_mask`` tells which).  Reached as ``hip.ops.conv2d_backward_prec``: the ``hip``
    package's own list of names and the signature of ``hip.conv2d_backward`` are kept as they were."""
    L = _abi.lib()
    prec = _precision("conv2d_backward", precision)
    x, w, grad_out, y = _abi._dev(x), _abi._dev(w), _abi._dev(grad_out), _abi._dev_opt(y)
    if x.dim() != 4 or w.dim() != 4 or w.shape[1] != x.shape[3]:
        raise RuntimeError("conv2d_backward: x must be [B,H,W,Cin] and w [Cout,Cin,KH,KW], got %s and %s"
                           % (tuple(x.shape), tuple(w.shape)))
    B, H, W, Cin = x.shape
    Cout, _, KH, KW = w.shape
    stride, pad = int(stride), int(pad)
    query, call, tail = (("cp_conv2d_backward_prec_workspace_bytes", "cp_conv2d_backward_prec_nhwc", (prec,)) if prec else
                         ("cp_conv2d_backward_workspace_bytes", "cp_conv2d_backward_nhwc", ()))
    ws = _abi._workspace(getattr(L, query)(B, H, W, Cin, Cout, KH, KW, stride, pad, int(bool(need_x_grad)), *tail), x.device,
                         "conv2d_backward")
    Ho, Wo = _conv_out(H, W, KH, KW, stride, stride, pad, pad)
    _abi._check_shapes("conv2d_backward", (("grad_out", grad_out, (B, Ho, Wo, Cout)), ("y", y, (B, Ho, Wo, Cout))))
    grad_x = torch.empty_like(x) if need_x_grad else None
    grad_w = torch.empty_like(w)
    grad_b = torch.empty(Cout, device=x.device, dtype=torch.float32) if need_bias_grad else None
    rc = getattr(L, call)(_abi._stream(), *_abi._ptrs(x, w, y, grad_out, grad_x, grad_w, grad_b), B, H, W, Cin, Cout, KH, KW, stride,
                          pad, *tail, _abi._ptr(ws), ws.numel())
    _abi._check(rc, call)
    return grad_x, grad_w, grad_b


def conv2d_backward_precision_mask(B, H, W, Cin, Cout, KH, KW, stride=1, pad=0, precision="f16x3"):
    """What ``conv2d_backward_prec(..., precision=precision)`` runs in f16x3 for a geometry (cp_conv2d_backward_prec_mask; host
    arithmetic): bit 0 = the weight gradient, bit 1 = the data gradient.  0 for "f32" and for the low-channel and generic paths.
    Raises RuntimeError for a geometry the operator refuses."""
    return _precision_mask("conv2d_backward_precision_mask", "conv2d_backward", "cp_conv2d_backward_prec_mask", precision,
                           B, H, W, Cin, Cout, KH, KW, stride, pad)


CONV_BWD_GENERIC, CONV_BWD_MFMA, CONV_BWD_LOWC = 0, 1, 2   # include/centerpose_hip.h: CP_CONV_BWD_*


def conv2d_backward_path(B, H, W, Cin, Cout, KH, KW, stride=1, pad=0):
    """The kernels ``conv2d_backward`` takes for a geometry (cp_conv2d_backward_path; host arithmetic, no device involved):
    CONV_BWD_MFMA (KH == KW in {1, 3}, stride 1 | 2, pad == KH // 2, Cin % 32 == 0), CONV_BWD_LOWC (3x3, pad 1, stride 1 | 2,
    16 -> 16 | 32 channels and at least 4096 output pixels: dla_34's level0 / level1) or CONV_BWD_GENERIC (everything else the
    operator accepts: correct, not fast).  Raises RuntimeError for a geometry the operator refuses."""
    rc = _abi.lib().cp_conv2d_backward_path(int(B), int(H), int(W), int(Cin), int(Cout), int(KH), int(KW), int(stride), int(pad))
    if rc < 0:
        _abi._refuse("conv2d_backward_path")
    return rc


def _norm_ws(what, query, x, *groups):
    """The geometry (B, H, W, C, *groups) and the workspace of a batch_norm / group_norm call on x."""
    _abi._on_device(x)
    if x.dim() != 4:
        raise RuntimeError("%s: x must be [B,H,W,C], got %s" % (what, tuple(x.shape)))
    geo = tuple(x.shape) + groups
    return geo, _abi._workspace(query(*geo), x.device, what)


def _bn_vec(t, C, name):
    t = _abi._dev_opt(t)
    _abi._check_shapes("batch_norm", [(name, t, (C,))])
    return t


def batch_norm_forward(x, gamma=None, beta=None, residual=None, running_mean=None, running_var=None, training=True,
                       momentum=0.1, eps=1e-5, act=0):
    """``act(batch_norm(x) [+ residual])`` (cp_batchnorm_forward_nhwc): x, residual [B,H,W,C] NHWC, gamma / beta [C] or None
    (1 / 0) -> (y [B,H,W,C], save_mean [C], save_invstd [C]).  ``training``: the batch's statistics, and running_mean /
    running_var (float32 device tensors, when given) are updated IN PLACE with ``momentum``; otherwise they are the
    statistics.  act 0 none, 1 relu.  Float32 and bitwise reproducible."""
    L = _abi.lib()
    geo, ws = _norm_ws("batch_norm", L.cp_batchnorm_workspace_bytes, x)
    x = _abi._dev(x)
    C = geo[3]
    gamma, beta = _bn_vec(gamma, C, "gamma"), _bn_vec(beta, C, "beta")
    residual = _abi._dev_opt(residual)
    _abi._check_shapes("batch_norm", [("residual", residual, x.shape)])
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (C,)):
            raise RuntimeError("batch_norm: %s must be a contiguous float32 [%d] tensor on the HIP device" % (name, C))
    y = torch.empty_like(x)
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    invstd = torch.empty_like(mean)
    rc = L.cp_batchnorm_forward_nhwc(_abi._stream(), *_abi._ptrs(x, gamma, beta, residual, running_mean, running_var, y, mean,
                                                                 invstd), *geo, int(bool(training)),
                                     float(momentum), float(eps), int(act), _abi._ptr(ws), ws.numel())
    _abi._check(rc, "cp_batchnorm_forward_nhwc")
    return y, mean, invstd


def batch_norm_backward(x, grad_out, save_mean, save_invstd, gamma=None, y=None, training=True, need_x_grad=True,
                        need_residual_grad=False, need_gamma_grad=True, need_beta_grad=True):
    """Gradients of batch_norm_forward (cp_batchnorm_backward_nhwc) -> (grad_x, grad_residual, grad_gamma, grad_beta), None
    where not asked for.  ``y``: the activated forward output when act was 1 (grad_out is gated by y > 0); without it
    grad_residual is ``grad_out`` itself, not a copy.  Float32 and bitwise reproducible."""
    L = _abi.lib()
    geo, ws = _norm_ws("batch_norm", L.cp_batchnorm_workspace_bytes, x)
    x, grad_out, y = _abi._dev(x), _abi._dev(grad_out), _abi._dev_opt(y)
    C = geo[3]
    _abi._check_shapes("batch_norm_backward", (("grad_out", grad_out, x.shape), ("y", y, x.shape)))
    gamma, save_mean, save_invstd = _bn_vec(gamma, C, "gamma"), _bn_vec(save_mean, C, "save_mean"), _bn_vec(save_invstd, C, "save_invstd")
    grad_x = torch.empty_like(x) if need_x_grad else None
    grad_res = torch.empty_like(x) if need_residual_grad and y is not None else None
    grad_g = torch.empty(C, device=x.device, dtype=torch.float32) if need_gamma_grad else None
    grad_b = torch.empty(C, device=x.device, dtype=torch.float32) if need_beta_grad else None
    if need_x_grad or grad_res is not None or need_gamma_grad or need_beta_grad:
        rc = L.cp_batchnorm_backward_nhwc(_abi._stream(), *_abi._ptrs(x, y, grad_out, gamma, save_mean, save_invstd, grad_x,
                                                                      grad_res, grad_g, grad_b), *geo,
                                          int(bool(training)), _abi._ptr(ws), ws.numel())
        _abi._check(rc, "cp_batchnorm_backward_nhwc")
    if need_residual_grad and y is None:
        grad_res = grad_out
    return grad_x, grad_res, grad_g, grad_b


def group_norm_forward(x, num_groups, gamma=None, beta=None, eps=1e-5, act=0):
    """``act(group_norm(x))`` (cp_groupnorm_forward_nhwc): x [B,H,W,C] NHWC, gamma / beta [C] or None (1 / 0) -> (y [B,H,W,C],
    save_mean [B,G], save_invstd [B,G]).  act 0 none, 1 relu.  ``C % 4 == 0`` and ``C / G`` 1, 2 or a multiple of 4.  Float32
    and bitwise reproducible."""
    L = _abi.lib()
    geo, ws = _norm_ws("group_norm", L.cp_groupnorm_workspace_bytes, x, int(num_groups))
    x = _abi._dev(x)
    B, C, G = geo[0], geo[3], geo[4]
    gamma, beta = _bn_vec(gamma, C, "gamma"), _bn_vec(beta, C, "beta")
    y = torch.empty_like(x)
    mean = torch.empty(B, G, device=x.device, dtype=torch.float32)
    invstd = torch.empty_like(mean)
    rc = L.cp_groupnorm_forward_nhwc(_abi._stream(), *_abi._ptrs(x, gamma, beta, y, mean, invstd), *geo,
                                     float(eps), int(act), _abi._ptr(ws), ws.numel())
    _abi._check(rc, "cp_groupnorm_forward_nhwc")
    return y, mean, invstd


def group_norm_backward(x, grad_out, num_groups, save_mean, save_invstd, gamma=None, y=None, need_x_grad=True,
                        need_gamma_grad=True, need_beta_grad=True):
    """Gradients of group_norm_forward (cp_groupnorm_backward_nhwc) -> (grad_x, grad_gamma, grad_beta), None where not asked
    for.  ``y``: the activated forward output when act was 1 (grad_out is gated by y > 0).  Float32 and bitwise reproducible."""
    L = _abi.lib()
    geo, ws = _norm_ws("group_norm", L.cp_groupnorm_workspace_bytes, x, int(num_groups))
    x, grad_out, y = _abi._dev(x), _abi._dev(grad_out), _abi._dev_opt(y)
    B, C, G = geo[0], geo[3], geo[4]
    _abi._check_shapes("group_norm_backward", (("grad_out", grad_out, x.shape), ("y", y, x.shape)))
    gamma = _bn_vec(gamma, C, "gamma")
    save_mean, save_invstd = _abi._dev(save_mean), _abi._dev(save_invstd)
    _abi._check_shapes("group_norm_backward", (("save_mean", save_mean, (B, G)), ("save_invstd", save_invstd, (B, G))))
    grad_x = torch.empty_like(x) if need_x_grad else None
    grad_g = torch.empty(C, device=x.device, dtype=torch.float32) if need_gamma_grad else None
    grad_b = torch.empty(C, device=x.device, dtype=torch.float32) if need_beta_grad else None
    if need_x_grad or need_gamma_grad or need_beta_grad:
        rc = L.cp_groupnorm_backward_nhwc(_abi._stream(), *_abi._ptrs(x, y, grad_out, gamma, save_mean, save_invstd, grad_x, grad_g,
                                                                      grad_b), *geo, _abi._ptr(ws), ws.numel())
        _abi._check(rc, "cp_groupnorm_backward_nhwc")
    return grad_x, grad_g, grad_b


def _gru_args(x3, h3, hprev):
    _abi._on_device(x3)
    if x3.dim() < 2 or x3.shape[-1] % 3:
        raise RuntimeError("gru_gate: x3 must be [..., 3 * Ch], got %s" % (tuple(x3.shape),))
    if (h3 is None) != (hprev is None):
        raise RuntimeError("gru_gate: h3 and hprev are given together, or neither (step 0)")
    x3 = _abi._dev(x3)
    Ch = x3.shape[-1] // 3
    lead = tuple(x3.shape[:-1])
    if h3 is not None:
        h3, hprev = _abi._dev(h3), _abi._dev(hprev)
        if h3.shape != x3.shape or tuple(hprev.shape) != lead + (Ch,):
            raise RuntimeError("gru_gate: h3 %s / hprev %s do not match x3 %s" % (tuple(h3.shape), tuple(hprev.shape), tuple(x3.shape)))
    return x3, h3, hprev, lead, x3.numel() // (3 * Ch), Ch


def gru_gate_forward(x3, h3=None, hprev=None):
    """The ConvGRU cell's gate arithmetic (cp_gru_gate_forward): x3 = [Wir x | Wiz x | Win x] (+ biases) and h3 = [Whr h | Whz h |
    Whn h] as [..., 3 Ch], hprev [..., Ch] -> hout [..., Ch] = (1 - z) n + z hprev.  ``h3 = hprev = None``: step 0, h = 0."""
    x3, h3, hprev, lead, M, Ch = _gru_args(x3, h3, hprev)
    hout = torch.empty(lead + (Ch,), device=x3.device, dtype=torch.float32)
    _abi._check(_abi.lib().cp_gru_gate_forward(_abi._stream(), *_abi._ptrs(x3, h3, hprev, hout), M, Ch), "cp_gru_gate_forward")
    return hout


def gru_gate_backward(x3, h3, hprev, grad_hout, need_h3_grad=True, need_hprev_grad=True):
    """Gradients of gru_gate_forward (cp_gru_gate_backward) -> (grad_x3, grad_h3, grad_hprev); the gates are recomputed from
    the inputs.  At step 0 (``h3 = hprev = None``) the two hidden-side gradients are None."""
    x3, h3, hprev, lead, M, Ch = _gru_args(x3, h3, hprev)
    grad_hout = _abi._dev(grad_hout)
    _abi._check_shapes("gru_gate_backward", [("grad_hout", grad_hout, lead + (Ch,))])
    grad_x3 = torch.empty_like(x3)
    grad_h3 = torch.empty_like(x3) if h3 is not None and need_h3_grad else None
    grad_hp = torch.empty_like(grad_hout) if h3 is not None and need_hprev_grad else None
    _abi._check(_abi.lib().cp_gru_gate_backward(_abi._stream(), *_abi._ptrs(x3, h3, hprev, grad_hout, grad_x3, grad_h3, grad_hp),
                                                M, Ch), "cp_gru_gate_backward")
    return grad_x3, grad_h3, grad_hp


def conv_transpose2d(x, w, scale=None, shift=None, act=0):
    """x [B,H,W,Cin] NHWC, w [Cin,Cout,4,4] (ConvTranspose2d(k=4, stride=2, padding=1) layout) -> [B,2H,2W,Cout] NHWC,
    y = act(deconv(x) * scale + shift); act 0 none, 1 relu.  Precision: set_default_precision."""
    L = _abi.lib()
    x, w = _abi._dev(x), _abi._dev(w)
    B, H, W, Cin = x.shape
    if tuple(w.shape[2:]) != (4, 4) or w.shape[0] != Cin:
        raise RuntimeError("conv_transpose2d: weight must be [Cin, Cout, 4, 4], got %s" % (tuple(w.shape),))
    Cout = w.shape[1]
    out = torch.empty(B, 2 * H, 2 * W, Cout, device=x.device, dtype=torch.float32)
    ws = _abi._workspace(L.cp_conv_transpose2d_workspace_bytes(Cin, Cout), x.device)
    scale, shift = _abi._dev_opt(scale), _abi._dev_opt(shift)
    rc = L.cp_conv_transpose2d_nhwc(_abi._stream(), *_abi._ptrs(x, w, scale, shift, out),
                                    B, H, W, Cin, Cout, act, _abi._ptr(ws), ws.numel())
    _abi._check(rc, "cp_conv_transpose2d_nhwc")
    return out


def conv_transpose2d_dw(x, w, f, add=None):
    """IDAUp's depth-wise up-sampling (cp_conv_transpose2d_dw_nhwc): x [B,H,W,C] NHWC, w [C,1,2f,2f] (ConvTranspose2d(C, C, 2f,
    stride=f, padding=f//2, groups=C) layout), add [B,fH,fW,C] or None -> add + up(x), [B,fH,fW,C] NHWC.  Float32."""
    L = _abi.lib()
    x, w = _abi._dev(x), _abi._dev(w)
    f = int(f)
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape) != (x.shape[3], 1, 2 * f, 2 * f):
        raise RuntimeError("conv_transpose2d_dw: x must be [B,H,W,C] and w [C,1,2f,2f], got %s and %s (f = %d)"
                           % (tuple(x.shape), tuple(w.shape), f))
    B, H, W, C = x.shape
    add = _abi._dev_opt(add)
    _abi._check_shapes("conv_transpose2d_dw", [("add", add, (B, f * H, f * W, C))])
    out = torch.empty(B, f * H, f * W, C, device=x.device, dtype=torch.float32)
    rc = L.cp_conv_transpose2d_dw_nhwc(_abi._stream(), *_abi._ptrs(x, w, add, out), B, H, W, C, f)
    _abi._check(rc, "cp_conv_transpose2d_dw_nhwc")
    return out


def conv_transpose2d_backward(x, w, grad_out, stride, pad, groups=1, need_x_grad=True, precision="f32"):
    """Gradients of a bias-free ``ConvTranspose2d`` (cp_conv_transpose2d_backward_nhwc): x [B,H,W,Cin] NHWC, w [Cin,Cout/groups,K,K],
    grad_out [B,stride H,stride W,Cout] NHWC -> (grad_x [B,H,W,Cin] | None, grad_w like w).  Depth-wise (groups == Cin == Cout,
    stride 2 or 4, K = 2 stride, pad = stride / 2) or dense (groups 1, K 4, stride 2, pad 1).  Bitwise reproducible.
    ``precision``: "f32" (exact float32, the plain call) or "f16x3" (cp_conv_transpose2d_backward_prec_nhwc: the dense layer's
    weight and data gradient in split binary16; depth-wise layers stay float32 --
    ``conv_transpose2d_backward_precision_mask`` tells what a geometry gets)."""
    L = _abi.lib()
    prec = _precision("conv_transpose2d_backward", precision)
    x, w, grad_out = _abi._dev(x), _abi._dev(w), _abi._dev(grad_out)
    stride, pad, groups = int(stride), int(pad), int(groups)
    if x.dim() != 4 or w.dim() != 4 or w.shape[0] != x.shape[3] or w.shape[2] != w.shape[3] or groups < 1:
        raise RuntimeError("conv_transpose2d_backward: x must be [B,H,W,Cin] and w [Cin,Cout/groups,K,K], got %s and %s"
                           % (tuple(x.shape), tuple(w.shape)))
    B, H, W, Cin = x.shape
    Cout, K = w.shape[1] * groups, w.shape[2]
    query, call, tail = (("cp_conv_transpose2d_backward_prec_workspace_bytes", "cp_conv_transpose2d_backward_prec_nhwc", (prec,))
                         if prec else ("cp_conv_transpose2d_backward_workspace_bytes", "cp_conv_transpose2d_backward_nhwc", ()))
    ws = _abi._workspace(getattr(L, query)(B, H, W, Cin, Cout, K, stride, pad, groups, int(bool(need_x_grad)), *tail),
                         x.device, "conv_transpose2d_backward")
    _abi._check_shapes("conv_transpose2d_backward", [("grad_out", grad_out, (B, stride * H, stride * W, Cout))])
    grad_x = torch.empty_like(x) if need_x_grad else None
    grad_w = torch.empty_like(w)
    rc = getattr(L, call)(_abi._stream(), *_abi._ptrs(x, w, grad_out, grad_x, grad_w), B, H, W, Cin, Cout, K, stride, pad, groups,
                          *tail, _abi._ptr(ws), ws.numel())
    _abi._check(rc, call)
    return grad_x, grad_w


def conv_transpose2d_backward_f32(x, w, grad_out, stride, pad, groups=1, need_x_grad=True):
    """``conv_transpose2d_backward`` without the ``precision`` argument: what the package exports as
    ``hip.conv_transpose2d_backward`` (its recorded signature); ``hip.ops.conv_transpose2d_backward`` is the operator with the
    argument."""
    return conv_transpose2d_backward(x, w, grad_out, stride, pad, groups, need_x_grad=need_x_grad, precision="f32")


def conv_transpose2d_backward_precision_mask(B, H, W, Cin, Cout, K=4, stride=2, pad=1, groups=1, precision="f16x3"):
    """What ``conv_transpose2d_backward(..., precision=precision)`` runs in f16x3 for a geometry
    (cp_conv_transpose2d_backward_prec_mask; host arithmetic): bit 0 = the weight gradient, bit 1 = the data gradient."""
    return _precision_mask("conv_transpose2d_backward_precision_mask", "conv_transpose2d_backward",
                           "cp_conv_transpose2d_backward_prec_mask", precision, B, H, W, Cin, Cout, K, stride, pad, groups)


def _pool_args(what, x, kernel, stride, pad):
    if x.dim() != 4:
        raise RuntimeError("%s: x must be [B,H,W,C], got %s" % (what, tuple(x.shape)))
    B, H, W, C = x.shape
    kernel, stride, pad = int(kernel), int(stride), int(pad)
    return (B, H, W, C, kernel, stride, pad), _conv_out(H, W, kernel, kernel, stride, stride, pad, pad)


def max_pool2d_forward(x, kernel, stride, pad):
    """``F.max_pool2d`` on an NHWC tensor (cp_maxpool2d_forward_nhwc): x [B,H,W,C] -> [B,Ho,Wo,C].  (kernel, stride, pad) is
    (2, 2, 0), which floors, or (3, 2, 1), padding as -inf; C % 4 == 0.  Bitwise torch's values."""
    x = _abi._dev(x)
    geo, (Ho, Wo) = _pool_args("max_pool2d", x, kernel, stride, pad)
    out = torch.empty(geo[0], max(Ho, 0), max(Wo, 0), geo[3], device=x.device, dtype=torch.float32)
    _abi._check(_abi.lib().cp_maxpool2d_forward_nhwc(_abi._stream(), _abi._ptr(x), _abi._ptr(out), *geo),
                "cp_maxpool2d_forward_nhwc")
    return out


def max_pool2d_backward(x, grad_out, kernel, stride, pad):
    """Gradient of max_pool2d_forward (cp_maxpool2d_backward_nhwc): x [B,H,W,C], grad_out [B,Ho,Wo,C] -> grad_x [B,H,W,C].  The
    winner of every window is recomputed from x (torch's: the first maximum in row-major order); bitwise reproducible."""
    x, grad_out = _abi._dev(x), _abi._dev(grad_out)
    geo, (Ho, Wo) = _pool_args("max_pool2d_backward", x, kernel, stride, pad)
    _abi._check_shapes("max_pool2d_backward", [("grad_out", grad_out, (geo[0], Ho, Wo, geo[3]))])
    grad_x = torch.empty_like(x)
    _abi._check(_abi.lib().cp_maxpool2d_backward_nhwc(_abi._stream(), *_abi._ptrs(x, grad_out, grad_x), *geo),
                "cp_maxpool2d_backward_nhwc")
    return grad_x


def conv2d_stem_backward(x, grad_out, stride=1, y=None, need_bias_grad=True):
    """Weight and bias gradient of a 7x7, padding-3 stem (cp_conv2d_stem_backward): x [B,Cin,H,W] NCHW planes with Cin in 1..3,
    grad_out [B,Ho,Wo,Cout] NHWC -> (grad_w [Cout,Cin,7,7], grad_bias [Cout] | None).  ``y``: the activated forward output when
    the layer ended in a ReLU (grad_out is gated by y > 0).  Float32 and bitwise reproducible; there is no input gradient."""
    L = _abi.lib()
    x, grad_out, y = _abi._dev(x), _abi._dev(grad_out), _abi._dev_opt(y)
    if x.dim() != 4 or grad_out.dim() != 4:
        raise RuntimeError("conv2d_stem_backward: x must be [B,Cin,H,W] and grad_out [B,Ho,Wo,Cout], got %s and %s"
                           % (tuple(x.shape), tuple(grad_out.shape)))
    B, Cin, H, W = x.shape
    Cout, stride = grad_out.shape[3], int(stride)
    # above 64 channels the pair that runs the same kernels over channel blocks (the hourglass's 3 -> 128 stem)
    query, launch = ((L.cp_conv2d_stem_backward_workspace_bytes, L.cp_conv2d_stem_backward) if Cout <= 64 else
                     (L.cp_conv2d_stem_wide_backward_workspace_bytes, L.cp_conv2d_stem_wide_backward))
    ws = _abi._workspace(query(B, H, W, Cin, Cout, stride), x.device, "conv2d_stem_backward")
    want = (B, (H - 1) // stride + 1, (W - 1) // stride + 1, Cout)
    _abi._check_shapes("conv2d_stem_backward", (("grad_out", grad_out, want), ("y", y, want)))
    grad_w = torch.empty(Cout, Cin, 7, 7, device=x.device, dtype=torch.float32)
    grad_b = torch.empty(Cout, device=x.device, dtype=torch.float32) if need_bias_grad else None
    rc = launch(_abi._stream(), *_abi._ptrs(x, grad_out, y, grad_w, grad_b, ws), ws.numel(), B, H, W, Cin, Cout, stride)
    _abi._check(rc, "cp_conv2d_stem_backward")
    return grad_w, grad_b


def _upsample2_args(what, low, big, big_name):
    if low.dim() != 4 or big.dim() != 4:
        raise RuntimeError("%s: low must be [B,H,W,C] and %s [B,2H,2W,C], got %s and %s"
                           % (what, big_name, tuple(low.shape), tuple(big.shape)))
    B, H, W, C = low.shape
    _abi._check_shapes(what, [(big_name, big, (B, 2 * H, 2 * W, C))])
    return B, H, W, C


def upsample2_add_forward(up1, low):
    """The hourglass merge on NHWC tensors (cp_upsample2_add_nhwc): up1 [B,2H,2W,C] + nearest2x(low [B,H,W,C]) -> [B,2H,2W,C];
    C % 4 == 0."""
    up1, low = _abi._dev(up1), _abi._dev(low)
    geo = _upsample2_args("upsample2_add", low, up1, "up1")
    out = torch.empty_like(up1)
    _abi._check_args(_abi.lib().cp_upsample2_add_nhwc(_abi._stream(), *_abi._ptrs(up1, low, out), *geo), "cp_upsample2_add_nhwc")
    return out


def upsample2_add_backward(grad_out, low_shape):
    """Gradient of upsample2_add_forward with respect to ``low`` (cp_upsample2_add_backward_nhwc): grad_out [B,2H,2W,C] ->
    grad_low [B,H,W,C], each 2x2 cell added in a fixed order (bitwise reproducible).  The gradient of ``up1`` is grad_out."""
    grad_out = _abi._dev(grad_out)
    grad_low = torch.empty(tuple(low_shape), device=grad_out.device, dtype=torch.float32)
    geo = _upsample2_args("upsample2_add_backward", grad_low, grad_out, "grad_out")
    _abi._check_args(_abi.lib().cp_upsample2_add_backward_nhwc(_abi._stream(), *_abi._ptrs(grad_out, grad_low), *geo),
                     "cp_upsample2_add_backward_nhwc")
    return grad_low
