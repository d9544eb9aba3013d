"""DCNv2 backward, CPU side (no device): the ABI surface, the shape refusals, the `_ext` shim's entry point, and the
test references themselves (tests/dcn_backward_ref.py) against float64 central differences of the oracle's forward."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from centerpose_amd import hip
from oracle import dcn as odcn
from tests import dcn_backward_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CENTERPOSE_SHAPES = [(64, 64, 128), (128, 128, 64), (256, 256, 32), (256, 128, 32), (512, 256, 16)]  # C, Co, H = W
needs_ref = pytest.mark.skipif(not odcn.have_reference(),
                               reason="oracle/_ref/libdcn_im2col_ref.so absent (built only where the reference tree exists)")


@pytest.fixture(scope="module")
def built():
    ge.build()
    return hip.lib()


def test_header_declares_and_library_exports_backward(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "centerpose_hip.h")).read(), flags=re.S)
    for name in ("cp_dcnv2_backward_workspace_bytes", "cp_dcnv2_backward"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(built, name) and name in hip.exported_symbols()
    assert built.cp_abi_version() == 7


@pytest.mark.parametrize("C,Co,H", CENTERPOSE_SHAPES)
@pytest.mark.parametrize("B", [1, 16, 64])
def test_workspace_query_is_host_arithmetic(built, C, Co, H, B):
    n = built.cp_dcnv2_backward_workspace_bytes(B, C, H, H, Co, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    assert n > 0 and n % 256 == 0
    # the NHWC input stage, its gradient and grad_output transposed are all in it
    assert n >= 4 * B * H * H * (2 * C + Co)


def _call(L, B=1, C=4, H=8, W=8, Co=4, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, dg=1, ws_bytes=1 << 30):
    fake = [ctypes.c_void_p(256)] * 11  # never dereferenced: every refusal comes before any launch
    return L.cp_dcnv2_backward(ctypes.c_void_p(0), *fake[:10], B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg,
                               fake[10], ws_bytes)


@pytest.mark.parametrize("kwargs,msg", [
    (dict(C=6, dg=4), "divisible"),
    (dict(kh=0), "bad shape"),
    (dict(H=2, W=2, ph=0, pw=0, kh=5, kw=5), "empty output"),
    (dict(H=3, W=3, dh=3, ph=0, pw=0), "empty output"),
    (dict(B=0), "bad shape"),
    (dict(sh=0), "bad shape"),
    (dict(B=4096, C=512, H=1024, W=1024), "2^31"),
    (dict(ws_bytes=64), "workspace too small"),
])
def test_backward_refuses_bad_shapes_without_a_device(built, kwargs, msg):
    assert _call(built, **kwargs) == -1  # CP_ERR_INVALID
    assert msg in built.cp_last_error().decode()
    if msg != "workspace too small":
        args = dict(B=1, C=4, H=8, W=8, Co=4, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, dg=1)
        args.update(kwargs)
        assert built.cp_dcnv2_backward_workspace_bytes(*args.values()) == 0


def test_null_gradient_is_refused(built):
    fake = [ctypes.c_void_p(256)] * 11
    fake[7] = ctypes.c_void_p(0)  # grad_mask
    rc = built.cp_dcnv2_backward(ctypes.c_void_p(0), *fake[:10], 1, 4, 8, 8, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1, fake[10], 1 << 30)
    assert rc == -1 and "null" in built.cp_last_error().decode()


def test_ext_backward_signature_and_cpu_refusal():
    from centerpose_amd.lib.models.networks.DCNv2 import _ext

    assert len(inspect.signature(_ext.dcn_v2_backward).parameters) == 15
    x = torch.zeros(1, 2, 4, 4)
    args = (x, torch.zeros(2, 2, 3, 3), torch.zeros(2), torch.zeros(1, 18, 4, 4), torch.zeros(1, 9, 4, 4),
            torch.zeros(1, 2, 4, 4), 3, 3, 1, 1, 1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        _ext.dcn_v2_backward(*args)
    for fn in (_ext.dcn_v2_psroi_pooling_forward, _ext.dcn_v2_psroi_pooling_backward):
        with pytest.raises(RuntimeError):
            fn()


def test_mirror_is_an_autograd_function():
    from centerpose_amd.lib.models.networks.DCNv2 import dcn_v2

    assert issubclass(dcn_v2._DCNv2, torch.autograd.Function)
    assert dcn_v2.dcn_v2_conv == dcn_v2._DCNv2.apply
    d = dcn_v2.DCN(16, 8, 3, 1, 1)
    assert sorted(d.state_dict()) == ["bias", "conv_offset_mask.bias", "conv_offset_mask.weight", "weight"]


def _smooth_case(seed, B=1, C=3, H=5, W=6, Co=2, pad=1):
    """Offsets with fractional parts in [0.2, 0.8]: every sample position is 0.2 away from an integer, where the bilinear
    map and the validity tests are smooth."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g)
    b = torch.randn(Co, generator=g)
    frac = 0.2 + 0.6 * torch.rand(B, 18, H, W, generator=g)
    off = frac + torch.randint(-2, 2, (B, 18, H, W), generator=g).float()
    mask = torch.rand(B, 9, H, W, generator=g)
    go = torch.randn(B, Co, H, W, generator=g)
    return x, w, b, off, mask, go


@needs_ref
def test_harness_matches_central_differences_of_oracle_forward():
    x, w, b, off, mask, go = _smooth_case(0)
    grads = R.backward_ref(x, w, b, off, mask, go, 3, 3, 1, 1, 1, 1, 1, 1, 1)

    def loss(xx, ww, bb, oo, mm):
        return float((odcn.dcn_v2_forward_f64(xx, ww, bb, oo, mm) * go.double()).sum())

    base = [x.double(), w.double(), b.double(), off.double(), mask.double()]
    order = {0: 0, 1: 3, 2: 4, 3: 1, 4: 2}  # harness order (input, offset, mask, weight, bias) -> base index
    rng = np.random.default_rng(1)
    eps = 1e-4
    for gi, bi in order.items():
        t = base[bi]
        for flat in rng.choice(t.numel(), size=min(12, t.numel()), replace=False):
            plus = [u.clone() for u in base]
            minus = [u.clone() for u in base]
            plus[bi].view(-1)[flat] += eps
            minus[bi].view(-1)[flat] -= eps
            fd = (loss(*plus) - loss(*minus)) / (2 * eps)
            got = float(grads[gi].reshape(-1)[flat])
            scale = float(grads[gi].abs().max())
            assert abs(got - fd) <= 1e-4 * scale + 1e-6, (gi, int(flat), got, fd)


@needs_ref
@pytest.mark.parametrize("geo", [
    (3, 3, 1, 1, 1, 1, 1, 1, 1),   # CenterPose
    (3, 3, 2, 2, 1, 1, 1, 1, 2),   # stride 2, two groups
    (5, 5, 1, 1, 2, 2, 1, 1, 1),
    (1, 3, 1, 1, 0, 1, 1, 1, 1),
    (3, 3, 1, 1, 2, 2, 2, 2, 1),   # dilation 2
    (3, 3, 1, 1, 2, 0, 1, 1, 1),   # pad_h != pad_w: the reference's input-gradient quirk
])
def test_harness_agrees_with_float64_restatement(geo):
    kh, kw, sh, sw, ph, pw, dh, dw, dg = geo
    g = torch.Generator().manual_seed(3)
    B, C, H, W, Co = 2, 4, 7, 9, 3
    Ho, Wo = R.out_size(H, W, kh, kw, sh, sw, ph, pw, dh, dw)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, kh, kw, generator=g)
    b = torch.randn(Co, generator=g)
    off = 2 * torch.randn(B, dg * 2 * kh * kw, Ho, Wo, generator=g)
    mask = torch.rand(B, dg * kh * kw, Ho, Wo, generator=g)
    go = torch.randn(B, Co, Ho, Wo, generator=g)
    ref = R.backward_ref(x, w, b, off, mask, go, *geo)
    f64 = R.backward_f64(x, w, b, off, mask, go, *geo)
    for name, a, e in zip(("input", "offset", "mask", "weight", "bias"), ref, f64):
        assert a.shape == e.shape, name
        assert float((a.double() - e).abs().max()) <= 1e-5 * float(e.abs().max()) + 1e-6, name
    if ph != pw:
        fixed = R.backward_f64(x, w, b, off, mask, go, *geo, quirk=False)
        assert float((ref[0].double() - fixed[0]).abs().max()) > 1e-2 * float(fixed[0].abs().max())
