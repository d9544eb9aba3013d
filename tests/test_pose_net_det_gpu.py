"""Whole-network training steps under ``hip.set_deterministic(True)`` (pytest -m gpu), on the set-ups of
tests/test_pose_net_gpu.py (PoseNet, dla_34) and tests/test_pose_net_gru_gpu.py (PoseNetGRU, dlav1_34): B = 2, 3 x 64 x 96,
head_conv 64, precision f32.

What now holds: with the deterministic DCNv2 input gradient (cp_dcnv2_backward_det) two training steps from the same state
give bit-identical outputs and bit-identical gradients for EVERY parameter that has one -- ``base``, ``dla_up`` and ``ida_up``
included, which tests/test_pose_net_gpu.py::test_eval_mode_and_repeatability could only compare with the reference because
they sit behind the float atomics of the default call.  No key is excused.  The same step stays within that file's 1e-3 bound
of the float64 reference."""
import pytest
import torch

from centerpose_amd import hip
from tests import pose_net_ref as R
from tests import test_pose_net_gpu as TP
from tests import test_pose_net_gru_gpu as TG

pytestmark = pytest.mark.gpu


@pytest.fixture
def deterministic():
    prev = hip.set_deterministic(True)
    yield
    hip.set_deterministic(prev)


def _assert_steps_identical(step):
    a, za = step()
    b, zb = step()
    for h in za:
        assert torch.equal(za[h], zb[h]), "first output that differs: %s" % h
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert list(pa) == list(pb)
    with_grad = [k for k in pa if pa[k].grad is not None]
    assert any(k.startswith("base.") for k in with_grad) and any(".conv_offset_mask." in k for k in with_grad)
    differing = [k for k in with_grad if pb[k].grad is None or not torch.equal(pa[k].grad, pb[k].grad)]
    assert not differing, "first gradient that differs: %s (%d of %d keys differ)" % (differing[0], len(differing),
                                                                                    len(with_grad))
    return a, za


def test_pose_net_step_is_bit_identical(device, deterministic):
    net, z = _assert_steps_identical(lambda: TP._step(device, False)[:2])
    # the same step against the float64 reference, per family, with test_pose_net_gpu.py's bound
    _, _, r64 = R.reference_case(False)
    failures, fam = [], {}
    for h, ref in r64.z.items():
        e = float((z[h].double() - ref).abs().max()) / float(ref.abs().max())
        fam["outputs"] = max(fam.get("outputs", 0.0), e)
        if e > TP.LIMIT:
            failures.append((h, e))
    params = dict(net.named_parameters())
    for k, g in r64.grads.items():
        if g is None:
            assert params[k].grad is None, k
            continue
        s = float(r64.grads[R.companion_weight(k)].abs().max()) if R.is_pre_bn_bias(k) else float(g.abs().max())
        e = float((params[k].grad.cpu().double() - g).abs().max()) / s
        name = "zero-gradient biases" if R.is_pre_bn_bias(k) else R.family(k, g.dim())
        fam[name] = max(fam.get(name, 0.0), e)
        if e > TP.LIMIT:
            failures.append((k, e))
    for name, e in fam.items():
        print("pose_net deterministic %-22s device %.2e (of max |float64|)" % (name, e))
    assert not failures, failures[:10]


def test_pose_net_gru_step_is_bit_identical(device, deterministic):
    """tests/pose_net_gru_ref.py's case: GroupNorm, the ConvGRU gate and the same IDAUp DCNs."""
    _assert_steps_identical(lambda: TG._step(device, False)[:2])
