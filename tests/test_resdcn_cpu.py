"""resdcn_N (resnet_dcn.py PoseResNet with DCN up-sampling): parameter tables, the model factory and its refusals,
and the synthetic weights' activation bounds on the reference module.  No GPU needed."""
import json
import os
import types

import pytest
import torch

from centerpose_amd import synth
from centerpose_amd.lib.models import model as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEPTHS = (18, 34, 50, 101, 152)


def _keys():
    with open(os.path.join(GOLD, "state_dict_keys_resdcn.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("depth", DEPTHS)
def test_param_spec_matches_reference_keys(depth):
    ref = _keys()["resdcn_%d" % depth]
    spec = synth.param_spec("resdcn_%d" % depth, synth.HEADS_POSE, head_conv=64)
    assert [[k, list(v)] for k, v in spec.items()] == ref


def test_key_counts():
    k = _keys()
    assert (len(k["resdcn_18"]), len(k["resdcn_101"]), len(k["resdcn_152"])) == (193, 697, 1003)


def test_create_model_resdcn_18_has_reference_keys():
    m = M.create_model("resdcn_18", synth.HEADS_POSE, 64)
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == _keys()["resdcn_18"]
    assert float(sd["hm.2.bias"][0]) == pytest.approx(-2.19)
    assert float(sd["hm_hp.2.bias"][0]) == pytest.approx(-2.19)
    assert float(sd["wh.2.bias"].abs().max()) == 0.0


def test_refusals():
    with pytest.raises(NotImplementedError):
        M.create_model("resdcn_18", synth.HEADS_POSE, 64, types.SimpleNamespace(tracking_task=True))
    with pytest.raises(NotImplementedError):
        M.create_model("resdcn_18", synth.HEADS_POSE, 0)
    with pytest.raises(NotImplementedError):
        M.create_model("resdcn_20", synth.HEADS_POSE, 64)
    with pytest.raises(NotImplementedError):
        M.create_model("res_18", synth.HEADS_POSE, 64)


def test_engine_refuses_tracking_and_bad_head_conv():
    import ctypes

    from centerpose_amd import hip

    L = hip.lib()
    h = ctypes.c_void_p()
    names = (ctypes.c_char_p * 1)(b"hm")
    classes = (ctypes.c_int * 1)(1)
    assert L.cp_model_create(b"resdcn_18", 1, 1, names, classes, 64, ctypes.byref(h)) == -1
    assert b"single frame" in L.cp_last_error()
    assert L.cp_model_create(b"resdcn_18", 0, 1, names, classes, 0, ctypes.byref(h)) == -1
    assert L.cp_model_create(b"resdcn_19", 0, 1, names, classes, 64, ctypes.byref(h)) == -1
    assert b"arch" in L.cp_last_error()
    assert L.cp_model_create(b"resdcn_101", 0, 1, names, classes, 64, ctypes.byref(h)) == 0
    L.cp_model_destroy(h)


def test_resdcn_weights_checksum_and_existing_arch_weights_unchanged():
    """make_state_dict's resdcn branch reproduces the weights the resdcn goldens were made from, and leaves the seeded
    DLA / hourglass weights (whose goldens carry a checksum) exactly as they were."""
    import numpy as np

    gold = np.load(os.path.join(GOLD, "backbone_resdcn_18.npz"))
    sd = synth.make_state_dict("resdcn_18", synth.HEADS_POSE)
    assert synth.abs_checksum(sd) == float(gold["_weights_checksum"])
    for arch, tracking, name in (("dla_34", False, "dla"), ("dla_34", True, "dla_track"), ("dlav1_34", False, "dlav1"),
                                 ("dlav1_34", True, "dlav1_track"), ("hourglass", False, "hourglass")):
        heads = synth.HEADS_TRACK if tracking else synth.HEADS_POSE
        g = np.load(os.path.join(GOLD, "backbone_%s.npz" % name))
        sd = synth.make_state_dict(arch, heads, tracking)
        chk = float(sum(v.double().sum() for v in sd.values() if v.is_floating_point()))
        assert abs(chk - float(g["_weights_checksum"][0])) < 1e-6 * max(1.0, abs(chk)), name
    assert synth.make_state_dict("dla_34", synth.HEADS_POSE)["hm.0.weight"].shape[0] == 256  # DLA default head_conv


def _reference_available():
    from oracle.tools import ref_harness

    return ref_harness.available() and os.path.exists(os.path.join(os.path.dirname(GOLD), "..", "oracle", "libcp_oracle.so"))


@pytest.mark.parametrize("depth", DEPTHS)
def test_synthetic_activations_bounded_on_reference(depth):
    """On the reference module at 128 x 128, the damped residual branches keep every stage O(1) (152 included), DCN
    offsets are pixels, not zero, and heat-map logits spread around -2.19."""
    if not _reference_available():
        pytest.skip("reference tree not present")
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(GOLD), "..", "tools"))
    import make_resdcn_goldens as mk

    m = mk.reference_model(depth, synth.HEADS_POSE)
    m.load_state_dict(synth.make_state_dict("resdcn_%d" % depth, synth.HEADS_POSE), strict=True)
    stats = {}
    hooks = [m.get_submodule(n).register_forward_hook(lambda mod, i, o, n=n: stats.__setitem__(n, o.detach()))
             for n in ("layer1", "layer2", "layer3", "layer4", "deconv_layers.0.conv_offset_mask", "deconv_layers.17")]
    with torch.no_grad():
        out = m(synth.frames(1, seed=3, h=128, w=128))[0]
    for h in hooks:
        h.remove()
    for n in ("layer1", "layer2", "layer3", "layer4", "deconv_layers.17"):
        rms = float(stats[n].pow(2).mean().sqrt())
        assert 0.05 < rms < 20.0, (n, rms)
    off = stats["deconv_layers.0.conv_offset_mask"][:, :18]
    assert 0.2 < float(off.abs().mean()) < 10.0
    hm = out["hm"]
    assert -4.0 < float(hm.mean()) < -0.5 and float(hm.std()) > 0.05
