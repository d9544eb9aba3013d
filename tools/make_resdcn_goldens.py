"""Write the resdcn goldens under tests/golden/ from the reference's own PoseResNet (resnet_dcn.py), on CPU.

    python tools/make_resdcn_goldens.py

* state_dict_keys_resdcn.json: the reference's state_dict key -> shape table for resdcn_18/34/50/101/152.
* backbone_resdcn_18.npz, backbone_resdcn_101.npz: heads at a 128 x 128 input (B = 1), a few taps, and
  _weights_checksum of the synthetic weights (synth.make_state_dict, seed 317, head_conv 64).

The model is built as PoseResNet(block, layers, heads, head_conv) directly: get_pose_net / init_weights would fetch
ImageNet weights.  oracle.tools.ref_harness.setup() installs the DCNv2 extension shim (it needs oracle/libcp_oracle.so
from build()).  The goldens come from a float64 forward -- the module in double precision, the DCN through the oracle's
float64 restatement (dcn_v2_forward_f64) -- rounded to float32 once at the end, so they do not depend on which CPU
kernels torch picks on the machine that runs the tool.  Needs the reference tree; a rerun reproduces the files bit
for bit.
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from centerpose_amd import synth  # noqa: E402
from oracle.tools import ref_harness  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
DEPTHS = (18, 34, 50, 101, 152)
TAPS = ("layer4", "deconv_layers.2", "deconv_layers.5", "deconv_layers.17")


def reference_model(depth, heads, head_conv=64):
    ref_harness.setup()
    from lib.models.networks import resnet_dcn

    block, layers = resnet_dcn.resnet_spec[depth]
    model = resnet_dcn.PoseResNet(block, layers, dict(heads), head_conv)  # no init_weights: no download
    model.eval()
    return model


def use_f64_dcn():
    """Route the shim's DCNv2 forward to the float64 restatement (3x3, stride 1, pad 1, dilation 1, one group: every
    DCN of resnet_dcn.py)."""
    import sys as _sys

    from oracle import dcn as odcn

    ref_harness.setup()

    def dcn_v2_forward(input, weight, bias, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, dg):
        assert (kh, kw, sh, sw, ph, pw, dh, dw, dg) == (3, 3, 1, 1, 1, 1, 1, 1, 1)
        return odcn.dcn_v2_forward_f64(input, weight, bias, offset, mask, pad=1)

    _sys.modules["_ext"].dcn_v2_forward = dcn_v2_forward


def weights_checksum(sd):
    return synth.abs_checksum(sd)


def forward_with_taps(model, x):
    taps = {}
    hooks = [model.get_submodule(n).register_forward_hook(lambda m, i, o, n=n: taps.__setitem__(n, o.detach().clone()))
             for n in TAPS]
    with torch.no_grad():
        out = model(x)[0]
    for h in hooks:
        h.remove()
    return out, taps


def main():
    torch.set_num_threads(8)
    heads = synth.HEADS_POSE
    use_f64_dcn()
    keys = {}
    for d in DEPTHS:
        m = reference_model(d, heads)
        keys["resdcn_%d" % d] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(GOLDEN, "state_dict_keys_resdcn.json"), "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
    for d in (18, 101):
        arch = "resdcn_%d" % d
        m = reference_model(d, heads)
        sd = synth.make_state_dict(arch, heads)
        m.load_state_dict(sd, strict=True)
        m.double()
        x = synth.frames(1, seed=7, h=128, w=128)
        out, taps = forward_with_taps(m, x.double())
        out = {k: v.float() for k, v in out.items()}
        taps = {k: v.float() for k, v in taps.items()}
        arrs = {"x": x.numpy(), "_weights_checksum": np.float64(weights_checksum(sd))}
        for k, v in out.items():
            arrs["head_" + k] = v.numpy()
        for k, v in taps.items():
            arrs["tap_" + k] = v.numpy()
        np.savez(os.path.join(GOLDEN, "backbone_%s.npz" % arch), **arrs)
        print(arch, {k: float(np.abs(v).max()) for k, v in arrs.items() if k.startswith("head_")})


if __name__ == "__main__":
    main()
