"""Two exact transforms of a state dict that move the magnitudes of a network's stored activations by powers of two and
leave its arithmetic alone.  No tests in here: tests/test_scale_equivariance_cpu.py pins both on the oracle, bit for bit;
tests/test_scale_equivariance_gpu.py holds the engine to them ("Power-of-two equivariance").

homogeneous(sd, a): every additive constant of the graph (`*.bias`, `*.running_mean`) times a, fed a * x (and a * pre_*).
Conv, BatchNorm in eval mode, ReLU, max-pool, up-sample and add are homogeneous of degree one once their constants are
scaled along, so every tap and raw head is a times the base model's.  The offset / mask convolutions of the deformable layers
get weight / a and their bias unchanged: their maps (and the sampling positions) are those of the base model.  sigmoid, tanh
and GroupNorm are not homogeneous: dlav1_34's ConvGRU taps and heads are out of this transform's scope (in_scope).

gauge(sd, t): at every site where a BatchNorm / bias + ReLU feeds ONE linear consumer, the producer's affine part times f
and the consumer's weight over f (ReLU commutes with f > 0).  The function is unchanged; only the tensor between the two
moves, by f.  f alternates 2^t, 2^-t in state-dict order, so that neighbouring stored tensors differ by 2^(2t).

A power of two commutes with every rounding (away from over- and underflow), so both statements hold bit for bit in any
IEEE arithmetic, whatever the order of its sums."""
import math
import re
from collections import OrderedDict

from tests import layer_parity_ref as R


def is_pow2(v):
    return v > 0 and math.frexp(v)[0] == 0.5


def _scaled(v, f):
    out = v * f
    assert bool((out / f == v).all()), "scaling by %g is not exact here" % f  # (no under- or overflow)
    return out


def homogeneous_keys(sd):
    """-> (keys multiplied by a, keys divided by a)"""
    up = [k for k in sd if "conv_offset_mask" not in k and (k.endswith(".bias") or k.endswith(".running_mean"))]
    down = [k for k in sd if "conv_offset_mask" in k and k.endswith(".weight")]
    return up, down


def homogeneous(sd, a):
    assert is_pow2(a), a
    up, down = (set(ks) for ks in homogeneous_keys(sd))
    return OrderedDict((k, _scaled(v, a) if k in up else _scaled(v, 1.0 / a) if k in down else v.clone()) for k, v in sd.items())


def homogeneous_inputs(x, kw, a):
    # (plain products: pre_hm = rand^8 has entries next to float32's smallest normal number, which 2^-14 takes into the
    # subnormals -- thirty orders of magnitude below the last bit of any sum they enter)
    return x * a, {k: v * a for k, v in kw.items()}


def in_scope(key, name):
    """Is the tap or head `name` ('head:<h>') of the case covered by the homogeneous transform?"""
    if R.CASES[key]["arch"].startswith("dlav1"):
        return not (name.startswith("convGRU.") or name.startswith("head:"))
    return True


def homogeneous_factor(name, a):
    """What the transform multiplies the tap or head by"""
    return 1.0 if name.endswith(".offmask") else a


_HG_HEAD = re.compile(r"^(\w+\.\d+)\.0\.conv\.weight$")
_RES_DCN_BN = re.compile(r"^deconv_layers\.(\d+)\.weight$")


def gauge_sites(sd):
    """The single-consumer sites of a state dict, in its order -> [(site, keys times f, keys over f, tap that moves or None)]"""
    sites = []
    for k in sd:
        if k.endswith(".bn1.weight") and k[:-10] + "conv2.weight" in sd:  # BasicBlock / Bottleneck / hourglass residual
            p = k[:-11]
            sites.append((p, [p + ".bn1.weight", p + ".bn1.bias"], [p + ".conv2.weight"], p + ".conv1"))
        elif k.endswith(".0.weight") and k[:-8] + "2.weight" in sd and k[:-8] + "0.bias" in sd:  # head: 3x3 + ReLU + 1x1
            h = k[:-9]
            sites.append((h, [h + ".0.weight", h + ".0.bias"], [h + ".2.weight"], None))
        elif _HG_HEAD.match(k) and _HG_HEAD.match(k).group(1) + ".1.weight" in sd:  # hourglass head, per stack
            h = _HG_HEAD.match(k).group(1)
            sites.append((h, [h + ".0.conv.weight", h + ".0.conv.bias"], [h + ".1.weight"], None))
        elif _RES_DCN_BN.match(k) and int(_RES_DCN_BN.match(k).group(1)) % 6 == 1:
            # resdcn: DCN -> BN (6i+1) -> ReLU (6i+2) -> ConvTranspose2d (6i+3), nothing else reads the ReLU
            i = int(_RES_DCN_BN.match(k).group(1))
            sites.append(("deconv_layers.%d" % i, ["deconv_layers.%d.weight" % i, "deconv_layers.%d.bias" % i],
                          ["deconv_layers.%d.weight" % (i + 2)], "deconv_layers.%d" % (i + 1)))
        elif k.endswith(".1.weight") and sd[k].dim() == 1 and k[:-8] + "3.weight" in sd and k[:-8] + "0.bias" in sd:
            # dlav1 head: 3x3 -> GroupNorm (h.1) -> ReLU -> 1x1 (h.3); GroupNorm's own affine part is the producer's
            h = k[:-9]
            sites.append((h, [h + ".1.weight", h + ".1.bias"], [h + ".3.weight"], None))
        elif k == "base.base_layer.1.weight":  # DLA: the stem (+ the tracking task's previous-frame stems, added to it) feeds level0 only
            pre = [q[:-7] for q in sd if q.startswith("base.pre_") and q.endswith(".1.weight")]
            ups = [b + leaf for b in ["base.base_layer.1"] + pre for leaf in (".weight", ".bias")]
            sites.append(("base.base_layer", ups, ["base.level0.0.weight"], "base.base_layer"))
        elif k == "base.level0.1.weight":  # DLA: level0 (conv + BN + ReLU) feeds level1's conv only
            sites.append(("base.level0", ["base.level0.1.weight", "base.level0.1.bias"], ["base.level1.0.weight"], "base.level0"))
    return sites


def gauge(sd, t):
    """-> (gauged state dict, {site: f}, {tap that moves: f})"""
    out = OrderedDict((k, v.clone()) for k, v in sd.items())
    factors, moved = OrderedDict(), OrderedDict()
    for n, (site, up, down, tap) in enumerate(gauge_sites(sd)):
        f = 2.0 ** (t if n % 2 == 0 else -t)
        for k in up:
            out[k] = _scaled(sd[k], f)
        for k in down:
            out[k] = _scaled(sd[k], 1.0 / f)
        factors[site] = f
        if tap is not None:
            moved[tap] = f
    return out, factors, moved
