"""resnet_dcn.py PoseResNet.forward restated with torch.nn.functional + the oracle's DCNv2 on the CPU (shared: no tests here).

``dtype=torch.float64`` runs every operator in float64 (oracle.dcn dispatches the deformable layers on the input's type).
``taps`` (a dict) receives the intermediate tensors under the engine's tap names: ``maxpool``, ``layerN`` and
``deconv_layers.{2,5,8,11,14,17}`` (the ReLU after each DCN's and each deconvolution's BatchNorm)."""
import torch
import torch.nn.functional as F

from centerpose_amd import synth
from oracle import dcn as odcn


def torch_resdcn_forward(sd, x, depth, heads, dtype=torch.float32, taps=None):
    if dtype == torch.float64:
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        x = x.double()
    elif dtype != torch.float32:
        raise ValueError("torch_resdcn_forward: dtype must be torch.float32 or torch.float64")

    def bn(t, p):
        return F.batch_norm(t, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"],
                            False, 0.0, 1e-5)

    def tap(name, t):
        if taps is not None:
            taps[name] = t
        return t

    bott, blocks = synth.RESNET_SPEC[depth]
    t = torch.relu(bn(F.conv2d(x, sd["conv1.weight"], None, 2, 3), "bn1"))
    t = tap("maxpool", F.max_pool2d(t, 3, 2, 1))
    for li, n in enumerate(blocks):
        for b in range(n):
            p = "layer%d.%d" % (li + 1, b)
            s = 2 if (b == 0 and li) else 1
            res = t
            if p + ".downsample.0.weight" in sd:
                res = bn(F.conv2d(t, sd[p + ".downsample.0.weight"], None, s), p + ".downsample.1")
            if bott:
                u = torch.relu(bn(F.conv2d(t, sd[p + ".conv1.weight"]), p + ".bn1"))
                u = torch.relu(bn(F.conv2d(u, sd[p + ".conv2.weight"], None, s, 1), p + ".bn2"))
                u = bn(F.conv2d(u, sd[p + ".conv3.weight"]), p + ".bn3")
            else:
                u = torch.relu(bn(F.conv2d(t, sd[p + ".conv1.weight"], None, s, 1), p + ".bn1"))
                u = bn(F.conv2d(u, sd[p + ".conv2.weight"], None, 1, 1), p + ".bn2")
            t = torch.relu(u + res)
        tap("layer%d" % (li + 1), t)
    for i in range(3):
        fc = "deconv_layers.%d" % (6 * i)
        om = F.conv2d(t, sd[fc + ".conv_offset_mask.weight"], sd[fc + ".conv_offset_mask.bias"], 1, 1)
        o1, o2, m = torch.chunk(om, 3, dim=1)  # dcn_v2.py DCN.forward
        t = odcn.dcn_v2_forward(t, sd[fc + ".weight"], sd[fc + ".bias"], torch.cat((o1, o2), 1).contiguous(),
                                torch.sigmoid(m).contiguous(), 3, 3, 1, 1, 1, 1, 1, 1, 1)
        t = tap("deconv_layers.%d" % (6 * i + 2), torch.relu(bn(t, "deconv_layers.%d" % (6 * i + 1))))
        t = F.conv_transpose2d(t, sd["deconv_layers.%d.weight" % (6 * i + 3)], None, 2, 1)
        t = tap("deconv_layers.%d" % (6 * i + 5), torch.relu(bn(t, "deconv_layers.%d" % (6 * i + 4))))
    return {h: F.conv2d(torch.relu(F.conv2d(t, sd[h + ".0.weight"], sd[h + ".0.bias"], 1, 1)), sd[h + ".2.weight"],
                        sd[h + ".2.bias"]) for h in heads}
