"""Writes tests/golden/hourglass_train_ref.npz: one training step of the reference's own hourglass module, in float64, on the
case of tests/hourglass_net_ref.py.

    python tools/make_hourglass_train_golden.py /path/to/CenterPose/src/lib

The argument is the reference's ``src/lib`` directory; ``models/networks/large_hourglass.py`` is imported from it at run time
and nothing of it is copied.  The module is ``exkp(2, 2, [256, 256, 384], [1, 1, 1], heads)`` with ``make_hg_layer`` as
``HourglassNet`` passes it (large_hourglass.py:290-309), loaded with ``hourglass_net_ref.case_state_dict()``, in training mode;
the loss is ``hourglass_net_ref.case_inputs()``'s linear functional of the 14 head maps.  The file holds

* ``keys`` / ``shapes``: the module's state-dict keys in order, and their shapes (``;``-joined text),
* ``z.K.<head>``: both stacks' head outputs,
* ``g.sum`` / ``g.abs`` / ``g.sample.<i>``: per parameter (in ``named_parameters`` order) the gradient's sum, absolute sum and
  ``hourglass_net_ref.grad_sample`` of it,
* ``b.<key>``: the updated running statistics and step counts of ``hourglass_net_ref.GOLDEN_BNS``.

tests/test_pose_net_hourglass_cpu.py pins tests/hourglass_net_ref.py in float64 to this file at 1e-9 relative.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
PATH = os.path.join(REPO, "tests", "golden", "hourglass_train_ref.npz")


def main(lib_dir):
    from tests import hourglass_net_ref as R

    spec = importlib.util.spec_from_file_location(
        "large_hourglass", os.path.join(lib_dir, "models", "networks", "large_hourglass.py"))
    lh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lh)
    c = R.CASE
    net = lh.exkp(c["n"], c["num_stacks"], c["dims"], c["modules"], R.HEADS, make_hg_layer=lh.make_hg_layer).double()
    net.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in R.case_state_dict().items()}, strict=True)
    net.train()
    x, lin = R.case_inputs()
    zs = net(x.double())
    loss = sum((z[h] * lin[k][h].double()).sum() for k, z in enumerate(zs) for h in R.HEADS)
    loss.backward()
    sd = net.state_dict()
    out = {"keys": np.array(list(sd)), "shapes": np.array([";".join(str(d) for d in v.shape) for v in sd.values()])}
    for k, z in enumerate(zs):
        for h in R.HEADS:
            out["z.%d.%s" % (k, h)] = z[h].detach().numpy()
    params = list(net.named_parameters())
    out["g.names"] = np.array([k for k, _ in params])
    out["g.sum"] = np.array([float(p.grad.sum()) for _, p in params])
    out["g.abs"] = np.array([float(p.grad.abs().sum()) for _, p in params])
    for i, (_, p) in enumerate(params):
        out["g.sample.%d" % i] = R.grad_sample(p.grad).numpy()
    for bn in R.GOLDEN_BNS:
        for leaf in ("running_mean", "running_var", "num_batches_tracked"):
            out["b.%s.%s" % (bn, leaf)] = sd["%s.%s" % (bn, leaf)].numpy()
    np.savez_compressed(PATH, **out)
    print("wrote %s: %d bytes, %d parameters" % (os.path.relpath(PATH, REPO), os.path.getsize(PATH), len(params)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
