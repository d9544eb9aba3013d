"""Writes tests/golden/pose_loss_ref.npz: the reference's own ObjectPoseLoss on the seeded cases of tests/pose_loss_cases.py.

Runs only where the reference project exists ($CENTERPOSE_REFERENCE, as the other make_*_goldens.py): it imports the
reference's `src/lib/trains/object_pose.py` unmodified, with the modules it imports but the loss does not use (cv2,
numba, progress.bar, lib.utils.debugger, lib.utils.oracle_utils) stubbed, and runs ObjectPoseLoss on the CPU in float32
with autograd.  The head outputs are non-leaf tensors (leaf * 1), as a model's are, so that `_sigmoid`'s in-place
`sigmoid_` accepts them.  Only outputs are stored; the inputs are regenerated from the case seeds.

  python tools/make_pose_loss_goldens.py      # rewrites the .npz bit for bit

Contents, per case <c>:
  <c>/loss []  <c>/stats [10] (tests/pose_loss_ref.py STATS order)  <c>/choice [B] int64
  <c>/term_<t> [B,S]   each term's per-variant matrix, summed over the stacks (the reference's hm_loss, ... before the
                       selection), for the terms that count
  <c>/grad<s>_<h>      dL/d(head h of stack s) for every head that receives a gradient
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "pose_loss_ref.npz")

from tests import pose_loss_cases as PC  # noqa: E402
from tests import pose_loss_ref as R  # noqa: E402


def run_reference(Ref, name):
    """The reference's loss on case `name`, with the [B,S] term matrices captured from its criterion calls."""
    opt, phase, outputs, batch = PC.case(name)
    leaves = [{k: torch.from_numpy(v).requires_grad_() for k, v in o.items()} for o in outputs]
    outs = [{k: v * 1 for k, v in o.items()} for o in leaves]
    bt = {k: torch.from_numpy(v) for k, v in batch.items()}
    crit = Ref(opt)
    rec = []
    for attr in ("crit", "crit_hm_hp", "crit_kp", "crit_kp_uncertainty", "crit_reg", "crit_reg_uncertainty"):
        m = getattr(crit, attr)
        m.register_forward_hook(lambda mod, args, out, attr=attr: rec.append((attr, out.detach().clone())))
    loss, stats, choice = crit(outs, bt, phase)
    loss.backward()
    return opt, phase, outputs, batch, loss, stats, choice, rec, leaves


def term_matrices(opt, phase, rec):
    """Maps the recorded criterion outputs, in call order, back to the terms (the order of object_pose.py:76-160)."""
    on = R.on_terms(opt)
    order = ["hm", "hp"] + [t for t in ("wh", "obj_scale", "off", "hp_offset", "hm_hp", "tracking", "tracking_hp")
                            if t in on]
    assert len(rec) == len(order) * opt.num_stacks, (len(rec), order)
    acc = {}
    for i, (_, v) in enumerate(rec):
        t = order[i % len(order)]
        acc[t] = acc.get(t, 0) + v / opt.num_stacks
    return acc


def main():
    Ref = PC.import_reference_loss()
    if Ref is None:
        raise SystemExit("reference not found under %s (set CENTERPOSE_REFERENCE)" % PC.REF)
    torch.set_num_threads(1)
    out = {}
    for name in PC.CASES:
        opt, phase, outputs, batch, loss, stats, choice, rec, leaves = run_reference(Ref, name)
        out["%s/loss" % name] = np.float32(loss.item())
        out["%s/stats" % name] = np.array([float(stats[k]) for k in R.STATS], np.float32)
        out["%s/choice" % name] = choice.numpy().astype(np.int64)
        for t, v in term_matrices(opt, phase, rec).items():
            out["%s/term_%s" % (name, t)] = v.numpy().astype(np.float32)
        for s, o in enumerate(leaves):
            for h, v in o.items():
                if v.grad is not None:
                    out["%s/grad%d_%s" % (name, s, h)] = v.grad.numpy()
    # zip entries with a fixed timestamp: a rerun rewrites the file bit for bit
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.save(buf, np.asarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
