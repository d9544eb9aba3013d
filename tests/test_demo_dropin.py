"""INTEGRATION level 0, executed: a demo-style caller (tests/demo_dropin_script.py) drives this repo's package as a drop-in
``lib`` -- `lib.opts`, `lib.detectors.detector_factory`, `Detector(opt).run(image_path, meta_inp=meta)` on an image file
and the nine timing keys of its result.  The device stages are replaced by the oracle there (no GPU), everything else is
the product's host code."""
import os
import subprocess
import sys

import numpy as np
import torch

from centerpose_amd import synth


def test_detector_run_on_an_image_file_through_the_mirror(tmp_path):
    from PIL import Image

    # an 800x600 RGB frame (the size of the Objectron demo images), seeded
    img = os.path.join(str(tmp_path), "frame.png")
    Image.fromarray(np.random.default_rng(3).integers(0, 256, (800, 600, 3), dtype=np.uint8)).save(img)
    ck = os.path.join(str(tmp_path), "dla34_synth.pth")
    torch.save({"epoch": 1, "state_dict": synth.make_state_dict("dla_34", synth.HEADS_POSE)}, ck)
    script = os.path.join(os.path.dirname(__file__), "demo_dropin_script.py")
    r = subprocess.run([sys.executable, script, img, ck], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DEMO_DROPIN_OK" in r.stdout
    line = [l for l in r.stdout.splitlines() if l.startswith("Frame 0|")]
    assert line, r.stdout[-2000:]
    for key in ("tot", "load", "pre", "net", "dec", "post", "merge", "pnp", "track"):
        assert key + " " in line[0]
