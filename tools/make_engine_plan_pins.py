"""Writes tests/golden/engine_plan_pins.json: what the engine's host code decides, per case of tests/engine_plan_cases.py, at the
commit this is run from -- to be run on an MI355X BEFORE a change to the engine's host code that must leave its decisions as they
are, and replayed after it by tests/test_engine_plan_pins_gpu.py.

    python tools/make_engine_plan_pins.py --commit $(git rev-parse HEAD) [--out tests/golden/engine_plan_pins.json]

Uses the Python binding only: HipModel.forward / detect, profile / profile_read, the CP_PROFILE_DUMP per-launch CSV,
workspace_bytes / workspace_used / maxpool_launches, select_kernels.  Every case runs three times without profiling; a case whose
digests differ between the runs is printed, keeps its launch rows and loses its digests."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from tests import engine_plan_cases as pc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit the library was built from (recorded in the fixture)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "engine_plan_pins.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pins = []
    for case in pc.CASES:
        pin = pc.record(case, dev, passes=3)
        if "unstable" in pin:
            print("digests differ between runs, dropped: %s %s" % (pin["id"], pin.pop("unstable")), flush=True)
            pin["digests"] = None
        print("%-72s %3d launches, work space %d of %d, maxpool2 %d" % (pin["id"], len(pin["launch_rows"]), pin["workspace_used"],
                                                                         pin["workspace_bytes"], pin["maxpool_launches"]), flush=True)
        pins.append(pin)
    with open(a.out, "w") as f:
        json.dump(dict(generated_from_commit=a.commit, row_fields=["variant", "M", "N", "K", "kh", "stride", "role"], cases=pins), f,
                  separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d cases)" % (a.out, len(pins)))


if __name__ == "__main__":
    main()
