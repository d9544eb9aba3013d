"""The engine's host-side decisions against tests/golden/engine_plan_pins.json (tools/make_engine_plan_pins.py, recorded at the
commit named inside): per case of tests/engine_plan_cases.py the ordered launch rows, the per-variant launch / FLOP / byte totals,
the work-space query's answer, the peak of a real pass, the stand-alone maxpool2 launches and a SHA-256 of every returned tensor
are equal to the recorded ones, field by field.  A change to how Fwd plans a convolution that moves any launch, any charge, any
allocation or any bit shows here."""
import json
import os

import pytest

from tests import engine_plan_cases as pc

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_plan_pins.json")) as _f:
    PINS = json.load(_f)
BY_ID = {p["id"]: p for p in PINS["cases"]}


def test_fixture_covers_the_cases():
    assert len(PINS["generated_from_commit"]) == 40
    assert sorted(BY_ID) == sorted(pc.case_id(c) for c in pc.CASES)
    # the dla_34 cases are bit-stable (the epilogue tests assert 20-pass bit equality there): they all keep their digests
    assert all(p["digests"] for i, p in BY_ID.items() if i.startswith("dla_34-"))


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_engine_plan_pin(device, case):
    want = BY_ID[pc.case_id(case)]
    got = json.loads(json.dumps(pc.record(case, device)))
    assert len(got["launch_rows"]) == len(want["launch_rows"])
    for i, (g, w) in enumerate(zip(got["launch_rows"], want["launch_rows"])):
        assert g == w, ("launch %d" % i, g, w)
    assert got["variants"] == want["variants"]
    for k in ("workspace_bytes", "workspace_used", "maxpool_launches"):
        assert got[k] == want[k], (k, got[k], want[k])
    if want["digests"] is not None:
        assert sorted(got["digests"]) == sorted(want["digests"])
        for k in want["digests"]:
            assert got["digests"][k] == want["digests"][k], k
