"""The convolution kernel selectors (cp_conv_variant, cp_conv16_supported, cp_conv16_variant, cp_conv16_project_supported,
cp_conv_geometry: pure host functions of a ConvParams) replayed on the grid of tests/golden/conv_select_grid.json, which
tools/make_conv_select_golden.py recorded from the commit named in the fixture: every row must get the recorded answer.  The profile
tables, tests/golden/engine_plan_pins.json and the engine's fusion decisions all rest on these answers; the GPU pins cover the
launches of 22 model passes, this covers both sides of every threshold the selectors read."""
import json
import os

import pytest

import __graft_entry__ as ge
from centerpose_amd import hip
from tests import conv_select_cases as cs

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(os.path.join(REPO, "tests", "golden", "conv_select_grid.json")))
    assert g["axes"] == cs.AXES and g["answer_fields"] == cs.OUT_FIELDS, "the fixture was recorded over other axes: regenerate it"
    return g


@pytest.fixture(scope="module")
def evaluate():
    ge.build()
    return cs.helper(hip.LIB_PATH)


def test_every_row_of_the_grid_selects_what_the_recorded_commit_selected(golden, evaluate):
    bad, n = [], 0
    for group in golden["groups"]:
        batch, hw = group["B"], group["map"]
        rows, answers = cs.decode(group["rows"])
        res = evaluate([cs.params(batch, hw, r) for r in rows]).tolist()
        n += len(rows)
        for r, a, got in zip(rows, answers, res):
            if got != golden["answers"][a]:
                bad.append("%s\n    recorded %s\n    now      %s" % (cs.describe(batch, hw, r), dict(zip(cs.OUT_FIELDS, golden["answers"][a])),
                                                                    dict(zip(cs.OUT_FIELDS, got))))
    assert n > 10000
    assert not bad, "%d of %d rows differ from commit %s:\n%s" % (len(bad), n, golden["generated_from_commit"], "\n".join(bad[:20]))


def test_the_fixture_holds_the_whole_grid(golden):
    """the rows recorded are the ones the grid builder makes now (a row dropped from the fixture would go unnoticed otherwise)"""
    assert [(g["B"], g["map"]) for g in golden["groups"]] == [(b, m) for b in cs.BATCHES for m in cs.MAPS]
    for group in golden["groups"]:
        assert cs.decode(group["rows"])[0] == cs.grid(group["B"], group["map"])
