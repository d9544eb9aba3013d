"""Writes tests/golden/conv_select_grid.json: what the convolution kernel selectors answer on the grid of tests/conv_select_cases.py,
at the commit this is run from -- to be run on the PARENT of a change to the selection code that must leave its decisions as they
are (no GPU needed: the selectors are host functions), and replayed after it by tests/test_conv_select_cpu.py.

    make -C centerpose_amd/csrc && python tools/make_conv_select_golden.py --commit $(git rev-parse HEAD)

(--lib: a library built from that commit and kept elsewhere.  The helper is compiled against this tree's cp_common.h, so ConvParams
and the selectors' signatures must be that commit's.)

Before it writes, it checks that the grid is worth pinning: every id the two generic selectors can return is in some row, and at
switch set 0 every *_wanted predicate of igemm16.hip is seen deciding both ways.  What no accepted ConvParams reaches is listed in
the fixture's header (UNREACHED) with the reason, and must indeed be absent."""
import argparse
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from centerpose_amd import hip  # noqa: E402
from tests import conv_select_cases as cs  # noqa: E402

REACHABLE = set(range(0, 22)) | set(range(27, 31)) | set(range(34, 40)) | {41}
# predicate -> (f16x3 ids that show it true, ids that show it false on a launch it was asked about), at switch set 0
WANTED = {
    "dcn16p_wanted": ({30, 38, 39}, {17, 18}),
    "dcn16t_wanted": ({39}, {30, 38}),
    "strm16_wanted": ({41}, {27}),          # (a 32-wide 3x3 that went on to halo16)
    "halo16_wanted": ({27, 28, 29}, {14, 15, 16}),
    "pw16_wanted": ({34, 35}, {14, 15, 16, 19, 20, 21}),
}
UNREACHED = {
    "dcn16s_wanted true at switch set 0 (id 36)": "a launch without whole 128-channel tiles that has dcn16s's 4096 16 x 24 items has more "
    "than dcn16t's 1024 8 x 16 blocks, and dcn16t is asked first; id 36 is reached under CP_SEL_DCN16S_ALWAYS and CP_SEL_DCN16T_NEVER",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit the library was built from (recorded in the fixture)")
    ap.add_argument("--lib", default=hip.LIB_PATH, help="the library to ask")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "conv_select_grid.json"))
    a = ap.parse_args()
    evaluate = cs.helper(a.lib)
    table, groups, n = {}, [], 0
    seen, seen16_sel0 = set(), set()
    for batch in cs.BATCHES:
        for hw in cs.MAPS:
            rows = cs.grid(batch, hw)
            res = evaluate([cs.params(batch, hw, r) for r in rows])
            answers = []
            for r, o in zip(rows, res.tolist()):
                answers.append(table.setdefault(tuple(o), len(table)))
                seen.add(o[0])
                if o[1]:
                    seen.add(o[2])
                    if cs.SELS[r[3]] == 0:
                        seen16_sel0.add(o[2])
            groups.append(dict(B=batch, map=hw, rows=cs.encode(rows, answers)))
            n += len(rows)
    assert len(table) < 64 * 64
    missing = REACHABLE - seen
    assert not missing and seen <= REACHABLE, (sorted(missing), sorted(seen - REACHABLE))
    for name, (yes, no) in sorted(WANTED.items()):
        assert yes & seen16_sel0 and no & seen16_sel0, (name, sorted(seen16_sel0))
    assert 36 not in seen16_sel0 and 36 in seen, "UNREACHED is out of date"
    answers = [list(o) for o, _ in sorted(table.items(), key=lambda kv: kv[1])]
    with open(a.out, "w") as f:
        json.dump(dict(generated_from_commit=a.commit, unreached=UNREACHED, axes=cs.AXES, row_chars=["pair", "config", "weights_tiling",
                       "sel", "answer / 64", "answer % 64"], answer_fields=cs.OUT_FIELDS, answers=answers, groups=groups), f,
                  separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d rows, %d distinct answers, ids %s" % (a.out, n, len(answers), sorted(seen)))


if __name__ == "__main__":
    main()
