"""The pair and triple interaction entries return the bits of the parent commit ba138e2, from
which the one stats / select / list driver was factored (docs/HISTORY.md section 13).

tools/record_interactions.py ran on the parent build and wrote
profiles/interactions_parent_ba138e2.json: per call the stats values (floats as hex), the number
of entries, a SHA-256 of the returned id arrays and values, the scratch held and the launch count.
Here the same cases are rebuilt through the tool's own case builder and every record must be
equal, under every launch budget of the case.  The cases are the smallest that reach each shared
piece: padding and the diagonal tile, two component chunks, ids with holes, a select that goes
past level 0, two reduction levels, two record windows, the restaging path of the triple kernel,
and the pair calls after the triple calls on one handle.

The replay needs a real MI355X; that the recording covers the cases is checked without one."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_interactions as rec  # noqa: E402

PARENT = os.path.join(ROOT, "profiles", "interactions_parent_ba138e2.json")
PARAMS = [(case[0], kind, budget) for case in rec.CASES for kind in case[3] for budget in case[4]]


def _want():
    with open(PARENT) as f:
        return json.load(f)


def test_recording_covers_the_cases():
    want = _want()
    assert want["seed"] == rec.SEED
    assert set(want["cases"]) == {case[0] for case in rec.CASES}
    for name, _, shape, kinds, budgets, calls in rec.CASES:
        got = want["cases"][name]
        assert got["seed"] == rec.case_seed(name) and got["shape"] == list(shape)
        assert set(got["handles"]) == {rec.handle_key(kind) for kind in kinds}
        for records in got["handles"].values():
            assert [(r["call"], r["args"]) for r in records] == list(calls)
            assert all(set(r["launches"]) == {str(b) for b in budgets} for r in records)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,budget", PARAMS,
                         ids=["%s-%s-budget%d" % (n, rec.handle_key(k), b) for n, k, b in PARAMS])
def test_same_bits_as_the_parent(name, kind, budget):
    want = _want()["cases"][name]["handles"][rec.handle_key(kind)]
    case = next(c for c in rec.CASES if c[0] == name)
    got = rec.run_case(case, kind, budget)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        w = dict(w, launches=w["launches"][str(budget)])
        assert g == w, (g, w)
