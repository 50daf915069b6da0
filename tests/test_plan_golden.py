"""The two launch planners of the generic kernel, pinned to their recorded outputs (host logic; no
GPU).  tests/golden/batch_queue_plans.json holds, for the case table of tests/_plan_cases.py, what
dpow_batch_plan and dpow_queue_plan returned before the batch's round planner and the queue's
launch planner shared their budget and group functions: per case the launch count or the budget,
the group, the entry count and a digest of the entry list."""
import json
import os

import pytest

import _plan_cases

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "batch_queue_plans.json")


@pytest.fixture(scope="module")
def golden_doc():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one(golden_doc):
    assert [c[:4] for c in golden_doc["cases"]] == list(_plan_cases.table())
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "launch_geometry.json"))


def test_the_table_holds_what_it_should():
    cases = list(_plan_cases.table())
    assert {c[1] for c in cases} == {1, 2, 3, 255, 256, 257, 1024}
    assert {c[3] for c in cases if c[0] == "batch"} == {-1, 0, 1}
    for n in _plan_cases.NS:
        ends = {w[1] - w[0] for e in (-1, 0, 1) for w in _plan_cases.batch_windows(n, "even", e)}
        edge = _plan_cases.round_slice(0, n) + _plan_cases.round_slice(1, n)
        assert ends == {edge - 1, edge, edge + 1}
        w = _plan_cases.batch_windows(n, "long_among_short", 0)
        assert max(b - a for a, b, _ in w) == 1 << 22 and (n == 1 or min(b - a for a, b, _ in w) == 4)
        ages = [_plan_cases.queue_inputs(n, a, "long")[1] for a in _plan_cases.QUEUE_AGES]
        assert [[a] * n for a in range(10)] == ages[:10]
        assert n == 1 or (sorted(set(ages[11])) == [0, 8] and ages[11].count(0) == 1)


def test_every_case(golden_doc):
    for c in golden_doc["cases"]:
        assert _plan_cases.record(c[:4]) == c[4], c[:4]
