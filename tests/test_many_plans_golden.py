"""The launch plans of the batched census and the batched scan, pinned to tests/golden/many_plans.json
(tests/golden/gen_golden.py --many-plans): what the library returned before the three batched host
loops were put on one planner.  Per plan the launch count, the entry count and the SHA-256 of the
dpow_batch_range rows are recomputed with the library in the tree and compared; so are
dpow_scan_plan_halve's budgets.  CPU only."""
import json
import os

import pytest

import distpow
from _many_plan_cases import census_windows, digest, expand, scan_windows

with open(os.path.join(os.path.dirname(__file__), "golden", "many_plans.json")) as f:
    GOLDEN = json.load(f)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_plans_are_the_recorded_ones(case):
    tasks = expand(case["tasks"])
    assert len(tasks) == case["n_tasks"]
    for p in case["plans"]:
        if p["plan"] == "census":
            blocks, launches = distpow.census_plan(census_windows(tasks), p["cap"])
        else:
            blocks, launches = distpow.scan_plan(scan_windows(tasks), p["cap"], p["capacity"])
        got = {"launches": launches, "entries": len(blocks), "sha256": digest(blocks)}
        assert got == {k: p[k] for k in got}, (case["name"], p["plan"], p["cap"], p["capacity"])


def test_halved_budgets_are_the_recorded_ones():
    pairs = [(h["total"], h["weight"]) for h in GOLDEN["halve"]]
    assert len(pairs) >= 12 and (256, 256) in pairs and (1 << 28, 16384) in pairs
    for h in GOLDEN["halve"]:
        assert distpow.scan_plan_halve(h["total"], h["weight"]) == (h["cap"], h["capacity"]), h


def test_the_fixture_holds_the_cases_it_must():
    """One task, 4096 tasks of 256 indices, empty tasks, a task cut by two seams, every cap, capacity,
    partition width and depth the plans are pinned at."""
    by_name = {c["name"]: c for c in GOLDEN["cases"]}
    assert by_name["one task"]["n_tasks"] == 1
    t = expand(by_name["4096 tasks of 256 indices"]["tasks"])
    assert len(t) == 4096 and all((k1 - k0) << (8 - w % 9) == 256 for k0, k1, w, _ in t)
    t = expand(by_name["empty tasks at the front, in the middle and at the end"]["tasks"])
    empty = [k0 == k1 for k0, k1, _, _ in t]
    assert empty[0] and empty[-1] and not all(empty) and any(empty[j] for j in range(1, len(t) - 1) if not empty[j - 1])
    # the second task of three begins in the first launch and ends in the third
    c = by_name["a task cut by two seams"]
    blocks, launches = distpow.census_plan(census_windows(expand(c["tasks"])), 4096)
    assert launches == 3 and {b.launch for b in blocks if b.task == 1} == {0, 1, 2}
    plans = [p for c in GOLDEN["cases"] for p in c["plans"]]
    assert {256, 4096, 1 << 28} <= {p["cap"] for p in plans}
    assert {1024, 65536} <= {p["capacity"] for p in plans if p["plan"] == "scan"}
    mixed = expand(by_name["mixed widths and depths"]["tasks"])
    assert {w for _, _, w, _ in mixed} == {0, 3, 8} and {z for _, _, _, z in mixed} == {0, 1, 6, 7, 9}
