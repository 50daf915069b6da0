"""The cases of tests/golden/many_plans.json: how a case's compact task description becomes task
tuples, and how a plan is digested.  Shared by tests/golden/gen_golden.py --many-plans, which
recorded the fixture, and tests/test_many_plans_golden.py, which recomputes it.

A task is (k_begin, k_end, worker_bits, ntz).  dpow_census_plan takes its first three fields;
dpow_scan_plan takes its local index range, k << (8 - worker_bits % 9), and its ntz."""
import hashlib
import random


def expand(spec):
    """The tasks of a case's "tasks" entry: {"list": [[k0, k1, wbits, ntz], ...]}, {"repeat": [k0, k1,
    wbits, ntz], "n": n}, or a seeded draw {"seed", "n", "worker_bits", "ntz", "k_starts", "max_k",
    "empty"}: per task a partition width, a depth and a start from the lists, and a length below
    max_k, 0 for one task in `empty`."""
    if "list" in spec:
        return [tuple(t) for t in spec["list"]]
    if "repeat" in spec:
        return [tuple(spec["repeat"])] * spec["n"]
    rnd = random.Random(spec["seed"])
    tasks = []
    for _ in range(spec["n"]):
        wbits, ntz, k0 = rnd.choice(spec["worker_bits"]), rnd.choice(spec["ntz"]), rnd.choice(spec["k_starts"])
        size = 0 if rnd.randrange(spec["empty"]) == 0 else 1 + rnd.randrange(spec["max_k"])
        tasks.append((k0, k0 + size, wbits, ntz))
    return tasks


def census_windows(tasks):
    return [(k0, k1, wbits) for k0, k1, wbits, _ in tasks]


def scan_windows(tasks):
    return [(k0 << (8 - wbits % 9), k1 << (8 - wbits % 9), ntz) for k0, k1, wbits, ntz in tasks]


def digest(blocks):
    """SHA-256 of the dpow_batch_range rows as the library returned them."""
    return hashlib.sha256(bytes(blocks)).hexdigest()
