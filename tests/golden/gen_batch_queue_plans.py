"""Records tests/golden/batch_queue_plans.json: what dpow_batch_plan and dpow_queue_plan return for
the case table of tests/_plan_cases.py, with the library built from this tree.  Regenerate only
when the planners' policy changes on purpose:
    python tests/golden/gen_batch_queue_plans.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "distributed-proof-of-work_amd"), os.path.join(ROOT, "tests")]

import _plan_cases  # noqa: E402

if __name__ == "__main__":
    rows = [json.dumps(c + [_plan_cases.record(c)], separators=(",", ":")) for c in _plan_cases.table()]
    path = os.path.join(HERE, "batch_queue_plans.json")
    with open(path, "w") as out:  # one case per line
        out.write('{"cases":[\n%s\n]}\n' % ",\n".join(rows))
    print(len(rows), "cases,", os.path.getsize(path), "bytes")
