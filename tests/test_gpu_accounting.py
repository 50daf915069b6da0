"""What the batched search and the task queue count is what their planners planned: launches,
rounds and candidates of tasks that cannot hit (N = 32) against dpow_batch_plan and a replay of
dpow_queue_plan for the same windows.  Under 2^25 candidates in all."""
import pytest

import distpow
from distpow import EXHAUSTED, BatchTask, TaskQueue

pytestmark = pytest.mark.gpu

WAIT_MS = 20000
WINDOWS = [(0, 5000), (0, 70000), (100, 101)]   # k, worker_bits 0: 256 local indices per k


def test_batch_counts_what_the_round_plan_holds(miner):
    tasks = [BatchTask([1, 2, 3, 4 + i], 32, 0, 0, kb, ke) for i, (kb, ke) in enumerate(WINDOWS)]
    entries, launches = distpow.batch_plan([(kb, ke, 0) for kb, ke in WINDOWS])
    planned = sum(e.i_end - e.i_begin for e in entries)
    assert planned == 256 * sum(ke - kb for kb, ke in WINDOWS) and launches >= 2
    res = miner.search_batch(tasks)
    st = miner.last_batch_stats
    print(f"batch: {st.launches} launches, {st.rounds} rounds, {st.candidates} candidates; plan {launches}, {planned}")
    assert [r.status for r in res] == [EXHAUSTED] * 3
    assert st.launches == launches and st.rounds == launches
    assert st.candidates == planned


def test_queue_counts_what_the_launch_plan_holds(miner):
    kb, ke = WINDOWS[1]
    left, age, launches = (ke - kb) * 256, 0, 0
    while left:
        blocks, _ = distpow.queue_plan([left], [age])
        left -= sum(b.i_end - b.i_begin for b in blocks)
        age += 1
        launches += 1
    assert launches >= 2
    with TaskQueue(0) as q:
        before = q.stats()[0]
        r = q.wait(q.submit(BatchTask([1, 2, 3, 4], 32, 0, 0, kb, ke)), WAIT_MS)
        after = q.stats()[0]
    assert r is not None and r.status == EXHAUSTED
    print(f"queue: result {r.launches} launches, stats {after.launches - before.launches} launches, "
          f"{after.candidates - before.candidates} candidates; plan {launches}")
    assert r.launches == launches
    assert after.launches - before.launches == launches
    assert after.candidates - before.candidates == (ke - kb) * 256
