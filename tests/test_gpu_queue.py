"""The task queue on the GPU (dpow_queue_*, distpow.TaskQueue): every answer against the CPU oracle,
hashlib or tests/golden/pow_golden.json, never against the queue or the batch.  Every wait has a
finite time-out, so a bug fails a test and does not hang it."""
import random
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

import distpow
from distpow import CANCELLED, DPOW_NO_HIT, EXHAUSTED, FOUND, BatchTask, TaskQueue

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 4, 7, 52, 53, 54, 55, 56, 63, 64, 65, 119, 120, 128, 416]   # tests/test_gpu_batch.py
EDGES = [0, 1, 256, 65536, 1 << 24, 1 << 32, 1 << 40, 1 << 48]
WAIT_MS = 20000
N7 = BatchTask([1, 2, 3, 4], 7, 0, 0, 0, 1 << 20)
N7_SECRET = [194, 170, 210, 13]


def _expect(oracle, t):
    r = oracle.mine_window(list(t.nonce), t.num_trailing_zeros, t.worker_byte, t.worker_bits, t.k_begin, t.k_end)
    if r is None or r[1] >= t.bound:
        return (EXHAUSTED, DPOW_NO_HIT, None)
    return (FOUND, r[1], bytes(r[0]))


def _expect_all(oracle, tasks):
    """The oracle's answers, on a few host threads (the oracle runs outside the interpreter lock)."""
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda t: _expect(oracle, t), tasks))


def _got(res):
    r = res.result
    return (r.status, r.global_idx, r.secret)


def _collect(q, n):
    out = {}
    for _ in range(n):
        r = q.next(WAIT_MS)
        assert r is not None, f"time-out with {len(out)} of {n} results"
        assert r.ticket not in out
        out[r.ticket] = r
    return out


@pytest.fixture()
def queue(miner):
    with TaskQueue(0) as q:
        yield q


def mix_tasks():
    rnd = random.Random(20251020)
    tasks = []
    for i in range(144):
        nonce = bytes(rnd.randrange(256) for _ in range(LENGTHS[i % 18]))
        n = [2, 3, 4][i % 3]
        wbits = [0, 3, 8, 9][(i // 3) % 4]
        wb = rnd.randrange(1 << (wbits % 9))
        edge = EDGES[(i // 2) % 8]
        width = {2: 64, 3: 256, 4: 1024}[n]
        kb = max(0, edge - rnd.randrange(1, 9))
        tasks.append(BatchTask(nonce, n, wb, wbits, kb, kb + width))
    return tasks


@pytest.fixture(scope="module")
def mix(oracle):
    tasks = mix_tasks()
    expected = _expect_all(oracle, tasks)
    found = sum(e[0] == FOUND for e in expected)
    assert 2 * found >= len(tasks) and 8 * (len(tasks) - found) >= len(tasks), found   # by the oracle alone
    return tasks, expected


def test_goldens_one_by_one_then_together(queue):
    singles = [(BatchTask([1, 2, 3, 4], 3, k_end=1 << 16), [97]), (BatchTask([1, 2, 3, 4], 6, k_end=1 << 16), [188, 163, 38]),
               (BatchTask([5, 6, 7, 8], 5, k_end=1 << 16), [84, 244, 3]), (BatchTask([2, 2, 2, 2], 5, k_end=1 << 16), [48, 119])]
    for t, secret in singles:
        ticket = queue.submit(t, user=7)
        r = queue.next(WAIT_MS)
        assert r is not None and r.ticket == ticket and r.user == 7
        assert r.status == FOUND and list(r.result.secret) == secret
        assert r.result.secret == distpow.secret_from_index(r.result.global_idx)
        assert distpow.verify(t.nonce, r.result.secret, t.num_trailing_zeros)
        assert r.launches >= 1 and r.queued_ms > 0
    tickets = [queue.submit(t) for t, _ in singles]
    parts = [queue.submit(BatchTask([1, 2, 3, 4], 7, wb, 2, 0, 1 << 20), user=100 + wb) for wb in range(4)]
    assert len(set(tickets + parts)) == 8 and 0 not in tickets + parts
    got = _collect(queue, 8)
    for ticket, (t, secret) in zip(tickets, singles):
        assert got[ticket].status == FOUND and list(got[ticket].result.secret) == secret
    hits = [got[p] for p in parts if got[p].status == FOUND]
    assert hits
    assert list(min(hits, key=lambda r: r.result.global_idx).result.secret) == N7_SECRET
    for wb, p in enumerate(parts):   # a partition's hit lies in that partition
        assert got[p].user == 100 + wb
        if got[p].status == FOUND:
            assert (got[p].result.global_idx & 0xFF) >> 6 == wb
    assert queue.stats()[1:] == (0, 0)


def test_seeded_mix_three_ways(mix, miner):
    tasks, expected = mix
    with TaskQueue(0) as q:
        # all submitted before the first next()
        tickets = [q.submit(t, user=i) for i, t in enumerate(tasks)]
        got = _collect(q, len(tasks))
        for i, ticket in enumerate(tickets):
            assert got[ticket].user == i and _got(got[ticket]) == expected[i], (i, tasks[i], expected[i], got[ticket])
        # submitted from 4 threads while a fifth collects
        got, errors = {}, []

        def collector():
            try:
                got.update(_collect(q, len(tasks)))
            except Exception as e:   # noqa: BLE001
                errors.append(e)

        def submitter(part):
            try:
                for i in range(part, len(tasks), 4):
                    q.submit(tasks[i], user=i)
            except Exception as e:   # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=collector)] + [threading.Thread(target=submitter, args=(p,)) for p in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=30)
        assert not errors and not any(th.is_alive() for th in threads), errors
        assert sorted(r.user for r in got.values()) == list(range(len(tasks)))
        for r in got.values():
            assert _got(r) == expected[r.user], (r.user, tasks[r.user], expected[r.user], r)
        # groups of 9 with one next() after each group: slots are reused by tasks of another layout
        # while older tasks are still live
        got = {}
        for off in range(0, len(tasks), 9):
            for i in range(off, off + 9):
                q.submit(tasks[i], user=i)
            r = q.next(WAIT_MS)
            assert r is not None
            got[r.user] = r
        for r in _collect(q, len(tasks) - len(got)).values():
            got[r.user] = r
        assert sorted(got) == list(range(len(tasks)))
        for i, r in got.items():
            assert _got(r) == expected[i], (i, tasks[i], expected[i], r)
        st, live, unc = q.stats()
        assert (live, unc) == (0, 0) and st.launches >= 3 and st.launches == st.rounds and st.kernel_ms > 0


def _small_tasks(seed, n):
    rnd = random.Random(seed)
    return [BatchTask(bytes(rnd.randrange(256) for _ in range(4)), 2, 0, 0, 0, 64) for _ in range(n)]


def test_ages_differ_in_one_launch(queue, oracle):
    """Fresh small tasks beside one old task: each is answered by the one launch it joins, while the
    old task goes on through its own, longer slices."""
    small = _small_tasks(20251021, 64)
    expected = _expect_all(oracle, small)
    big = queue.submit(N7)
    undecided = 0
    for off in range(0, 64, 8):
        undecided += queue.stats()[1] >= 1
        tickets = [queue.submit(t, user=off + j) for j, t in enumerate(small[off:off + 8])]
        for j, ticket in enumerate(tickets):   # every small task is collected before the N = 7 task
            r = queue.wait(ticket, WAIT_MS)
            assert r is not None and r.user == off + j
            assert _got(r) == expected[off + j], (off + j, r)
            assert r.launches == 1
    r = queue.wait(big, WAIT_MS)
    assert r is not None and r.status == FOUND and list(r.result.secret) == N7_SECRET
    assert r.launches >= 3
    print(f"N = 7 task: {r.launches} launches, {r.queued_ms:.2f} ms; undecided at {undecided} of 8 groups")


def test_cancel(queue, oracle, golden):
    # (a) right after submit
    big = queue.submit(N7)
    t0 = time.perf_counter()
    assert queue.cancel(big) is True
    r = queue.wait(big, WAIT_MS)
    latency = time.perf_counter() - t0
    assert r is not None and r.status == CANCELLED and r.result.secret is None
    assert queue.cancel(big) is False
    print(f"cancel latency {latency * 1e6:.0f} us")
    # (b) fresh tasks after a cancel: some land in the cancelled task's slot
    small = _small_tasks(20251022, 32)
    expected = _expect_all(oracle, small)
    tickets = [queue.submit(t) for t in small]
    got = _collect(queue, 32)
    assert [_got(got[t]) for t in tickets] == expected
    # (c) a ticket that is decided already
    t = queue.submit(BatchTask([1, 2, 3, 4], 3, k_end=1 << 16))
    deadline = time.perf_counter() + 20
    while queue.stats()[2] == 0 and time.perf_counter() < deadline:
        time.sleep(0.001)
    assert queue.cancel(t) is False
    r = queue.wait(t, WAIT_MS)
    assert r is not None and r.status == FOUND and list(r.result.secret) == [97]
    # (d) half of 32 live N = 6 tasks
    rnd = random.Random(20251023)
    six = [BatchTask([1, 2, 3, 4], 6, k_end=1 << 16)] + [BatchTask(bytes(rnd.randrange(256) for _ in range(4)), 6, k_end=1 << 16)
                                                         for _ in range(31)]
    keep = list(range(0, 32, 2))
    expected = dict(zip(keep, _expect_all(oracle, [six[i] for i in keep])))
    assert expected[0] == (FOUND, 2532284, bytes([188, 163, 38]))   # the golden
    tickets = [queue.submit(t, user=i) for i, t in enumerate(six)]
    t0 = time.perf_counter()
    flags = [queue.cancel(tickets[i]) for i in range(1, 32, 2)]
    got = _collect(queue, 32)
    print(f"16 cancels and 32 results in {(time.perf_counter() - t0) * 1e3:.2f} ms")
    for i in range(32):
        r = got[tickets[i]]
        if i % 2 == 0:
            assert _got(r) == expected[i], (i, r)
        elif flags[i // 2]:
            assert r.status == CANCELLED
        else:   # decided before its cancel came
            assert r.status in (FOUND, EXHAUSTED)
    assert sum(flags) >= 1


def test_bounds_and_empty_windows(queue, oracle):
    base = BatchTask([1, 2, 3, 4], 4, 0, 0, 0, 1 << 12)
    st, g, sec = _expect(oracle, base)
    assert st == FOUND
    at = BatchTask(base.nonce, 4, 0, 0, 0, 1 << 12, bound=g)
    above = BatchTask(base.nonce, 4, 0, 0, 0, 1 << 12, bound=g + 1)
    tickets = [queue.submit(t) for t in (at, above, base)]
    got = _collect(queue, 3)
    assert _got(got[tickets[0]]) == (EXHAUSTED, DPOW_NO_HIT, None) == _expect(oracle, at)
    assert _got(got[tickets[1]]) == (FOUND, g, sec) and _got(got[tickets[2]]) == (FOUND, g, sec)
    before = queue.stats()[0]
    empty = BatchTask([1, 2, 3, 4], 1, 0, 0, 7, 7)
    bounded = BatchTask([1, 2, 3, 4], 1, 0, 0, 5, 9, bound=5 << 8)
    for t in (empty, bounded):
        ticket = queue.submit(t)
        r = queue.wait(ticket, WAIT_MS)
        assert r is not None and _got(r) == _expect(oracle, t) == (EXHAUSTED, DPOW_NO_HIT, None)
        assert r.launches == 0
    after = queue.stats()[0]
    assert (after.launches, after.candidates) == (before.launches, before.candidates)


def test_equals_search_and_search_batch(queue, miner, mix):
    tasks, expected = mix
    pick = list(range(0, 144, 144 // 32))[:32]
    batch = miner.search_batch([tasks[i] for i in pick])
    tickets = [queue.submit(tasks[i]) for i in pick]
    got = _collect(queue, 32)
    for i, b, ticket in zip(pick, batch, tickets):
        t = tasks[i]
        s = miner.search(t.nonce, t.num_trailing_zeros, t.worker_byte, t.worker_bits, t.k_begin, t.k_end, t.bound)
        a = (s.status, s.global_idx, s.secret)
        assert a == (b.status, b.global_idx, b.secret) == _got(got[ticket]), (i, t, s, b, got[ticket])


def test_limits_and_close(miner, oracle):
    rnd = random.Random(20251024)
    n_max = distpow._lib.DPOW_BATCH_MAX
    tasks = [BatchTask(bytes(rnd.randrange(256) for _ in range(8)), 8, 0, 0, 1 << 20, (1 << 20) + 64)
             for _ in range(n_max + 1)]
    expected = _expect_all(oracle, tasks)
    assert sum(e[0] == EXHAUSTED for e in expected[:n_max]) >= 4080
    q = TaskQueue(0)
    try:
        tickets = [q.submit(t, user=i) for i, t in enumerate(tasks[:n_max])]
        with pytest.raises(distpow.DpowError) as e:
            q.submit(tasks[n_max], user=n_max)
        assert e.value.code == distpow.EAGAIN
        first = q.next(WAIT_MS)
        assert first is not None
        tickets.append(q.submit(tasks[n_max], user=n_max))
        got = _collect(q, n_max)
        got[first.ticket] = first
        assert len(set(tickets)) == n_max + 1 and set(got) == set(tickets)
        for i, ticket in enumerate(tickets):
            assert got[ticket].user == i and _got(got[ticket]) == expected[i], (i, got[ticket])
        # close with live tasks: windows far too long to end
        for i in range(8):
            q.submit(BatchTask(tasks[i].nonce, 32, 0, 0, 1 << 24, (1 << 24) + (1 << 30)))
        time.sleep(0.01)
        assert q.stats()[1] == 8
        t0 = time.perf_counter()
    finally:
        q.close()
    assert time.perf_counter() - t0 < 20
    # a new queue on the same device works, and so do two at once
    with TaskQueue(0) as q1, TaskQueue(0) as q2:
        a = q1.submit(BatchTask([1, 2, 3, 4], 3, k_end=1 << 16))
        b = q2.submit(BatchTask([2, 2, 2, 2], 5, k_end=1 << 16))
        ra, rb = q1.wait(a, WAIT_MS), q2.wait(b, WAIT_MS)
        assert ra is not None and list(ra.result.secret) == [97]
        assert rb is not None and list(rb.result.secret) == [48, 119]
