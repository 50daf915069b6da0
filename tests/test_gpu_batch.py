"""The batched search on the GPU (dpow_search_batch, Miner.search_batch / mine_many): every answer
against the CPU oracle, hashlib or tests/golden/pow_golden.json, never against the batch itself."""
import random
import threading
import time

import pytest

import distpow
from distpow import CANCELLED, DPOW_NO_HIT, EXHAUSTED, FOUND, BatchTask

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 4, 7, 52, 53, 54, 55, 56, 63, 64, 65, 119, 120, 128, 416]
BOUNDARIES = [1, 256, 65536, 1 << 24, 1 << 32, 1 << 40, 1 << 48]   # chunk-length changes (k = 0 -> 1 first)
SEED = 20240611


def _expect(oracle, t):
    """SearchResult fields the oracle gives for a BatchTask (the bound applied as dpow_search does)."""
    r = oracle.mine_window(list(t.nonce), t.num_trailing_zeros, t.worker_byte, t.worker_bits, t.k_begin, t.k_end)
    if r is None or r[1] >= t.bound:
        return (EXHAUSTED, DPOW_NO_HIT, None)
    return (FOUND, r[1], bytes(r[0]))


def _got(res):
    return (res.status, res.global_idx, res.secret)


def layout_tasks():
    """About 200 tasks: every nonce length crossed with windows of 8-64 k that start just below a
    chunk-length change, worker_bits cycling through {0, 3, 8, 9}, N = 2; and N = 6 tasks on 16-k
    windows (no hit there by the oracle: checked in the test)."""
    rnd = random.Random(SEED)
    tasks = []
    for li, nl in enumerate(LENGTHS):
        nonce = bytes(rnd.randrange(256) for _ in range(nl))
        for bi, edge in enumerate(BOUNDARIES):
            width = rnd.randrange(8, 65)
            kb = edge - min(edge, rnd.randrange(1, width))   # starts below the edge, ends above it
            wbits = [0, 3, 9, 0, 3, 0, 8, 9, 3, 0][(li + bi) % 10]
            wb = rnd.randrange(1 << (wbits % 9))
            tasks.append(BatchTask(nonce, 2, wb, wbits, kb, kb + width))
    for li, nl in enumerate(LENGTHS):
        for edge in (BOUNDARIES[li % 7], BOUNDARIES[(li + 3) % 7], BOUNDARIES[(li + 5) % 7], 5000 + li):
            nonce = bytes(rnd.randrange(256) for _ in range(nl))
            tasks.append(BatchTask(nonce, 6, 0, 0, edge - 5 if edge > 5 else 0, (edge - 5 if edge > 5 else 0) + 16))
    return tasks


@pytest.fixture(scope="module")
def layout(miner, oracle):
    tasks = layout_tasks()
    expected = [_expect(oracle, t) for t in tasks]
    results = miner.search_batch(tasks)
    return tasks, expected, results


def test_goldens_in_one_batch(miner):
    tasks = [BatchTask([1, 2, 3, 4], 3, k_end=1 << 12), BatchTask([1, 2, 3, 4], 6, k_end=1 << 16),
             BatchTask([5, 6, 7, 8], 5, k_end=1 << 16), BatchTask([2, 2, 2, 2], 5, k_end=1 << 16)]
    tasks += [BatchTask([1, 2, 3, 4], 7, wb, 2, 0, 1 << 20) for wb in range(4)]
    res = miner.search_batch(tasks)
    assert [list(r.secret) for r in res[:4]] == [[97], [188, 163, 38], [84, 244, 3], [48, 119]]
    assert all(r.status == FOUND for r in res[:4])
    for r, t in zip(res[:4], tasks):
        assert r.secret == distpow.secret_from_index(r.global_idx)
        assert distpow.verify(t.nonce, r.secret, t.num_trailing_zeros)
    parts = [r for r in res[4:] if r.status == FOUND]
    assert parts, res[4:]
    best = min(parts, key=lambda r: r.global_idx)
    assert list(best.secret) == [194, 170, 210, 13]
    for wb, r in enumerate(res[4:]):  # a partition's hit lies in that partition
        if r.status == FOUND:
            assert (r.global_idx & 0xFF) >> 6 == wb


def test_layout_and_boundary_batch(layout):
    tasks, expected, results = layout
    assert 190 <= len(tasks) <= 210
    n2 = [e for t, e in zip(tasks, expected) if t.num_trailing_zeros == 2]
    n6 = [e for t, e in zip(tasks, expected) if t.num_trailing_zeros == 6]
    assert len(n2) == len(LENGTHS) * len(BOUNDARIES)
    assert sum(e[0] == FOUND for e in n2) * 4 >= 3 * len(n2)   # by the oracle alone: no all-exhausted pass
    assert n6 and all(e[0] == EXHAUSTED for e in n6)
    for i, (t, e, r) in enumerate(zip(tasks, expected, results)):
        assert _got(r) == e, (i, t, e, r)


def test_batch_equals_search(miner, layout):
    tasks, expected, results = layout
    step = len(tasks) // 32
    for t, r in list(zip(tasks, results))[::step][:32]:
        s = miner.search(t.nonce, t.num_trailing_zeros, t.worker_byte, t.worker_bits, t.k_begin, t.k_end, t.bound)
        assert _got(s) == _got(r), (t, s, r)


def test_bounds_in_one_batch(miner, oracle):
    base = BatchTask([1, 2, 3, 4], 4, 0, 0, 0, 1 << 12)
    st, g, sec = _expect(oracle, base)
    assert st == FOUND
    at = BatchTask(base.nonce, 4, 0, 0, 0, 1 << 12, bound=g)
    above = BatchTask(base.nonce, 4, 0, 0, 0, 1 << 12, bound=g + 1)
    r_at, r_above, r_free = miner.search_batch([at, above, base])
    assert _got(r_at) == (EXHAUSTED, DPOW_NO_HIT, None)
    assert _got(r_above) == (FOUND, g, sec) and _got(r_free) == (FOUND, g, sec)
    assert _got(r_at) == _expect(oracle, at)


def test_long_among_short(miner, oracle):
    rnd = random.Random(SEED + 1)
    tasks = [BatchTask([1, 2, 3, 4], 6, 0, 0, 0, 1 << 16)]
    tasks += [BatchTask(bytes(rnd.randrange(256) for _ in range(4)), 2, 0, 0, 0, 64) for _ in range(63)]
    tasks.append(BatchTask([9, 9, 9, 9], 6, 0, 0, 100, 116))
    expected = [_expect(oracle, t) for t in tasks]
    assert expected[0][0] == FOUND and expected[-1][0] == EXHAUSTED
    res = miner.search_batch(tasks)
    assert [_got(r) for r in res] == expected
    assert miner.last_batch_stats.rounds > 1        # the long task's survivors carried over
    assert miner.last_batch_stats.launches == miner.last_batch_stats.rounds


@pytest.mark.parametrize("n", [1, 2, 65, 1024])
def test_batch_sizes(miner, oracle, n):
    rnd = random.Random(SEED + n)
    tasks = [BatchTask(bytes(rnd.randrange(256) for _ in range(rnd.choice([0, 4, 9]))), 1, 0, 0,
                       kb, kb + 4) for kb in (rnd.randrange(1 << 20) for _ in range(n))]
    tasks[n // 2] = BatchTask(tasks[n // 2].nonce, 1, 0, 0, 7, 7)   # an empty window
    before = miner.stats().searches
    res = miner.search_batch(tasks)
    assert [_got(r) for r in res] == [_expect(oracle, t) for t in tasks]
    assert res[n // 2].status == EXHAUSTED
    assert miner.stats().searches == before          # a batch does not touch dpow_stats
    assert miner.last_batch_stats.candidates >= 1024 * (n - 1) or n == 1


def test_n9_task_among_small(miner, golden, oracle):
    deep = next(h for h in golden["deep_hits"] if h["ntz"] == 9)
    k = deep["global_idx"] >> 8
    rnd = random.Random(SEED + 9)
    tasks = [BatchTask(bytes(rnd.randrange(256) for _ in range(4)), 2, 0, 0, 0, 32) for _ in range(8)]
    tasks.insert(3, BatchTask(deep["nonce"], 9, 0, 0, k - 2048, k + 2048))
    res = miner.search_batch(tasks)
    assert _got(res[3]) == (FOUND, deep["global_idx"], bytes(deep["secret"]))
    for t, r in zip(tasks[:3] + tasks[4:], res[:3] + res[4:]):
        assert _got(r) == _expect(oracle, t)


def test_cancel_raised_on_entry(miner):
    miner.cancel()
    try:
        res = miner.search_batch([BatchTask([1, 2, 3, 4], 2, k_end=64), BatchTask([5], 3, k_end=64)])
    finally:
        miner.clear_cancel()
    assert [r.status for r in res] == [CANCELLED, CANCELLED]
    assert miner.last_batch_stats.launches == 0


def test_cancel_mid_batch(miner, oracle):
    tasks = [BatchTask([1, 2, 3, i], 32, 0, 0, 1 << 24, (1 << 24) + (1 << 30)) for i in range(8)]
    out = {}

    def run():
        out["r"] = miner.search_batch(tasks)
        out["t_end"] = time.perf_counter()

    th = threading.Thread(target=run)
    th.start()
    time.sleep(0.05)
    t_cancel = time.perf_counter()
    miner.cancel()
    th.join(timeout=30)
    miner.clear_cancel()
    assert not th.is_alive()
    latency = out["t_end"] - t_cancel
    print(f"batch cancel latency {latency * 1e3:.2f} ms, {miner.last_batch_stats.launches} launches")
    assert [r.status for r in out["r"]] == [CANCELLED] * 8
    assert latency < 0.25
    # the context is usable right after
    t = BatchTask([1, 2, 3, 4], 3, 0, 0, 0, 1 << 12)
    assert _got(miner.search(t.nonce, 3, 0, 0, 0, 1 << 12)) == _expect(oracle, t)


def test_mine_many(miner, oracle):
    rnd = random.Random(SEED + 4)
    reqs = [BatchTask(bytes(rnd.randrange(256) for _ in range(4)), 4) for _ in range(16)]
    res = miner.mine_many(reqs)
    for t, r in zip(reqs, res):
        exp = oracle.mine_window(list(t.nonce), 4, 0, 0, 0, 1 << 14)
        assert exp is not None
        assert _got(r) == (FOUND, exp[1], bytes(exp[0])), (t, r)


def test_node_slot_attached_is_refused(miner):
    import ctypes

    class Slot(ctypes.Structure):
        """dpow_node_slot (include/dpow.h)."""
        _fields_ = [("best", ctypes.c_uint64), ("stop", ctypes.c_uint32), ("pad", ctypes.c_uint32 * 13)]

    slot = Slot()
    addr = ctypes.addressof(slot)
    distpow.lib().dpow_node_slot_reset(addr)
    miner.attach_node(addr)
    try:
        with pytest.raises(distpow.DpowError) as e:
            miner.search_batch([BatchTask([1, 2, 3, 4], 2, k_end=8)])
        assert e.value.code == distpow.EINVAL
    finally:
        miner.attach_node(None)
    assert miner.search_batch([BatchTask([1, 2, 3, 4], 0, k_end=8)])[0].global_idx == 0
