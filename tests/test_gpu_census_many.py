"""GPU: the batched census (dpow_census_batch, Miner.census_many / census_batch) -- the census of
many tasks in one pass.

Every expectation comes from something that is not this kernel: a Python loop over hashlib, the
committed CPU-scanned hit lists (tests/golden/layout_deep_hits.json), the specialised search kernels
(Miner.search), the scan (Miner.scan) and the one-task census (Miner.census).  One launch mixes
message layouts, partition widths and chunk lengths, and every task's answer is compared count by
count, so cross-talk between the workgroups of different tasks shows as a wrong number.

_nonce, _depths and _census_of are tests/test_gpu_census.py's, restated.  Each test prints its time
(pytest -s).
"""
import ctypes
import hashlib
import json
import os
import random
import threading
import time

import pytest

import distpow
from distpow import CANCELLED, EINVAL, EXHAUSTED, FOUND, Census, CensusTask
from distpow import _lib

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_deep_hits.json")) as _f:
    CASES = {c["name"]: c for c in json.load(_f)["cases"]}
D = _lib.CENSUS_DEPTHS


def _secret_of(g):
    out, k = [g & 0xFF], g >> 8
    while k:
        out.append(k & 0xFF)
        k >>= 8
    return bytes(out)


def _thread_bytes(wb, wbits):
    """worker.go:302-316."""
    rbits = 8 - wbits % 9
    return sorted(((wb << rbits) | i) & 0xFF for i in range(1 << rbits))


def _nonce(n, salt=0):
    rnd = random.Random(1000 * n + salt)
    return bytes(rnd.randrange(256) for _ in range(n))


def _depths(nonce, wb, wbits, k0, k1):
    """The reference's enumeration (k outer, threadByte inner) with hashlib: [(global index, depth)]."""
    base, tbs, out = hashlib.md5(bytes(nonce)), _thread_bytes(wb, wbits), []
    for k in range(k0, k1):
        for tb in tbs:
            h = base.copy()
            h.update(_secret_of(k << 8 | tb))
            hx = h.hexdigest()
            out.append((k << 8 | tb, 32 - len(hx.rstrip("0"))))
    return out


def _census_of(pairs, d_from=0):
    """The census of [(global index, depth)] in index order, from depth d_from up, as a Census."""
    count, first, tz = [0] * D, [None] * D, [0] * D
    for g, t in pairs:
        for d in range(d_from, t + 1):
            count[d] += 1
            if first[d] is None:
                first[d], tz[d] = g, t
    return Census(tuple(count), tuple(first), tuple(tz), max((d for d in range(D) if count[d]), default=0))


def _same_from(c, exp, d_from):
    return (c.count_ge[d_from:], c.first_ge[d_from:], c.first_tz[d_from:]) == \
           (exp.count_ge[d_from:], exp.first_ge[d_from:], exp.first_tz[d_from:])


def _expected(task):
    return _census_of(_depths(task.nonce, task.worker_byte, task.worker_bits, task.k_begin, task.k_end))


def _against_hashlib(miner, tasks, what):
    """One census_batch call of `tasks` against hashlib, task by task: every task EXHAUSTED at its
    k_end with all 33 counts, firsts and depths.  Returns the expected censuses."""
    t = time.perf_counter()
    exp = [_expected(task) for task in tasks]
    t_cpu = time.perf_counter() - t
    t = time.perf_counter()
    got = miner.census_batch(tasks)
    dt = time.perf_counter() - t
    st = miner.last_census_many_stats
    assert len(got) == len(tasks)
    for j, (task, (status, c, k_done), e) in enumerate(zip(tasks, got, exp)):
        assert (status, k_done) == (EXHAUSTED, task.k_end), j
        assert c == e, (j, task.k_begin, task.k_end)
    assert st.candidates == sum(e.count_ge[0] for e in exp)
    print(f"{what}: {len(tasks)} tasks, {st.candidates} candidates, {st.launches} launches, call {dt * 1e3:.2f} ms "
          f"({st.kernel_ms:.3f} ms of kernel), hashlib {t_cpu:.2f} s")
    return exp


def test_every_layout_in_one_launch(miner):
    """132 nonce lengths -- one and two final blocks, midstates, every p / 4 -- in one launch, each
    window 12 k of the full partition from k = 0, 250 or 65530: the second and third cross a
    chunk-length change."""
    tasks = []
    for j, n in enumerate(list(range(131)) + [1024]):
        k0 = (0, 250, 65530)[j % 3]
        tasks.append(CensusTask(_nonce(n, 7), 0, 0, k0, k0 + 12))
    assert len(tasks) == 132
    exp = _against_hashlib(miner, tasks, "every layout")
    assert miner.last_census_many_stats.launches == 1
    assert all(e.count_ge[0] == 3072 for e in exp)
    rare = sum(1 for e in exp if e.deepest >= 3)
    print(f"{rare} of 132 tasks hold a depth >= 3")
    assert rare >= 40  # the LDS path runs in them


def test_partial_waves_beside_each_other(miner):
    """Partition (167, 8) has one candidate per k: eight windows that end inside a wave and inside a
    step, as tasks of one call.  A clamped lane counted once, or in a neighbour's table, shows as a
    wrong count."""
    nonce = _nonce(4, 1)
    tasks = [CensusTask(nonce, 167, 8, 3, 3 + n) for n in (1, 63, 64, 65, 255, 256, 257, 1000)]
    exp = _against_hashlib(miner, tasks, "partial waves")
    assert [e.count_ge[0] for e in exp] == [1, 63, 64, 65, 255, 256, 257, 1000]
    assert miner.last_census_many_stats.launches == 1


def test_4096_one_step_tasks(miner):
    """DPOW_BATCH_MAX tables, the live list at its maximum, descriptors copied to device memory:
    4096 tasks of one workgroup step each, every partition of width 1."""
    tasks = [CensusTask(j.to_bytes(2, "little") + b"\x5a\xa5", j & 255, 8, j, j + 256) for j in range(4096)]
    assert len(tasks) == _lib.DPOW_BATCH_MAX
    exp = _against_hashlib(miner, tasks, "4096 one-step tasks")
    assert miner.last_census_many_stats.launches == 1
    rare = sum(1 for e in exp if e.deepest >= 3)
    print(f"{rare} of 4096 tasks hold a depth >= 3")
    assert rare >= 100


def test_duplicates_and_empties(miner):
    a = CensusTask(_nonce(9, 2), 3, 2, 5, 45)
    b = CensusTask(_nonce(60, 2), 0, 0, 255, 259)
    empty = CensusTask(_nonce(9, 2), 3, 2, 77, 77)
    tasks = [a, a, empty, b, a]
    exp = _against_hashlib(miner, tasks, "duplicates and an empty task")
    assert exp[0] == exp[1] == exp[4] and exp[0].count_ge[0] == 40 * 64
    assert exp[2] == Census.empty()
    # only empty tasks: no launch
    got = miner.census_batch([empty, CensusTask(b"", 0, 0, 0, 0), CensusTask(_nonce(70), 255, 8, 1 << 40, 1 << 40)])
    assert got == [(EXHAUSTED, Census.empty(), 77), (EXHAUSTED, Census.empty(), 0), (EXHAUSTED, Census.empty(), 1 << 40)]
    st = miner.last_census_many_stats
    assert (st.launches, st.rounds, st.candidates) == (0, 0, 0)
    assert miner.census_many([empty]) == [Census.empty()]


def test_launch_seams(miner, monkeypatch):
    """A budget of 4096 local indices per launch (DPOW_DIAG_CENSUS_MANY_CAP): five tasks of 1000, 5000,
    256, 12288 and 3 k at partition (5, 3), 32 candidates per k.  Four of them are cut, each at many
    launch boundaries.  With these sizes a launch holds two tasks at most (only the 3-k task is
    shorter than a launch, and it is the last), so a second call adds launches of three and four."""
    monkeypatch.setenv("DPOW_DIAG_CENSUS_MANY_CAP", "4096")
    for sizes, k0 in (((1000, 5000, 256, 12288, 3), 0), ((100, 3, 2, 200, 1, 130), 65500)):
        tasks = [CensusTask(_nonce(5 + j, 3), 5, 3, k0, k0 + n) for j, n in enumerate(sizes)]
        blocks, launches = distpow.census_plan([(t.k_begin, t.k_end, 3) for t in tasks], 4096)
        per_launch = {}
        for b in blocks:
            per_launch.setdefault(b.launch, set()).add(b.task)
        print(f"plan: {launches} launches, {len(blocks)} descriptors, up to {max(map(len, per_launch.values()))} tasks each")
        _against_hashlib(miner, tasks, f"seams {sizes}")
        st = miner.last_census_many_stats
        assert st.launches == st.rounds == launches > 1
    monkeypatch.delenv("DPOW_DIAG_CENSUS_MANY_CAP")
    # the budget is read per call
    tasks = [CensusTask(_nonce(5, 3), 5, 3, 0, 1000)]
    assert miner.census_many(tasks) == [_expected(tasks[0])]
    assert miner.last_census_many_stats.launches == 1


def test_against_the_other_views(miner):
    """Eight random 4-byte nonces over k in [0, 2^12): first_ge[d] is Miner.search's answer at d,
    count_ge[2] the length of the scan's list at N = 2, the whole census Miner.census's."""
    rnd = random.Random(20240)
    nonces = [bytes(rnd.randrange(256) for _ in range(4)) for _ in range(8)]
    k1 = 1 << 12
    t = time.perf_counter()
    got = miner.census_many([CensusTask(n, 0, 0, 0, k1) for n in nonces])
    dt = time.perf_counter() - t
    assert miner.last_census_many_stats.launches == 1
    for nonce, c in zip(nonces, got):
        assert c.count_ge[0] == k1 * 256
        for d in range(1, 6):
            r = miner.search(nonce, d, 0, 0, 0, k1)
            if c.first_ge[d] is None:
                assert r.status == EXHAUSTED, d
            else:
                assert (r.status, r.global_idx, r.secret) == (FOUND, c.first_ge[d], c.secret(d)), d
        assert c.count_ge[2] == len(miner.scan(nonce, 2, 0, 0, 0, k1))
        assert c == miner.census(nonce, 0, 0, 0, k1)
    print(f"8 tasks of 2^20 candidates: call {dt * 1e3:.2f} ms; deepest {[c.deepest for c in got]}")


def test_committed_lists_across_launches(miner):
    """The CPU-scanned lists of len02, len56 and mid115 (one final block, two final blocks, a
    midstate) in one call: 2.5e10 candidates, 95 launches, both seams inside a launch."""
    names = ["len02", "len56", "mid115"]
    cs = [CASES[n] for n in names]
    t = time.perf_counter()
    got = miner.census_batch([CensusTask(c["nonce"], 0, 0, c["k_begin"], c["k_end"]) for c in cs])
    dt = time.perf_counter() - t
    st = miner.last_census_many_stats
    total = sum((c["k_end"] - c["k_begin"]) * 256 for c in cs)
    assert st.candidates == total and st.launches == (total + (1 << 28) - 1) >> 28
    for name, c, (status, census, k_done) in zip(names, cs, got):
        assert (status, k_done) == (EXHAUSTED, c["k_end"]), name
        assert _same_from(census, _census_of(sorted((g, tz) for g, tz in c["hits"]), 8), 8), name
        assert census.count_ge[0] == (c["k_end"] - c["k_begin"]) * 256, name
        assert census.deepest == max(tz for _, tz in c["hits"]), name
    print(f"{names}: {total} candidates, {st.launches} launches in {dt * 1e3:.1f} ms ({st.kernel_ms:.1f} ms of kernel)")


def test_cancel_raised_on_entry(miner):
    tasks = [CensusTask([1, 2, 3, 4], 0, 0, 7, 64), CensusTask(b"", 1, 1, 9, 9), CensusTask(_nonce(80), 0, 0, 0, 1 << 30)]
    miner.cancel()
    try:
        got = miner.census_batch(tasks)
    finally:
        miner.clear_cancel()
    assert got == [(CANCELLED, Census.empty(), 7), (CANCELLED, Census.empty(), 9), (CANCELLED, Census.empty(), 0)]
    assert miner.last_census_many_stats.launches == 0


def test_cancel_mid_call(miner):
    """One 2^30-k task (partition (9, 4): 2^34 candidates, 64 launches) followed by four small ones,
    the flag raised from a thread while the call runs."""
    nonce, k_end, out = [1, 2, 3, 4], 1 << 30, {}
    small = [CensusTask(_nonce(6, j), j, 2, 10 * j, 10 * j + 50) for j in range(1, 4)] + [CensusTask(b"x", 0, 0, 4, 4)]
    tasks = [CensusTask(nonce, 9, 4, 0, k_end)] + small

    def run():
        out["r"] = miner.census_batch(tasks)
        out["t_end"] = time.perf_counter()

    th = threading.Thread(target=run)
    th.start()
    time.sleep(0.02)
    t_cancel = time.perf_counter()
    miner.cancel()
    th.join(timeout=30)
    miner.clear_cancel()
    assert not th.is_alive()
    status, c, k_done = out["r"][0]
    launches = miner.last_census_many_stats.launches
    print(f"census_batch cancel latency {(out['t_end'] - t_cancel) * 1e3:.2f} ms at k {k_done}, {launches} launches")
    # the cut task: cancelled at a launch boundary, with the complete census of [0, k_done)
    assert status == CANCELLED and 0 <= k_done < k_end
    assert k_done * 16 == launches << 28 == miner.last_census_many_stats.candidates
    assert c == miner.census(nonce, 9, 4, 0, k_done)
    # the tasks not begun: cancelled where they start, but for the empty one
    assert out["r"][1:4] == [(CANCELLED, Census.empty(), t.k_begin) for t in small[:3]]
    assert out["r"][4] == (EXHAUSTED, Census.empty(), 4)
    # a second call from k_done finishes every task, and the first task's parts merge to its window's census
    rest = miner.census_batch([CensusTask(nonce, 9, 4, k_done, k_end)] + small)
    assert [s for s, _, _ in rest] == [EXHAUSTED] * 5 and rest[0][2] == k_end
    assert c.merged(rest[0][1]) == miner.census(nonce, 9, 4, 0, k_end)
    for t, (_, got, k) in zip(small, rest[1:]):
        assert (got, k) == (miner.census(t.nonce, t.worker_byte, t.worker_bits, t.k_begin, t.k_end), t.k_end)


def test_node_slot_attached_is_refused_and_stats_stay(miner):
    class Slot(ctypes.Structure):
        """dpow_node_slot (include/dpow.h)."""
        _fields_ = [("best", ctypes.c_uint64), ("stop", ctypes.c_uint32), ("pad", ctypes.c_uint32 * 13)]

    slot = Slot()
    addr = ctypes.addressof(slot)
    distpow.lib().dpow_node_slot_reset(addr)
    miner.attach_node(addr)
    try:
        with pytest.raises(distpow.DpowError) as e:
            miner.census_many([CensusTask([1, 2, 3, 4], k_end=8)])
        assert e.value.code == EINVAL
    finally:
        miner.attach_node(None)
    # the context is still usable, and the call leaves dpow_stats alone
    miner.reset_stats()
    t = CensusTask([1, 2, 3, 4], k_end=2)
    assert miner.census_many([t]) == [_expected(t)]
    st = miner.stats()
    assert (st.searches, st.launches, st.candidates) == (0, 0, 0)
