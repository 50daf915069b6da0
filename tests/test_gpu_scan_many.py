"""GPU: the batched scan (dpow_scan_batch, Miner.scan_batch, Miner.scan_many) -- every hit of many
windows in one call, each task's list what Miner.scan returns for it.

Every expectation comes from something that is not this kernel: a Python loop over hashlib, the
committed CPU-scanned hit lists (tests/golden/layout_deep_hits.json) and Miner.scan.  One launch
mixes message layouts, partition widths, chunk lengths and depths, so a hit filed under the wrong
task or tested against a neighbour's depth shows as a wrong list.

Each test prints its time (pytest -s).
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
from distpow import CANCELLED, DPOW_K_LIMIT, EINVAL, ERANGE, EXHAUSTED, MORE, ScanHit, ScanTask
from distpow import _lib

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_deep_hits.json")) as _f:
    CASES = {c["name"]: c for c in json.load(_f)["cases"]}


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


def _reference(nonce, ntz, wb, wbits, k0, k1):
    """The reference's enumeration (k outer, threadByte inner) with hashlib: every hit as a ScanHit."""
    base, tbs, out = hashlib.md5(bytes(nonce)), _thread_bytes(wb, wbits), []
    for k in range(k0, k1):
        for tb in tbs:
            sec = _secret_of(k << 8 | tb)
            h = base.copy()
            h.update(sec)
            hx = h.hexdigest()
            tz = 32 - len(hx.rstrip("0"))
            if tz >= ntz:
                out.append(ScanHit(k << 8 | tb, tz, sec))
    return out


def _nonce(n, salt=0):
    rnd = random.Random(1000 * n + salt)
    return bytes(rnd.randrange(256) for _ in range(n))


def _ref_of(t, k_begin=None):
    return _reference(t.nonce, t.num_trailing_zeros, t.worker_byte, t.worker_bits,
                      t.k_begin if k_begin is None else k_begin, t.k_end)


def _windows(tasks):
    """The tasks as dpow_scan_plan takes them: local index ranges and depths."""
    return [(t.k_begin << (8 - t.worker_bits % 9), t.k_end << (8 - t.worker_bits % 9), t.num_trailing_zeros)
            for t in tasks]


def _planned_launches(tasks, cap=0):
    return distpow.scan_plan(_windows(tasks), cap)[1]


def test_every_layout_in_one_launch(miner):
    """132 nonce lengths -- every p = len % 64, one and two final blocks, midstates -- at k = 0 and
    across the chunk-length changes at k = 256 and 65536, the depth cycling per task."""
    lens = list(range(131)) + [1024]
    tasks = []
    for j, n in enumerate(lens):
        k0 = (0, 250, 65530)[j // 3 % 3]
        tasks.append(ScanTask(_nonce(n), 1 + j % 3, 0, 0, k0, k0 + 12))
    assert len(tasks) == 132 and _planned_launches(tasks) == 1
    exp = [_ref_of(t) for t in tasks]
    t0 = time.perf_counter()
    got = miner.scan_batch(tasks)
    dt = time.perf_counter() - t0
    st = miner.last_scan_many_stats
    assert st.launches == 1 and st.candidates == 132 * 12 * 256
    for t, (r, hits, k_done), e in zip(tasks, got, exp):
        assert (r, k_done) == (EXHAUSTED, t.k_end), len(t.nonce)
        assert hits == e, (len(t.nonce), t.num_trailing_zeros, t.k_begin)
    assert sum(map(len, exp)) > 5000
    print(f"132 layouts, {sum(map(len, exp))} hits, one launch: {dt * 1e3:.1f} ms")


def _mixed_tasks():
    rnd = random.Random(17)
    tasks = []
    for wbits in range(10):  # workerBits 9 is workerBits 0 (worker.go's % 9)
        legal = 1 << (wbits % 9)
        for wb in sorted({0, legal - 1, rnd.randrange(legal), rnd.randrange(legal)}):
            k0 = rnd.choice((0, 3, 250, 65530, 1 << 24))
            tasks.append(ScanTask(_nonce(rnd.choice((0, 4, 47, 55, 56, 63, 64, 119)), wbits), rnd.choice((0, 1, 2, 5, 32, 40)),
                                  wb, wbits, k0, k0 + rnd.randrange(4, 17)))
    # an N = 0 task next to an N = 32 task of the same window, duplicates, empty tasks
    tasks[3:3] = [ScanTask(_nonce(9), 0, 2, 2, 7, 15), ScanTask(_nonce(9), 32, 2, 2, 7, 15), ScanTask(_nonce(9), 0, 2, 2, 7, 15)]
    tasks.insert(10, ScanTask(_nonce(5), 1, 0, 0, 9, 9))
    tasks.append(tasks[6])
    tasks.append(ScanTask(b"", 0, 255, 8, 77, 77))
    return tasks


def test_mixed_depths_and_partitions(miner):
    tasks = _mixed_tasks()
    assert 30 <= len(tasks) <= 48 and {t.num_trailing_zeros for t in tasks} == {0, 1, 2, 5, 32, 40}
    assert {t.worker_bits for t in tasks} == set(range(10))
    t0 = time.perf_counter()
    got = miner.scan_many(tasks)
    dt = time.perf_counter() - t0
    assert miner.last_scan_many_stats.launches == _planned_launches(tasks)
    for t, hits in zip(tasks, got):
        assert hits == _ref_of(t), t
        assert hits == miner.scan(t.nonce, t.num_trailing_zeros, t.worker_byte, t.worker_bits, t.k_begin, t.k_end), t
    # every index of the N = 0 task, none of its N = 32 neighbour, the duplicate its own copy
    tbs = _thread_bytes(2, 2)
    assert [h.global_idx for h in got[3]] == [k << 8 | tb for k in range(7, 15) for tb in tbs]
    assert got[4] == [] and got[5] == got[3] and got[-2] == got[6] and got[10] == [] and got[-1] == []
    print(f"{len(tasks)} tasks, {sum(map(len, got))} hits: {dt * 1e3:.1f} ms")


def test_many_small_tasks(miner):
    """4096 one-k tasks at N = 1: a descriptor table long enough to be copied to the device first,
    every descriptor a task's only and partial one."""
    tasks = [ScanTask(_nonce(1 + j % 70, j), 1, 0, 0, j % 300, j % 300 + 1) for j in range(4096)]
    exp = [_ref_of(t) for t in tasks]
    t0 = time.perf_counter()
    got = miner.scan_many(tasks)
    dt = time.perf_counter() - t0
    st = miner.last_scan_many_stats
    # 16 hit weight per task: 1024 tasks, so 1024 descriptors, per launch
    assert st.launches == _planned_launches(tasks) == 4 and st.candidates == 4096 * 256
    assert got == exp
    print(f"4096 tasks, {sum(map(len, exp))} hits, {st.launches} launches: {dt * 1e3:.1f} ms")


def _seam_tasks():
    rnd = random.Random(5)
    # 1536, 3072, 1536 and 1024 local indices: each begins a launch under both budgets, so 768 cuts the
    # first at k = 256 and the third at k = 65536, 512 the fourth at k = 256, and both the second
    # (one candidate per k) at k = 65536
    tasks = [ScanTask(_nonce(4, 1), 1, 0, 0, 253, 259), ScanTask(_nonce(70, 2), 0, 131, 8, 65536 - 1536, 65536 + 1536),
             ScanTask(_nonce(60, 3), 2, 0, 0, 65533, 65539), ScanTask(_nonce(4, 4), 0, 0, 0, 254, 258)]
    while len(tasks) < 30:
        wbits = rnd.choice((0, 0, 1, 3, 8))
        k0 = rnd.choice((0, 250, 65530))
        tasks.append(ScanTask(_nonce(rnd.randrange(0, 130), len(tasks)), rnd.choice((0, 1, 2, 3)), rnd.randrange(1 << wbits),
                              wbits, k0, k0 + rnd.randrange(1, 14)))
    return tasks


@pytest.mark.parametrize("cap", [512, 768])
def test_launch_seams(miner, monkeypatch, cap):
    """DPOW_DIAG_SCAN_MANY_CAP puts launch boundaries inside small tasks: the same lists from more launches."""
    tasks = _seam_tasks()
    monkeypatch.delenv("DPOW_DIAG_SCAN_MANY_CAP", raising=False)
    plain = miner.scan_many(tasks)
    launches = miner.last_scan_many_stats.launches
    assert plain == [_ref_of(t) for t in tasks]
    # the plan under the small budget cuts tasks between k = 255 and 256, and between 65535 and 65536
    w = _windows(tasks)
    blocks, n_l = distpow.scan_plan(w, cap)
    cuts = {(b.task, b.i_end) for b, nxt in zip(blocks, blocks[1:]) if b.launch != nxt.launch and b.task == nxt.task}
    cut_k = {i >> (8 - tasks[t].worker_bits % 9) for t, i in cuts}
    assert 256 in cut_k and 65536 in cut_k, sorted(cut_k)
    monkeypatch.setenv("DPOW_DIAG_SCAN_MANY_CAP", str(cap))
    t0 = time.perf_counter()
    seamed = miner.scan_many(tasks)
    dt = time.perf_counter() - t0
    launches_seamed = miner.last_scan_many_stats.launches
    monkeypatch.delenv("DPOW_DIAG_SCAN_MANY_CAP")
    assert seamed == plain
    assert launches_seamed == n_l > launches == _planned_launches(tasks)
    print(f"cap {cap}: {launches_seamed} launches against {launches}, {dt * 1e3:.1f} ms")


def test_overflow_replans_with_halved_budgets(miner, monkeypatch):
    """DPOW_DIAG_SCAN_MANY_LIST=256 shrinks the hit list, not the plan: the same lists from more launches."""
    tasks = [ScanTask(_nonce(4 + 9 * j, j), 1, 0, 0, 100 * j, 100 * j + 128) for j in range(8)]
    exp = [_ref_of(t) for t in tasks]
    # the plain plan's first launch holds all eight tasks, and hashlib counts more than 256 hits in it
    blocks, n_l = distpow.scan_plan(_windows(tasks))
    assert n_l == 1 and sum(b.i_end - b.i_begin for b in blocks) == 8 << 15
    assert sum(map(len, exp)) > 256
    monkeypatch.delenv("DPOW_DIAG_SCAN_MANY_LIST", raising=False)
    plain = miner.scan_many(tasks)
    launches = miner.last_scan_many_stats.launches
    monkeypatch.setenv("DPOW_DIAG_SCAN_MANY_LIST", "256")
    t0 = time.perf_counter()
    small = miner.scan_many(tasks)
    dt = time.perf_counter() - t0
    st = miner.last_scan_many_stats
    monkeypatch.delenv("DPOW_DIAG_SCAN_MANY_LIST")
    assert plain == exp and small == exp
    assert st.launches > launches == 1
    print(f"{sum(map(len, exp))} hits: {launches} launch, {st.launches} with a 256-entry list, {dt * 1e3:.1f} ms")


def _expected_page(tasks, k_from, refs, max_hits):
    """One call's answer by the paging rule: [(status, hits, k_done)] for tasks continued from k_from,
    refs[i] the complete list of task i from k_from[i]."""
    out, room, stopped = [], max_hits, False
    for t, k0, ref in zip(tasks, k_from, refs):
        if k0 == t.k_end:
            out.append((EXHAUSTED, [], k0))
        elif stopped:
            out.append((MORE, [], k0))
        else:
            taken, k_done = [], t.k_end
            for k in sorted({h.global_idx >> 8 for h in ref}):
                of_k = [h for h in ref if h.global_idx >> 8 == k]
                if len(of_k) > room:
                    stopped, k_done = True, k
                    break
                taken += of_k
                room -= len(of_k)
            out.append((MORE if stopped else EXHAUSTED, taken, k_done))
    return out


@pytest.mark.parametrize("max_hits", [256, 1000])
def test_paging(miner, max_hits):
    """A dense mix: every call's statuses, k_done values and hits by the rule, until nothing is left."""
    tasks = [ScanTask(_nonce(4, 1), 0, 0, 0, 3, 6), ScanTask(_nonce(5, 2), 1, 0, 0, 0, 40), ScanTask(b"ab", 0, 5, 5, 9, 9),
             ScanTask(_nonce(6, 3), 0, 1, 2, 250, 262), ScanTask(_nonce(7, 4), 32, 0, 0, 0, 5),
             ScanTask(_nonce(64, 5), 0, 200, 8, 65530, 65545), ScanTask(_nonce(8, 6), 2, 0, 0, 0, 300)]
    whole = [_ref_of(t) for t in tasks]
    assert miner.scan_many(tasks) == whole
    assert miner.scan_many(tasks, max_hits=max_hits) == whole
    k_from, lists, calls = [t.k_begin for t in tasks], [[] for _ in tasks], 0
    t0 = time.perf_counter()
    while any(k != t.k_end for k, t in zip(k_from, tasks)):
        now = [ScanTask(t.nonce, t.num_trailing_zeros, t.worker_byte, t.worker_bits, k, t.k_end) for t, k in zip(tasks, k_from)]
        refs = [[h for h in w if h.global_idx >> 8 >= k] for w, k in zip(whole, k_from)]
        got = miner.scan_batch(now, max_hits=max_hits)
        assert got == _expected_page(now, k_from, refs, max_hits), calls
        assert sum(len(h) for _, h, _ in got) <= max_hits
        for i, (r, hits, k_done) in enumerate(got):
            lists[i] += hits
            k_from[i] = k_done
        calls += 1
        assert calls < 100
    assert lists == whole and calls >= 3
    print(f"max_hits {max_hits}: {sum(map(len, whole))} hits in {calls} calls, {(time.perf_counter() - t0) * 1e3:.1f} ms")


def test_committed_lists(miner):
    """Three layouts' CPU-scanned windows in one call at N = 8: whole lists, with depths."""
    names = ["len02", "len56", "mid115"]
    cases = [CASES[n] for n in names]
    tasks = [ScanTask(bytes(c["nonce"]), 8, 0, 0, c["k_begin"], c["k_end"]) for c in cases]
    t0 = time.perf_counter()
    got = miner.scan_many(tasks)
    dt = time.perf_counter() - t0
    st = miner.last_scan_many_stats
    for c, hits in zip(cases, got):
        for h in hits:
            assert h.secret == _secret_of(h.global_idx)
        assert [(h.global_idx, h.tz) for h in hits] == [(g, tz) for g, tz in c["hits"] if tz >= 8], c["name"]
    assert st.launches == _planned_launches(tasks)
    print(f"{names}: {st.candidates} candidates, {st.launches} launches in {dt * 1e3:.1f} ms ({st.kernel_ms:.1f} ms of kernel)")


def test_cancel_raised_on_entry(miner):
    tasks = [ScanTask([1, 2, 3, 4], 2, 0, 0, 7, 64), ScanTask(b"", 0, 1, 1, 9, 9), ScanTask(_nonce(80), 1, 0, 0, 0, 1 << 30)]
    miner.cancel()
    try:
        got = miner.scan_batch(tasks)
    finally:
        miner.clear_cancel()
    assert got == [(CANCELLED, [], 7), (CANCELLED, [], 9), (CANCELLED, [], 0)]
    assert miner.last_scan_many_stats.launches == 0


def test_cancel_mid_call(miner):
    """One 2^30-k task at N = 32 (partition (9, 4): 2^34 candidates, 64 launches) followed by small
    ones, the flag raised from a thread while the call runs."""
    nonce, k_end, out = [1, 2, 3, 4], 1 << 30, {}
    small = [ScanTask(_nonce(6, j), 1, j, 2, 10 * j, 10 * j + 50) for j in range(1, 4)] + [ScanTask(b"x", 0, 0, 0, 4, 4)]
    tasks = [ScanTask(nonce, 32, 9, 4, 0, k_end)] + small
    miner.scan_many(small)  # (the buffers exist before the clock starts)

    def run():
        out["r"] = miner.scan_batch(tasks)
        out["t_end"] = time.perf_counter()

    th = threading.Thread(target=run)
    th.start()
    time.sleep(0.02)
    t_cancel = time.perf_counter()
    miner.cancel()
    th.join(timeout=30)
    miner.clear_cancel()
    assert not th.is_alive()
    status, hits, k_done = out["r"][0]
    launches = miner.last_scan_many_stats.launches
    print(f"scan_batch cancel latency {(out['t_end'] - t_cancel) * 1e3:.2f} ms at k {k_done}, {launches} launches")
    # the cut task: cancelled at a launch boundary, a whole k; the tasks behind it not begun, the empty one done
    assert status == CANCELLED and hits == [] and 0 <= k_done < k_end and (k_done << 4) % (1 << 28) == 0
    assert launches == (k_done << 4) >> 28
    assert out["r"][1:] == [(CANCELLED, [], t.k_begin) for t in small[:3]] + [(EXHAUSTED, [], 4)]
    # the context goes on: the small tasks, submitted again, are Miner.scan's
    assert miner.scan_many(small) == [_ref_of(t) for t in small]


def test_argument_errors(miner):
    L = distpow.lib()
    nonce = ctypes.create_string_buffer(b"\x01\x02\x03\x04", 4)
    out = (_lib.ScanHitC * 256)()
    n_out = ctypes.c_size_t(77)
    pn = ctypes.byref(n_out)

    def call(nonce_p=ctypes.addressof(nonce), nlen=4, wb=0, k0=0, k1=4, n=1, hits=out, max_hits=256, n_hits=pn, ctx=miner._ctx):
        arr = (_lib.ScanTaskC * 1)()
        c = arr[0]
        c.nonce, c.nonce_len, c.ntz, c.worker_byte, c.worker_bits, c.k_begin, c.k_end = nonce_p, nlen, 1, wb, 0, k0, k1
        c.status, c.k_done = 99, 99
        r = L.dpow_scan_batch(ctx, arr, n, hits, max_hits, n_hits, None)
        return r, c.status, c.k_done, c.first_hit, c.n_hits

    for kw, code in [({"hits": None}, EINVAL), ({"n_hits": None}, EINVAL), ({"n": 0}, EINVAL), ({"n": 4097}, EINVAL),
                     ({"nonce_p": None}, EINVAL), ({"wb": 256}, EINVAL), ({"k0": 5}, EINVAL), ({"max_hits": 255}, EINVAL),
                     ({"nlen": _lib.DPOW_MAX_NONCE + 1}, EINVAL), ({"k1": DPOW_K_LIMIT + 1}, ERANGE), ({"ctx": None}, EINVAL)]:
        assert call(**kw)[:3] == (code, 99, 99), kw
    assert n_out.value == 77
    # only empty tasks: exhausted without a launch; N > 32 hashes and finds nothing
    assert miner.scan_batch([ScanTask(nonce.raw, 1, 0, 0, 9, 9), ScanTask(b"", 0, 3, 2, 0, 0)]) == [(EXHAUSTED, [], 9), (EXHAUSTED, [], 0)]
    assert miner.last_scan_many_stats.launches == 0
    assert miner.scan_batch([ScanTask(nonce.raw, 33, 0, 0, 0, 64)]) == [(EXHAUSTED, [], 64)]
    assert miner.last_scan_many_stats.launches == 1 and miner.last_scan_many_stats.candidates == 64 * 256
    # the context is still usable, and the call leaves dpow_stats alone
    miner.reset_stats()
    r, status, k_done, first, n_hits = call()
    exp = _reference(nonce.raw, 1, 0, 0, 0, 4)
    assert (r, status, k_done, first, n_hits, n_out.value) == (0, EXHAUSTED, 4, 0, len(exp), len(exp))
    assert [(h.global_idx, h.tz) for h in out[:n_out.value]] == [(h.global_idx, h.tz) for h in exp]
    st = miner.stats()
    assert (st.searches, st.launches, st.candidates) == (0, 0, 0)


def test_node_slot_attached_is_refused(miner):
    class Slot(ctypes.Structure):
        """dpow_node_slot (include/dpow.h)."""
        _fields_ = [("best", ctypes.c_uint64), ("stop", ctypes.c_uint32), ("pad", ctypes.c_uint32 * 13)]

    slot = Slot()
    addr = ctypes.addressof(slot)
    distpow.lib().dpow_node_slot_reset(addr)
    miner.attach_node(addr)
    try:
        with pytest.raises(distpow.DpowError) as e:
            miner.scan_many([ScanTask([1, 2, 3, 4], 2, k_end=8)])
        assert e.value.code == EINVAL
    finally:
        miner.attach_node(None)
    assert miner.scan_many([ScanTask([1, 2, 3, 4], 0, k_end=1)])[0][0].global_idx == 0
