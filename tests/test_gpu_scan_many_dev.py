"""GPU: the batched device scan (dpow_scan_batch_device, Miner.scan_batch_cuda, Miner.scan_many_cuda)
-- the hits of many windows in one call, task after task in increasing global index, left in GPU
memory with their row pointers.

Every expectation comes from something that is not this call: a Python loop over hashlib (computed
once per module and shared), Miner.scan_many, Miner.scan_cuda and Miner.digests_cuda, each pinned by
tests of its own, and the CPU restatement of the paging contract (_scan_many_dev_model.call_model).

Each test prints its time (pytest -s).
"""
import ctypes
import hashlib
import random
import time

import pytest

import distpow
from distpow import CANCELLED, EINVAL, EXHAUSTED, MORE, ScanTask
from distpow import _lib
from _scan_many_dev_model import call_model, launches_of, windows_of

pytestmark = pytest.mark.gpu

MIN_HITS = 16384


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


def _reference(t):
    """The reference's enumeration (k outer, threadByte inner) with hashlib: ([global index], [depth])."""
    base, tbs, idx, dep = hashlib.md5(bytes(t.nonce)), _thread_bytes(t.worker_byte, t.worker_bits), [], []
    for k in range(t.k_begin, t.k_end):
        for tb in tbs:
            h = base.copy()
            h.update(_secret_of(k << 8 | tb))
            hx = h.hexdigest()
            tz = 32 - len(hx.rstrip("0"))
            if tz >= t.num_trailing_zeros:
                idx.append(k << 8 | tb)
                dep.append(tz)
    return idx, dep


def _nonce(n, salt=0):
    rnd = random.Random(1000 * n + salt)
    return bytes(rnd.randrange(256) for _ in range(n))


def _grid_tasks():
    """41 tasks: nonce lengths on both sides of the one/two final block change, depths from all to
    none, three partition widths with non-zero worker bytes, windows of 1 to 1000 k that start at 0,
    just below the chunk-length changes at k = 2^8 and 2^16 and elsewhere, empty tasks first, in the
    middle and last, and a duplicated task."""
    lens, depths, parts = (0, 4, 55, 56, 63), (0, 1, 2, 3, 33), ((0, 0), (5, 3), (200, 8))
    starts, spans = (0, 250, 65530, 3), (1, 7, 1000, 40, 13, 300, 2)
    tasks = []
    for j in range(36):
        wb, wbits = parts[j % 3]
        k0 = starts[j % 4]
        tasks.append(ScanTask(_nonce(lens[j % 5], j), depths[(j // 5 + j) % 5], wb, wbits, k0, k0 + spans[j % 7]))
    dup = tasks[18]  # 13 k of 256 candidates at N = 1
    tasks.insert(0, ScanTask(_nonce(4), 1, 0, 0, 9, 9))
    tasks.insert(17, ScanTask(_nonce(56), 0, 3, 3, 70000, 70000))
    tasks.insert(18, ScanTask(b"", 2, 0, 0, 0, 0))
    tasks.append(dup)
    tasks.append(ScanTask(_nonce(63), 0, 255, 8, 77, 77))
    return tasks


@pytest.fixture(scope="module")
def grid():
    tasks = _grid_tasks()
    t0 = time.perf_counter()
    ref = [_reference(t) for t in tasks]
    print(f"hashlib grid: {len(tasks)} tasks, {sum(len(i) for i, _ in ref)} hits in {time.perf_counter() - t0:.1f} s")
    assert len(tasks) == 41 and {len(t.nonce) for t in tasks} == {0, 4, 55, 56, 63}
    assert {t.num_trailing_zeros for t in tasks} == {0, 1, 2, 3, 33} and {t.worker_bits for t in tasks} == {0, 3, 8}
    assert any(t.k_begin < 256 < t.k_end for t in tasks) and any(t.k_begin < 65536 < t.k_end for t in tasks)
    return tasks, ref


def _rows_of(ref):
    rows = [0]
    for idx, _ in ref:
        rows.append(rows[-1] + len(idx))
    return rows


def _check_call(miner, tasks, ref, out, want_depths=True):
    res, idx, dep, rows = out
    exp_rows = _rows_of(ref)
    assert res == [(EXHAUSTED, t.k_end) for t in tasks]
    assert miner.last_scan_many_device_rows == exp_rows
    if rows is not None:
        assert rows.tolist() == exp_rows
    got_idx = idx.tolist()
    got_dep = dep.tolist() if want_depths else None
    assert len(got_idx) == exp_rows[-1]
    for j, (e_idx, e_dep) in enumerate(ref):
        assert got_idx[exp_rows[j]:exp_rows[j + 1]] == e_idx, (j, tasks[j])
        if want_depths:
            assert got_dep[exp_rows[j]:exp_rows[j + 1]] == e_dep, (j, tasks[j])


def test_readme_tasks(miner):
    tasks = [ScanTask([1, 2, 3, 4], 6, k_end=1 << 16), ScanTask([5, 6, 7, 8], 2, 5, 3, 0, 100)]
    exp = miner.scan_many(tasks)
    t0 = time.perf_counter()
    idx, dep, rows = miner.scan_many_cuda(tasks)
    dt = time.perf_counter() - t0
    assert rows.tolist() == [0, len(exp[0]), len(exp[0]) + len(exp[1])] and sum(map(len, exp)) > 0
    assert idx.tolist() == [h.global_idx for hs in exp for h in hs]
    assert dep.tolist() == [h.tz for hs in exp for h in hs]
    print(f"README tasks: {idx.numel()} hits in {dt * 1e3:.2f} ms")


def test_hashlib_grid_in_one_call(miner, grid):
    tasks, ref = grid
    assert len(launches_of(windows_of(tasks))) == 1
    t0 = time.perf_counter()
    out = miner.scan_batch_cuda(tasks)
    dt = time.perf_counter() - t0
    st = miner.last_scan_many_device_stats
    _check_call(miner, tasks, ref, out)
    assert st.rounds == 1 and st.launches == 5   # mask, rows, place, depth, the last rows launch
    assert st.candidates == sum((t.k_end - t.k_begin) << (8 - t.worker_bits % 9) for t in tasks)
    print(f"grid: {out[1].numel()} hits of {st.candidates} candidates in {dt * 1e3:.2f} ms, kernels {st.kernel_ms:.3f} ms")


@pytest.mark.parametrize("cap", [256, 4096])
def test_launch_seams_change_nothing(miner, grid, monkeypatch, cap):
    """The diagnostic budget cuts tasks across launches: a task's row is written by an earlier launch
    than its last hit, and the list is placed piece by piece."""
    tasks, ref = grid
    n_launches = len(launches_of(windows_of(tasks), cap))
    assert n_launches > len(tasks)
    monkeypatch.setenv("DPOW_DIAG_SCAN_MANY_DEV_CAP", str(cap))
    t0 = time.perf_counter()
    out = miner.scan_batch_cuda(tasks)
    dt = time.perf_counter() - t0
    assert miner.last_scan_many_device_stats.rounds == n_launches
    _check_call(miner, tasks, ref, out)
    if cap == 4096:  # no depths, no caller's rows: the answer through the task structs
        out = miner.scan_batch_cuda(tasks, want_depths=False, want_rows=False)
        assert out[2] is None and out[3] is None
        _check_call(miner, tasks, ref, out, want_depths=False)
    print(f"cap {cap}: {n_launches} launches in {dt * 1e3:.1f} ms")


@pytest.mark.parametrize("n_tasks", [2049, 4096])
def test_more_than_one_round_of_totals(miner, n_tasks):
    """One ragged descriptor per task (256 candidates each), more descriptors than one round of 2048
    totals of the last workgroup's prefix; 4096 is the most tasks of a call."""
    tasks = [ScanTask(j.to_bytes(4, "little"), 1, 0, 0, j % 300, j % 300 + 1) for j in range(n_tasks)]
    assert len(launches_of(windows_of(tasks))) == 1
    ref = [_reference(t) for t in tasks]
    t0 = time.perf_counter()
    out = miner.scan_batch_cuda(tasks)
    dt = time.perf_counter() - t0
    _check_call(miner, tasks, ref, out)
    print(f"{n_tasks} tasks of 256: {out[1].numel()} hits in {dt * 1e3:.2f} ms")


@pytest.mark.parametrize("case", ["16384x300", "whole-and-ragged"])
def test_one_large_task_against_scan_cuda(miner, case):
    """16384 x 300 local indices at N = 2; and a task of more than 2^26 local indices that no power of
    two divides, whose descriptors are 16384 long but for the last."""
    import torch
    if case == "16384x300":
        t = ScanTask([1, 2, 3, 4], 2, 0, 0, 0, 16384 * 300 // 256)
    else:
        t = ScanTask(_nonce(56, 3), 2, 77, 8, 3, 3 + (1 << 26) + 2 * 16384 + 777)
        blocks = launches_of(windows_of([t]))[0]
        assert blocks[0][2] - blocks[0][1] == 16384 and 0 < blocks[-1][2] - blocks[-1][1] < 16384
    e_idx, e_dep = miner.scan_cuda(t.nonce, t.num_trailing_zeros, t.worker_byte, t.worker_bits, t.k_begin, t.k_end)
    t0 = time.perf_counter()
    res, idx, dep, rows = miner.scan_batch_cuda([t])
    dt = time.perf_counter() - t0
    assert res == [(EXHAUSTED, t.k_end)] and rows.tolist() == [0, e_idx.numel()] and e_idx.numel() > 1000
    assert torch.equal(idx, e_idx) and torch.equal(dep, e_dep)
    print(f"{case}: {idx.numel()} hits in {dt * 1e3:.2f} ms")


def test_stale_bitmap_is_never_read():
    """A dense call leaves every word of its descriptors' slots set; the sparse, shorter, ragged call
    behind it on the same context must read none of them."""
    dense = [ScanTask(_nonce(4, 1), 0, 0, 0, 0, 64)]
    sparse = [ScanTask(_nonce(55, 2), 3, 5, 3, 0, 301), ScanTask(_nonce(4, 3), 3, 0, 0, 2, 5)]
    ref = [_reference(t) for t in sparse]
    with distpow.Miner(0) as m:
        res, idx, _, _ = m.scan_batch_cuda(dense)
        assert idx.numel() == 16384 and idx.tolist() == list(range(16384))
        _check_call(m, sparse, ref, m.scan_batch_cuda(sparse))


def _dense_ref(t):
    idx = [k << 8 | tb for k in range(t.k_begin, t.k_end) for tb in _thread_bytes(t.worker_byte, t.worker_bits)]
    return idx


PAGING = {
    # about 3 x 16384 hits, cuts inside tasks, an empty task among them
    "inside": [ScanTask(_nonce(4, 5), 0, 0, 0, 0, 30), ScanTask(_nonce(9), 0, 0, 0, 4, 4), ScanTask(_nonce(4, 6), 0, 0, 0, 5, 45),
               ScanTask(_nonce(56, 7), 0, 3, 3, 0, 500), ScanTask(_nonce(63, 8), 0, 0, 0, 100, 160)],
    # the first task is exactly one page: the cut falls on the first descriptor of the task behind it
    "boundary": [ScanTask(_nonce(4, 5), 0, 0, 0, 7, 71), ScanTask(_nonce(4, 6), 0, 0, 0, 0, 40),
                 ScanTask(_nonce(9), 0, 0, 0, 4, 4), ScanTask(_nonce(63, 8), 0, 0, 0, 100, 190)],
}


@pytest.mark.parametrize("layout", sorted(PAGING))
def test_paging_follows_the_restatement(miner, layout):
    tasks = PAGING[layout]
    full = [_dense_ref(t) for t in tasks]
    assert 2.5 * MIN_HITS < sum(map(len, full)) < 3.5 * MIN_HITS
    k = [t.k_begin for t in tasks]
    got = [[] for _ in tasks]
    calls = 0
    while True:
        page = [ScanTask(t.nonce, 0, t.worker_byte, t.worker_bits, k[i], t.k_end) for i, t in enumerate(tasks)]
        rest = [[g for g in full[i] if (g >> 8) >= k[i]] for i in range(len(tasks))]
        e_res, e_rows, e_seg = call_model(page, rest, MIN_HITS)
        res, idx, dep, rows = miner.scan_batch_cuda(page, max_hits=MIN_HITS)
        calls += 1
        assert res == e_res and rows.tolist() == e_rows == miner.last_scan_many_device_rows, (layout, calls)
        assert idx.tolist() == [g for s in e_seg for g in s]
        if layout == "boundary" and calls == 1:
            assert res[0] == (EXHAUSTED, 71) and res[1] == (MORE, 0) and rows.tolist() == [0, 16384, 16384, 16384, 16384]
        flat = idx.tolist()
        for i in range(len(tasks)):
            got[i] += flat[e_rows[i]:e_rows[i + 1]]
            k[i] = res[i][1]
        assert calls < 10
        if all(r == EXHAUSTED for r, _ in res):
            break
    assert got == full and calls >= 3
    # the paging wrapper gives the unpaged list
    idx, dep, rows = miner.scan_many_cuda(tasks, max_hits=MIN_HITS)
    assert idx.tolist() == [g for s in full for g in s] and rows.tolist() == _rows_of([(s, None) for s in full])
    one = miner.scan_many_cuda(tasks)
    assert one[0].tolist() == idx.tolist() and one[1].tolist() == dep.tolist() and one[2].tolist() == rows.tolist()


def _raw_call(miner, tasks, idx, max_hits):
    arr = (_lib.ScanTaskC * len(tasks))()
    keep = [ctypes.create_string_buffer(bytes(t.nonce), max(len(t.nonce), 1)) for t in tasks]
    for c, t, b in zip(arr, tasks, keep):
        c.nonce, c.nonce_len, c.ntz, c.worker_byte, c.worker_bits = ctypes.addressof(b), len(t.nonce), t.num_trailing_zeros, t.worker_byte, t.worker_bits
        c.k_begin, c.k_end, c.k_done, c.status, c.first_hit, c.n_hits = t.k_begin, t.k_end, 66, 55, 77, 88
    n_out, st = ctypes.c_size_t(99), _lib.BatchStats()
    rc = distpow.lib().dpow_scan_batch_device(miner._ctx, arr, len(tasks), idx.data_ptr(), None, None, max_hits,
                                              ctypes.byref(n_out), ctypes.byref(st))
    return rc, arr, n_out.value, st


def test_room_below_one_descriptor_is_refused(miner):
    import torch
    idx = torch.full((MIN_HITS,), -1, dtype=torch.int64, device=torch.device("cuda", miner.device))
    rc, arr, n_out, st = _raw_call(miner, PAGING["inside"], idx, MIN_HITS - 1)
    assert rc == EINVAL and n_out == 99 and st.launches == 0
    assert all((c.status, c.k_done, c.first_hit, c.n_hits) == (55, 66, 77, 88) for c in arr)
    assert bool((idx == -1).all())


def test_cancel_raised_on_entry(miner):
    tasks = PAGING["inside"]
    miner.cancel()
    try:
        res, idx, dep, rows = miner.scan_batch_cuda(tasks)
    finally:
        miner.clear_cancel()
    assert res == [(CANCELLED, t.k_begin) for t in tasks] and idx.numel() == 0 and dep.numel() == 0
    assert rows.tolist() == [0] * (len(tasks) + 1)
    assert miner.last_scan_many_device_stats.launches == 0


def test_only_empty_tasks_make_no_launch(miner):
    tasks = [ScanTask(_nonce(4), 1, 0, 0, 9, 9), ScanTask(b"", 0, 255, 8, 0, 0)]
    res, idx, dep, rows = miner.scan_batch_cuda(tasks)
    assert res == [(EXHAUSTED, 9), (EXHAUSTED, 0)] and idx.numel() == 0 and rows.tolist() == [0, 0, 0]
    assert miner.last_scan_many_device_stats.launches == 0


def test_composition_with_digests_cuda(miner):
    """The list goes on to dpow_digests_device without leaving the GPU: the depths it computes for a
    task's segment are the ones the call wrote."""
    import torch
    tasks = [ScanTask(_nonce(55, 1), 1, 0, 0, 250, 300), ScanTask(_nonce(63, 2), 2, 3, 2, 65530, 65600),
             ScanTask(_nonce(4, 3), 0, 9, 4, 0, 40)]
    res, idx, dep, rows = miner.scan_batch_cuda(tasks)
    r = rows.tolist()
    assert all(r[i + 1] > r[i] for i in range(3))
    for i, t in enumerate(tasks):
        _, d = miner.digests_cuda(t.nonce, idx[r[i]:r[i + 1]])
        assert torch.equal(d, dep[r[i]:r[i + 1]]), i
