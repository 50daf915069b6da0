"""Host side of the batched search (dpow_search_batch), no GPU needed: the candidate words the
generic kernel hashes (dpow_batch_candidate, the kernel's own assembly code) against hashlib, the
round plan and block map (dpow_batch_plan, dpow_batch_plan_block), and the argument errors that
are decided before the device is touched."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import _md5py
import distpow
from distpow import _lib

K_CASES = [0, 1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, 1 << 32, 1 << 40, 1 << 48, (1 << 55) - 2]
CAP = 1 << 28  # candidates per launch (csrc/batch.h kBatchCap)


def _nonce(n, salt=0):
    return bytes((37 * j + 11 + salt) & 0xFF for j in range(n))


def _chunk_len(k):
    return (k.bit_length() + 7) // 8


def test_candidate_words_match_hashlib(oracle):
    """iv and words of dpow_batch_candidate, through a Python MD5 compress, give
    hashlib.md5(nonce || threadByte || chunk_k); nblk is 2 exactly when p + 1 + L > 55."""
    assert sorted({_chunk_len(k) for k in K_CASES}) == list(range(8))
    for wbits in (0, 1, 3, 8, 9):
        rb = 8 - wbits % 9
        wb = (1 << (wbits % 9)) - 1  # the last partition (worker_bits 9: the % 9 quirk, one partition)
        tbs = oracle.thread_bytes(wb, wbits)
        assert len(tbs) == 1 << rb
        for nl in list(range(131)) + [1024]:
            nonce = _nonce(nl, wbits)
            for n, k in enumerate(K_CASES):
                t = (nl + 3 * n) % (1 << rb)
                iv, words, nblk = distpow.batch_candidate(nonce, wb, wbits, (k << rb) | t)
                L = _chunk_len(k)
                assert nblk == (2 if nl % 64 + 1 + L > 55 else 1), (nl, k, wbits)
                st = tuple(iv)
                for b in range(nblk):
                    st = _md5py.compress(st, words[16 * b:16 * b + 16])
                secret = bytes([tbs[t]]) + bytes(oracle.chunk_of(k))
                assert len(secret) == 1 + L
                assert _md5py.digest_from_state(st) == hashlib.md5(nonce + secret).digest(), (nl, k, wbits, t)


def test_candidate_block_count_at_the_55_byte_edge():
    for nl in (52, 53, 54, 55):
        for L, k in ((1, 200), (2, 40000), (3, 1 << 20)):
            _, _, nblk = distpow.batch_candidate(_nonce(nl), 0, 0, k << 8)
            assert nblk == (2 if nl + 1 + L > 55 else 1), (nl, L)


DT = np.dtype([("launch", "<u4"), ("task", "<u4"), ("i_begin", "<u8"), ("i_end", "<u8"), ("group", "<u4"),
               ("rows", "<u4")])


def _check_plan(windows, block_launches=0):
    entries, launches = distpow.batch_plan(windows)
    assert ctypes.sizeof(_lib.BatchRange) == DT.itemsize
    a = np.frombuffer(entries, dtype=DT) if len(entries) else np.zeros(0, dtype=DT)
    # launches are numbered 0, 1, ... in order, every one with at least one entry
    assert (np.diff(a["launch"].astype(np.int64)) >= 0).all()
    assert launches == (int(a["launch"][-1]) + 1 if len(a) else 0)
    assert len(np.unique(a["launch"])) == launches
    # no launch exceeds the cap
    per_launch = np.bincount(a["launch"], weights=(a["i_end"] - a["i_begin"]).astype(np.float64), minlength=1)
    assert per_launch.max(initial=0) <= CAP
    # every task's ranges are increasing, disjoint and cover its window exactly once
    for i, (kb, ke, wbits) in enumerate(windows):
        rb = 8 - wbits % 9
        mine = a[a["task"] == i]
        if kb == ke:
            assert len(mine) == 0
            continue
        assert int(mine["i_begin"][0]) == kb << rb and int(mine["i_end"][-1]) == ke << rb
        assert (mine["i_begin"][1:] == mine["i_end"][:-1]).all()
        assert (mine["i_end"] > mine["i_begin"]).all()
        assert (np.diff(mine["launch"].astype(np.int64)) == 1).all()  # one slice per round until it ends
    # slices fit the launch's grid: rows * group covers the longest slice of the launch
    assert ((a["i_end"] - a["i_begin"]) <= a["rows"].astype(np.uint64) * a["group"].astype(np.uint64)).all()
    # the block map of the first launches, workgroup by workgroup (the kernel's own arithmetic)
    for launch in range(min(block_launches, launches)):
        idx = np.nonzero(a["launch"] == launch)[0]
        first, n_live = int(idx[0]), len(idx)
        ent = (_lib.BatchRange * n_live).from_buffer(entries, first * DT.itemsize)
        rows, group = int(a["rows"][first]), int(a["group"][first])
        assert (a["rows"][idx] == rows).all() and (a["group"][idx] == group).all()
        at = {int(a["task"][j]): int(a["i_begin"][j]) for j in idx}   # next expected lo per task
        begin = dict(at)
        last_group = 0
        for b in range(rows * n_live):
            r = distpow.batch_plan_block(ent, n_live, b)
            if r is None:
                continue
            task, lo, hi = r
            assert lo == at[task] and lo < hi <= lo + group
            at[task] = hi
            c = (lo - begin[task]) // group
            assert c >= last_group       # group c of every task before group c + 1 of any
            last_group = c
        for j in idx:
            assert at[int(a["task"][j])] == int(a["i_end"][j])  # the slice is covered exactly once
    return a, launches


def test_round_plan_random_windows():
    rnd = random.Random(20240611)
    for case in range(12):
        n = rnd.choice([1, 2, 3, 17, 64, 300])
        windows = []
        for _ in range(n):
            kb = rnd.choice([0, 1, 255, 65530, rnd.randrange(1 << 30), (1 << 40) - 3])
            ke = kb + rnd.choice([0, 0, 1, 7, 64, 1000, rnd.randrange(1 << 14), rnd.randrange(1 << 20)])
            windows.append((kb, ke, rnd.choice([0, 0, 1, 2, 3, 8, 9])))
        _check_plan(windows, block_launches=2)


def test_round_plan_slices_grow_geometrically():
    a, launches = _check_plan([(0, 1 << 22, 0)], block_launches=1)
    sizes = (a["i_end"] - a["i_begin"]).astype(np.int64)
    assert launches >= 4 and sizes[0] == 1 << 20
    assert (sizes[1:-1] == np.minimum(sizes[:-2] * 4, CAP)).all()


def test_round_plan_one_long_task_among_short():
    windows = [(0, 16, 0), (5, 5, 0), (1 << 24, (1 << 24) + (1 << 40), 0), (100, 4000, 3), (7, 8, 9)]
    a, launches = _check_plan(windows, block_launches=3)
    long_ = a[a["task"] == 2]
    assert int((long_["i_end"] - long_["i_begin"]).sum()) == 1 << 48
    assert launches == len(long_) >= (1 << 48) // CAP


def test_all_empty_windows_plan_nothing():
    entries, launches = distpow.batch_plan([(3, 3, 0), (0, 0, 2)])
    assert len(entries) == 0 and launches == 0


def _tasks(specs):
    """dpow_batch_task array from (nonce, ntz, wb, wbits, kb, ke) tuples; status preset to 77."""
    arr = (_lib.BatchTaskC * max(len(specs), 1))()
    keep = []
    for c, (nonce, ntz, wb, wbits, kb, ke) in zip(arr, specs):
        buf = (ctypes.c_uint8 * max(len(nonce), 1)).from_buffer_copy(bytes(nonce) or b"\0")
        keep.append(buf)
        c.nonce = ctypes.addressof(buf)
        c.nonce_len = len(nonce)
        c.ntz, c.worker_byte, c.worker_bits, c.k_begin, c.k_end = ntz, wb, wbits, kb, ke
        c.best_global_idx = distpow.DPOW_NO_HIT
        c.status = 77
    return arr, keep


def test_argument_errors_before_any_gpu_work():
    """The tasks' own errors are decided before the context is looked at, so they show without
    one: a window past DPOW_K_LIMIT is DPOW_ERANGE (not the NULL context's DPOW_EINVAL), every
    other bad argument DPOW_EINVAL, and no task is written."""
    L = distpow.lib()
    ok = ([1, 2, 3, 4], 3, 0, 0, 0, 8)
    arr, keep = _tasks([ok, ([1], 2, 0, 0, 0, distpow.DPOW_K_LIMIT + 1)])
    assert L.dpow_search_batch(None, arr, 2, None) == distpow.ERANGE
    assert "DPOW_K_LIMIT" in _lib.last_error()
    assert [c.status for c in arr] == [77, 77]
    bad = {
        "k_begin > k_end": ([1], 2, 0, 0, 9, 8),
        "DPOW_MAX_NONCE": (bytes(1025), 2, 0, 0, 0, 8),
        "worker_byte": ([1], 2, 256, 0, 0, 8),
    }
    for text, spec in bad.items():
        arr, keep = _tasks([ok, spec])
        assert L.dpow_search_batch(None, arr, 2, None) == distpow.EINVAL
        assert text in _lib.last_error(), _lib.last_error()
        assert [c.status for c in arr] == [77, 77]
    arr, keep = _tasks([ok])
    arr[0].nonce = None                                      # nonce_len 4 with a NULL nonce
    assert L.dpow_search_batch(None, arr, 1, None) == distpow.EINVAL and "nonce is NULL" in _lib.last_error()
    arr, keep = _tasks([ok])
    assert L.dpow_search_batch(None, arr, 0, None) == distpow.EINVAL and "n_tasks" in _lib.last_error()
    assert L.dpow_search_batch(None, arr, _lib.DPOW_BATCH_MAX + 1, None) == distpow.EINVAL
    assert "n_tasks" in _lib.last_error()
    assert L.dpow_search_batch(None, None, 1, None) == distpow.EINVAL and "tasks is NULL" in _lib.last_error()
    # a good batch without a context: the context's own error, still nothing written
    assert L.dpow_search_batch(None, arr, 1, None) == distpow.EINVAL and "ctx is NULL" in _lib.last_error()
    assert arr[0].status == 77
    # a nonce of exactly DPOW_MAX_NONCE bytes and a window up to DPOW_K_LIMIT are legal
    arr, keep = _tasks([(bytes(1024), 2, 255, 8, distpow.DPOW_K_LIMIT - 1, distpow.DPOW_K_LIMIT)])
    assert L.dpow_search_batch(None, arr, 1, None) == distpow.EINVAL and "ctx is NULL" in _lib.last_error()


def test_plan_and_candidate_argument_errors():
    with pytest.raises(distpow.DpowError) as e:
        distpow.batch_plan([(9, 8, 0)])
    assert e.value.code == distpow.EINVAL
    with pytest.raises(distpow.DpowError) as e:
        distpow.batch_plan([(0, distpow.DPOW_K_LIMIT + 1, 0)])
    assert e.value.code == distpow.ERANGE
    with pytest.raises(distpow.DpowError) as e:
        distpow.batch_plan([])
    assert e.value.code == distpow.EINVAL
    with pytest.raises(distpow.DpowError) as e:
        distpow.batch_candidate(bytes(1025), 0, 0, 0)
    assert e.value.code == distpow.EINVAL
    with pytest.raises(distpow.DpowError) as e:
        distpow.batch_candidate(b"", 0, 0, distpow.DPOW_K_LIMIT << 8)
    assert e.value.code == distpow.ERANGE


def test_python_binding_lists_the_batch_entry_points():
    L = distpow.lib()
    for name in ("dpow_search_batch", "dpow_batch_candidate", "dpow_batch_plan", "dpow_batch_plan_block"):
        assert getattr(L, name).argtypes is not None
    assert ctypes.sizeof(_lib.BatchTaskC) == 80 and ctypes.sizeof(_lib.BatchStats) == 24
    assert distpow.BatchTask([1], 2).k_end == 1 and distpow.BatchTask([1], 2).bound == distpow.DPOW_NO_HIT
