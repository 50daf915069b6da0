"""Host side of the batched census (dpow_census_batch), no GPU needed: the launch planner
(dpow_census_plan, the function the call's own loop steps through) and the argument errors that are
decided before the device is touched.

The planner's rules (include/dpow.h): a launch takes tasks in array order until
it holds `cap` local indices; only its last task can be cut, at a multiple of 256 local indices from
the task's begin; a task's part of a launch is cut into descriptors of batch_group(the launch's
total), the last one possibly shorter; an empty task has no descriptor."""
import ctypes
import random

import numpy as np
import pytest

import distpow
from distpow import DPOW_K_LIMIT, EINVAL, ERANGE, _lib

CAP = 1 << 28            # local indices per launch (csrc/batch.h kBatchCap)
BLOCKS = 4096            # workgroups a launch aims for (kBatchBlocks)
MIN_GROUP, MAX_GROUP = 256, 16384  # kBatchMinGroup, kBatchMaxGroup
MAX_BLOCKS = _lib.CENSUS_MANY_MAX_BLOCKS

DT = np.dtype([("launch", "<u4"), ("task", "<u4"), ("i_begin", "<u8"), ("i_end", "<u8"), ("group", "<u4"),
               ("rows", "<u4")])


def _batch_group(total):
    """csrc/batch.cpp batch_group."""
    q = total // BLOCKS
    return min(max(1 << (q.bit_length() - 1) if q else 0, MIN_GROUP), MAX_GROUP)


def test_the_descriptor_bound_is_the_one_stated():
    """Whole descriptors: fewer than 8192 below the largest group, cap / 16384 at it; one partial per task."""
    assert MAX_BLOCKS == CAP // MAX_GROUP + _lib.DPOW_BATCH_MAX == 20480
    for total in (1, 255, 256, (1 << 21) - 1, 1 << 21, (1 << 26) - 1, 1 << 26, CAP - 1, CAP):
        assert total // _batch_group(total) <= CAP // MAX_GROUP


def _check_plan(windows, cap=0):
    """Every rule on the plan of `windows` = [(k_begin, k_end, worker_bits)]; returns (entries, launches)."""
    entries, launches = distpow.census_plan(windows, cap)
    assert ctypes.sizeof(_lib.BatchRange) == DT.itemsize
    a = np.frombuffer(entries, dtype=DT) if len(entries) else np.zeros(0, dtype=DT)
    budget = (cap or CAP) & ~255
    rb = [8 - w[2] % 9 for w in windows]
    ib = np.array([w[0] << r for w, r in zip(windows, rb)], dtype=np.uint64)
    ie = np.array([w[1] << r for w, r in zip(windows, rb)], dtype=np.uint64)
    live = [i for i in range(len(windows)) if ib[i] < ie[i]]
    if not live:
        assert len(a) == 0 and launches == 0
        return a, launches
    launch, task = a["launch"].astype(np.int64), a["task"].astype(np.int64)
    lo, hi = a["i_begin"], a["i_end"]
    size = (hi - lo).astype(np.int64)
    assert (hi > lo).all()
    # launches are numbered 0, 1, ... in order, and take tasks in array order
    assert launch[0] == 0 and set(np.diff(launch)) <= {0, 1} and launches == launch[-1] + 1
    assert (np.diff(task) >= 0).all()
    # exactly the non-empty tasks appear, and a task's descriptors tile its range once, in order
    assert sorted(set(task.tolist())) == live
    same = task[1:] == task[:-1]
    assert (lo[1:][same] == hi[:-1][same]).all()
    first = np.concatenate(([True], ~same))
    last = np.concatenate((~same, [True]))
    assert (lo[first] == ib[task[first]]).all() and (hi[last] == ie[task[last]]).all()
    # a cut between launches: inside a task only, at a multiple of 256 from the task's begin
    seam = launch[1:] != launch[:-1]
    cut = seam & same
    assert ((hi[:-1][cut] - ib[task[:-1][cut]]) % 256 == 0).all()
    # (a launch whose last task is not cut ended it: the tiling above says so)
    # per launch: the budget, the group, the descriptor bound
    starts = np.flatnonzero(np.concatenate(([True], seam)))
    ends = np.concatenate((starts[1:], [len(a)]))
    assert (size <= MAX_GROUP).all()
    for n, (s, e) in enumerate(zip(starts, ends)):
        total = int(size[s:e].sum())
        assert total <= budget, (n, total)
        assert e - s <= MAX_BLOCKS, (n, e - s)
        group = _batch_group(total)
        assert (a["group"][s:e] == group).all(), (n, group)
        assert (size[s:e] <= group).all()
        # every descriptor of a task's part but its last is a whole group; rows counts the part's
        part_last = np.concatenate((task[s + 1:e] != task[s:e - 1], [True]))
        assert (size[s:e][~part_last] == group).all()
        t_l, cnt = np.unique(task[s:e], return_counts=True)
        rows = dict(zip(t_l.tolist(), cnt.tolist()))
        assert a["rows"][s:e].tolist() == [rows[t] for t in task[s:e].tolist()]
        # greedy fill: a launch that is not the last had no room for 256 more local indices
        if n + 1 < launches:
            assert budget - total < 256, (n, total)
    return a, launches


def test_a_single_task_is_the_census_loop():
    """census.cpp's loop: 2^28 local indices per launch from the window's begin, batch_group of the launch."""
    for k0, k1, wbits in [(0, 1, 0), (3, 4, 8), (7, (1 << 21) + 12345, 0), (5, (1 << 30) + 77, 8), (1, 1 << 25, 3),
                          (1 << 24, (1 << 24) + (1 << 21) + 1, 0)]:
        a, launches = _check_plan([(k0, k1, wbits)])
        rb = 8 - wbits % 9
        lo, end, n = k0 << rb, k1 << rb, 0
        while lo < end:
            hi = min(lo + CAP, end)
            mine = a[a["launch"] == n]
            group = _batch_group(hi - lo)
            assert (int(mine["i_begin"][0]), int(mine["i_end"][-1])) == (lo, hi)
            assert len(mine) == (hi - lo + group - 1) // group and (mine["group"] == group).all()
            lo, n = hi, n + 1
        assert n == launches


@pytest.mark.parametrize("cap", [256, 1 << 20, 0])
def test_mixed_windows_in_one_call(cap):
    """1 k to 2^30 k, the three partition widths, empty tasks in the middle, B up to 4096."""
    rnd = random.Random(cap + 1)
    biggest = {256: 10, 1 << 20: 19, 0: 30}[cap]  # log2 of the largest window in k: the plan stays a few 10^5 entries
    for B in (1, 2, 3, 17, 256, 4096):
        windows = []
        for j in range(B):
            wbits = rnd.choice((0, 3, 8))
            # the largest windows at one candidate per k; others shrink with the partition's width
            top = biggest if wbits == 8 else max(biggest - (8 - wbits % 9) - 2, 0)
            if B >= 256:
                top = min(top, 12)
            k0 = rnd.choice((0, 1, 3, 255, 65530, 1 << 24))
            n_k = 0 if rnd.random() < 0.15 else rnd.choice((1, 2, 255, 256, 257, rnd.randrange(1, (1 << top) + 1),
                                                            1 << top))
            windows.append((k0, k0 + n_k, wbits))
        if B >= 3:
            windows[B // 2] = (9, 9, 0)  # an empty task in the middle
        windows[rnd.randrange(B)] = (5, 5 + (1 << (biggest if B < 256 else 12)), 8)
        a, launches = _check_plan(windows, cap)
        print(f"cap {cap or CAP} B {B}: {len(a)} descriptors in {launches} launches")
        assert launches >= 1


def test_4096_one_k_tasks_fill_one_launch():
    a, launches = _check_plan([(j, j + 1, 8) for j in range(4096)])
    assert launches == 1 and len(a) == 4096 and (a["group"] == 256).all()
    a, launches = _check_plan([(j, j + 1, 0) for j in range(4096)])  # 256 candidates each
    assert launches == 1 and len(a) == 4096 and (a["i_end"] - a["i_begin"] == 256).all()
    # the descriptor bound is met with 4096 tasks that each end in a partial descriptor
    a, launches = _check_plan([(0, 65537, 8)] * 4095 + [(0, 1 << 20, 8)])
    assert launches == 2 and (a["launch"] == 0).sum() == 4095 * 5 + 4 == 20479 <= MAX_BLOCKS


def test_only_empty_tasks_plan_nothing():
    a, launches = _check_plan([(4, 4, 0), (0, 0, 8), (DPOW_K_LIMIT, DPOW_K_LIMIT, 3)])
    assert len(a) == 0 and launches == 0


def test_seams_of_the_gpu_test():
    """tests/test_gpu_census_many.py's seam case: cap 4096, partition width 32 per k."""
    windows = [(0, n, 3) for n in (1000, 5000, 256, 12288, 3)]
    a, launches = _check_plan(windows, 4096)
    total = sum(n * 32 for _, n, _ in windows)
    assert launches == (total + 4095) // 4096  # every launch but the last is full: all sizes are multiples of 32
    per_launch = [len(set(a["task"][a["launch"] == n].tolist())) for n in range(launches)]
    # Only the 3-k task is shorter than a launch and it comes last, so a launch holds two tasks at
    # most here; four of the five tasks are cut, each at many launch boundaries.
    assert max(per_launch) == 2 and per_launch.count(2) == 4
    # Its second call: launches that hold three and four tasks.
    a, launches = _check_plan([(0, n, 3) for n in (100, 3, 2, 200, 1, 130)], 4096)
    per_launch = [len(set(a["task"][a["launch"] == n].tolist())) for n in range(launches)]
    assert per_launch == [4, 1, 3, 1]


def test_plan_argument_errors():
    L = distpow.lib()
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    n_l = u64()

    def call(kb=(0,), ke=(4,), wb=(0,), n=1, cap=0, launches=ctypes.byref(n_l)):
        return L.dpow_census_plan((u64 * len(kb))(*kb), (u64 * len(ke))(*ke), (u32 * len(wb))(*wb), n, cap, None, 0,
                                  launches)

    assert call() == 4 and n_l.value == 1  # 1024 local indices: four descriptors of 256 in one launch
    assert call(launches=None) == EINVAL
    assert call(n=0) == EINVAL
    assert call(kb=(0,) * 4097, ke=(1,) * 4097, wb=(0,) * 4097, n=4097) == EINVAL
    assert call(kb=(5,)) == EINVAL
    assert call(ke=(DPOW_K_LIMIT + 1,)) == ERANGE
    assert call(cap=255) == EINVAL and call(cap=CAP + 1) == EINVAL
    assert call(cap=511) == 4 and n_l.value == 4  # rounded down to a multiple of 256: four launches of one
    assert L.dpow_census_plan(None, None, None, 1, 0, None, 0, ctypes.byref(n_l)) == EINVAL


def _tasks(specs):
    """A dpow_census_task array for [(nonce bytes or None, nonce_len, worker_byte, worker_bits, k_begin, k_end)]
    with every output byte set to 0xA5, and what keeps its nonces alive."""
    arr = (_lib.CensusTaskC * len(specs))()
    ctypes.memset(arr, 0xA5, ctypes.sizeof(arr))
    keep = []
    for c, (nonce, nlen, wb, wbits, k0, k1) in zip(arr, specs):
        buf = ctypes.create_string_buffer(nonce, max(len(nonce), 1)) if nonce is not None else None
        keep.append(buf)
        c.nonce = ctypes.addressof(buf) if buf is not None else None
        c.nonce_len, c.worker_byte, c.worker_bits, c.k_begin, c.k_end = nlen, wb, wbits, k0, k1
    return arr, keep


GOOD = (b"\x01\x02\x03\x04", 4, 0, 0, 0, 4)


@pytest.mark.parametrize("bad, code", [
    ((b"\x01\x02\x03\x04", 4, 256, 0, 0, 4), EINVAL),                       # worker_byte > 255
    ((b"\x01\x02\x03\x04", 4, 0, 0, 5, 4), EINVAL),                         # k_begin > k_end
    ((bytes(_lib.DPOW_MAX_NONCE + 1), _lib.DPOW_MAX_NONCE + 1, 0, 0, 0, 4), EINVAL),  # nonce too long
    ((None, 4, 0, 0, 0, 4), EINVAL),                                        # NULL nonce with a length
    ((b"\x01\x02\x03\x04", 4, 0, 0, 0, DPOW_K_LIMIT + 1), ERANGE),          # k_end beyond DPOW_K_LIMIT
], ids=["worker_byte", "k_order", "nonce_len", "nonce_null", "k_limit"])
@pytest.mark.parametrize("where", [0, 2])
def test_argument_errors_leave_the_tasks_untouched(bad, code, where):
    """The tasks' own errors come before the context's: a NULL context reaches every one of them."""
    specs = [GOOD, GOOD, GOOD]
    specs[where] = bad
    arr, keep = _tasks(specs)
    before = ctypes.string_at(arr, ctypes.sizeof(arr))
    st = _lib.BatchStats(7, 7, 7, 7.0)
    assert distpow.lib().dpow_census_batch(None, arr, 3, ctypes.byref(st)) == code
    assert ctypes.string_at(arr, ctypes.sizeof(arr)) == before
    assert (st.launches, st.candidates) == (7, 7)
    del keep


def test_call_argument_errors():
    L = distpow.lib()
    arr, keep = _tasks([GOOD])
    before = ctypes.string_at(arr, ctypes.sizeof(arr))
    assert L.dpow_census_batch(None, None, 1, None) == EINVAL
    assert L.dpow_census_batch(None, arr, 0, None) == EINVAL
    assert L.dpow_census_batch(None, arr, _lib.DPOW_BATCH_MAX + 1, None) == EINVAL
    assert L.dpow_census_batch(None, arr, 1, None) == EINVAL  # a NULL context, the tasks being good
    assert b"ctx is NULL" in L.dpow_last_error()
    assert ctypes.string_at(arr, ctypes.sizeof(arr)) == before
    del keep


def test_the_task_struct_is_the_headers():
    """dpow_census_task: 6 input words, k_done, status, then dpow_census (8-byte aligned)."""
    assert _lib.CensusTaskC.census.offset == 56
    assert ctypes.sizeof(_lib.CensusTaskC) == 56 + ctypes.sizeof(_lib.CensusC) == 56 + 33 * 8 * 2 + 33 * 4 + 4
