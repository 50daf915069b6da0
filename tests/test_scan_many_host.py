"""Host side of the batched scan (dpow_scan_batch), no GPU needed: the launch planner (dpow_scan_plan,
the function the call's own loop steps through), the halving rule of its overflow path
(dpow_scan_plan_halve) and the argument errors that are decided before the device is touched.

The planner's rules (include/dpow.h): a launch takes tasks in array order under
two budgets, `cap` local indices and capacity / 4 hit weight, a part of n indices at depth N weighing
ceil(n / 16^min(N, 7)); only its last task can be cut, at a multiple of 256 local indices from the
task's begin; a task's part of a launch is cut into descriptors of batch_group(the launch's total),
the last one possibly shorter; an empty task has no descriptor.  (A raised cancel flag on entry needs
a context, so a device: tests/test_gpu_scan_many.py has it.)"""
import ctypes
import random

import numpy as np
import pytest

import distpow
from distpow import DPOW_K_LIMIT, EINVAL, ERANGE, _lib

CAP = 1 << 28            # local indices per launch (csrc/batch.h kBatchCap)
LIST = 1 << 16           # entries of a launch's hit list (csrc/md5_scan.h kScanCap)
BLOCKS = 4096            # workgroups a launch aims for (kBatchBlocks)
MIN_GROUP, MAX_GROUP = 256, 16384  # kBatchMinGroup, kBatchMaxGroup
MAX_BLOCKS = _lib.SCAN_MANY_MAX_BLOCKS

DT = np.dtype([("launch", "<u4"), ("task", "<u4"), ("i_begin", "<u8"), ("i_end", "<u8"), ("group", "<u4"),
               ("rows", "<u4")])


def _batch_group(total):
    """csrc/batch.cpp batch_group."""
    q = total // BLOCKS
    return min(max(1 << (q.bit_length() - 1) if q else 0, MIN_GROUP), MAX_GROUP)


def _weight(n, ntz):
    d = 16 ** min(ntz, 7)
    return (n + d - 1) // d


def _launches(a):
    """[(s, e)] index ranges of the plan's launches."""
    if not len(a):
        return []
    seam = a["launch"][1:] != a["launch"][:-1]
    starts = np.flatnonzero(np.concatenate(([True], seam)))
    return list(zip(starts.tolist(), np.concatenate((starts[1:], [len(a)])).tolist()))


def _parts(a, s, e):
    """[(task, lo, hi)] of the launch a[s:e]: its descriptors joined per task."""
    out = []
    for t, lo, hi in zip(a["task"][s:e].tolist(), a["i_begin"][s:e].tolist(), a["i_end"][s:e].tolist()):
        if out and out[-1][0] == t and out[-1][2] == lo:
            out[-1][2] = hi
        else:
            out.append([t, lo, hi])
    return out


def _check_plan(windows, cap=0, capacity=0):
    """Every rule on the plan of `windows` = [(i_begin, i_end, ntz)]; returns (entries, launches)."""
    entries, launches = distpow.scan_plan(windows, cap, capacity)
    assert ctypes.sizeof(_lib.BatchRange) == DT.itemsize
    a = np.frombuffer(entries, dtype=DT) if len(entries) else np.zeros(0, dtype=DT)
    budget = (cap or CAP) & ~255
    w_budget = ((capacity or LIST) // 4) & ~255
    ib = np.array([w[0] for w in windows], dtype=np.uint64)
    ie = np.array([w[1] for w in windows], dtype=np.uint64)
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
    # coverage: exactly the non-empty tasks appear, and a task's descriptors tile its range once, in order
    assert sorted(set(task.tolist())) == live
    same = task[1:] == task[:-1]
    assert (lo[1:][same] == hi[:-1][same]).all()
    first = np.concatenate(([True], ~same))
    last = np.concatenate((~same, [True]))
    assert (lo[first] == ib[task[first]]).all() and (hi[last] == ie[task[last]]).all()
    # cuts: between launches a task is cut only at a multiple of 256 from its begin, and only a
    # launch's last task is (a launch's other tasks end in it: the tiling above says so)
    seam = launch[1:] != launch[:-1]
    cut = seam & same
    assert ((hi[:-1][cut] - ib[task[:-1][cut]]) % 256 == 0).all()
    assert (size <= MAX_GROUP).all()
    for n, (s, e) in enumerate(_launches(a)):
        total = int(size[s:e].sum())
        parts = _parts(a, s, e)
        weight = sum(_weight(p_hi - p_lo, windows[t][2]) for t, p_lo, p_hi in parts)
        # both budgets, the descriptor bound, the group
        assert total <= budget, (n, total)
        assert weight <= w_budget, (n, weight)
        assert e - s <= MAX_BLOCKS, (n, e - s)
        # a launch takes at least 256 indices, or every index the tasks have left
        assert total >= 256 or n + 1 == launches or parts[-1][2] == windows[parts[-1][0]][1], (n, total)
        group = _batch_group(total)
        assert (a["group"][s:e] == group).all(), (n, group)
        assert (size[s:e] <= group).all()
        # every descriptor of a task's part but its last is a whole group; rows counts the part's
        part_last = np.concatenate((task[s + 1:e] != task[s:e - 1], [True]))
        assert (size[s:e][~part_last] == group).all()
        t_l, cnt = np.unique(task[s:e], return_counts=True)
        rows = dict(zip(t_l.tolist(), cnt.tolist()))
        assert a["rows"][s:e].tolist() == [rows[t] for t in task[s:e].tolist()]
        # greedy fill: a launch that is not the last had no room for 256 more indices of the next task
        if n + 1 < launches:
            t_next = int(task[e])
            room = min(budget - total, (w_budget - weight) * 16 ** min(windows[t_next][2], 7))
            left = int(ie[t_next] - lo[e])
            assert room < 256 and left > room, (n, total, weight)
    return a, launches


@pytest.mark.parametrize("ntz", list(range(10)) + [32])
def test_a_single_task_steps_by_the_scans_slice(ntz):
    """One task: the launches are dpow_scan's, scan_slice(N) local indices each from the window's begin."""
    slice_ = distpow.scan_slice(ntz)
    assert slice_ == {0: 1 << 14, 1: 1 << 18, 2: 1 << 22, 3: 1 << 26}.get(ntz, 1 << 28)
    for i0, n in [(0, 1), (7 << 8, 3 * slice_ + 256 * 5), (5, min(4 * slice_, 1 << 30) + 77), (256, slice_),
                  (1 << 32, slice_ + 1)]:
        a, launches = _check_plan([(i0, i0 + n, ntz)])
        lo, end, k = i0, i0 + n, 0
        for s, e in _launches(a):
            hi = min(lo + slice_, end)
            assert (int(a["i_begin"][s]), int(a["i_end"][e - 1])) == (lo, hi), (ntz, k)
            group = _batch_group(hi - lo)
            assert e - s == (hi - lo + group - 1) // group and (a["group"][s:e] == group).all()
            lo, k = hi, k + 1
        assert lo == end and k == launches == (n + slice_ - 1) // slice_


@pytest.mark.parametrize("cap, capacity", [(0, 0), (1 << 20, 0), (512, 0), (768, 0), (0, 1024), (1 << 16, 4096)])
def test_both_budgets_hold_for_random_mixes(cap, capacity):
    """Mixed depths and sizes, empty tasks in the middle, B up to 4096: _check_plan's rules."""
    rnd = random.Random(cap * 7 + capacity + 1)
    small_budget = (cap and cap <= 1024) or (capacity and capacity <= 1024)
    for B in (1, 2, 3, 17, 256) + (() if small_budget else (4096,)):  # (small budgets: thousands of launches)
        windows = []
        for j in range(B):
            ntz = rnd.choice((0, 0, 1, 1, 2, 3, 4, 5, 7, 8, 32, 40))
            # sizes that keep the plan to some 10^5 descriptors: dense tasks stay small
            top = {0: 13, 1: 17}.get(ntz, 22)
            if B >= 256 or small_budget:
                top = min(top, 12)
            i0 = rnd.choice((0, 256, 3 << 5, 255 << 8, 65530 << 8, 1 << 32))
            n = 0 if rnd.random() < 0.15 else rnd.choice((1, 32, 255, 256, 257, rnd.randrange(1, (1 << top) + 1),
                                                          1 << top))
            windows.append((i0, i0 + n, ntz))
        if B >= 3:
            windows[B // 2] = (9, 9, 0)  # an empty task in the middle
        if not cap and not capacity and B < 256:
            windows[rnd.randrange(B)] = (5, 5 + (1 << 29), 9)  # a task of two launches' candidates
        a, launches = _check_plan(windows, cap, capacity)
        print(f"cap {cap or CAP} capacity {capacity or LIST} B {B}: {len(a)} descriptors in {launches} launches")
        assert launches >= 1 or all(w[0] == w[1] for w in windows)


def test_the_hit_weight_cuts_a_dense_task_next_to_sparse_ones():
    """A launch's weight counts every part: dense tasks fill it long before the candidate budget."""
    # 2^14 weight: the N = 0 task takes 10000, the N = 1 task 16 * 6384 = 102144 indices and is cut there
    a, launches = _check_plan([(0, 10000, 0), (0, 1 << 20, 1), (0, 1 << 20, 8)])
    (s, e), = _launches(a)[:1]
    assert _parts(a, s, e) == [[0, 0, 10000], [1, 0, 102144]]
    # N >= 7 weighs 1 per 2^28: 4096 one-k tasks at N = 8 are one launch, 4096 at N = 0 are 64
    assert _check_plan([(j << 8, (j + 1) << 8, 8) for j in range(4096)])[1] == 1
    assert _check_plan([(j << 8, (j + 1) << 8, 0) for j in range(4096)])[1] == 64
    # ceil, not floor: 4096 tasks of one candidate at N = 3 weigh 4096, not 1
    a, launches = _check_plan([(j, j + 1, 3) for j in range(4096)], 0, 4096)
    assert launches == 4 and [e - s for s, e in _launches(a)] == [1024] * 4


def test_the_descriptor_bound_is_met():
    assert MAX_BLOCKS == CAP // MAX_GROUP + _lib.DPOW_BATCH_MAX == 20480
    a, launches = _check_plan([(0, 65537, 8)] * 4095 + [(0, 1 << 20, 8)])
    assert launches == 2 and (a["launch"] == 0).sum() == 4095 * 5 + 4 == 20479 <= MAX_BLOCKS


def test_empty_tasks_have_no_part():
    a, launches = _check_plan([(4, 4, 0), (0, 0, 8), (DPOW_K_LIMIT << 8, DPOW_K_LIMIT << 8, 3)])
    assert len(a) == 0 and launches == 0
    a, launches = _check_plan([(4, 4, 0), (0, 300, 1), (7, 7, 3), (0, 10, 0), (1 << 40, 1 << 40, 0)])
    assert launches == 1 and a["task"].tolist() == [1, 1, 3]


def test_seams_of_the_gpu_test():
    """DPOW_DIAG_SCAN_MANY_CAP = 512 and 768 cut tasks at k = 255/256 and 65535/65536 (partition width 2 per k)."""
    windows = [(250 << 1, 262 << 1, 1), (65530 << 1, 65542 << 1, 2), (0, 3 << 8, 0)]
    for cap in (512, 768):
        a, launches = _check_plan(windows, cap)
        cuts = {(int(t), int(h)) for (s, e) in _launches(a)[:-1] for t, h in [(a["task"][e - 1], a["i_end"][e - 1])]}
        assert launches > 1 and all(h % 256 == windows[t][0] % 256 for t, h in cuts)


def test_halving_reaches_256():
    """The overflow path: the launch at the cursor shrinks strictly with every halving, down to 256
    candidates, for a dense task, a sparse one and a mix; the budgets stay multiples of 256."""
    for windows in ([(0, 1 << 20, 0)], [(0, 1 << 30, 5)], [(0, 1 << 15, 1)] * 8,
                    [(0, 100, 0), (0, 1 << 24, 2), (0, 5000, 0)]):
        cap, capacity, steps, prev = 0, 0, 0, None
        while True:
            a, _ = _check_plan(windows, cap, capacity)
            s, e = _launches(a)[0]
            parts = _parts(a, s, e)
            total = sum(h - l for _, l, h in parts)
            weight = sum(_weight(h - l, windows[t][2]) for t, l, h in parts)
            assert prev is None or total < prev
            if total <= 256:
                break
            prev = total
            windows = [(l, h, windows[t][2]) for t, l, h in parts]  # the call plans the same parts again
            cap, capacity = distpow.scan_plan_halve(total, weight)
            assert cap % 256 == 0 and capacity % 1024 == 0 and 256 <= cap <= max(256, (total + 1) // 2 + 255)
            assert 1024 <= capacity <= LIST // 2
            steps += 1
        assert steps <= 28
    assert distpow.scan_plan_halve(256, 256) == (256, 1024)
    assert distpow.scan_plan_halve(1 << 28, 1 << 14) == (1 << 27, 1 << 15)
    assert distpow.scan_plan_halve(257, 1) == (256, 1024)


def test_plan_argument_errors():
    L = distpow.lib()
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    n_l = u64()

    def call(ib=(0,), ie=(1024,), nz=(1,), n=1, cap=0, capacity=0, launches=ctypes.byref(n_l)):
        return L.dpow_scan_plan((u64 * len(ib))(*ib), (u64 * len(ie))(*ie), (u32 * len(nz))(*nz), n, cap, capacity,
                                None, 0, launches)

    assert call() == 4 and n_l.value == 1  # 1024 local indices: four descriptors of 256 in one launch
    assert call(launches=None) == EINVAL
    assert call(n=0) == EINVAL
    assert call(ib=(0,) * 4097, ie=(1,) * 4097, nz=(0,) * 4097, n=4097) == EINVAL
    assert call(ib=(2000,)) == EINVAL
    assert call(ie=((DPOW_K_LIMIT << 8) + 1,)) == ERANGE
    assert call(cap=255) == EINVAL and call(cap=CAP + 1) == EINVAL
    assert call(capacity=1023) == EINVAL and call(capacity=LIST + 1) == EINVAL
    assert call(cap=511) == 4 and n_l.value == 4  # rounded down to a multiple of 256: four launches of one
    assert call(nz=(0,), capacity=2047) == 4 and n_l.value == 4  # 256 hit weight: four launches at N = 0
    assert L.dpow_scan_plan(None, None, None, 1, 0, 0, None, 0, ctypes.byref(n_l)) == EINVAL


def _tasks(specs):
    """A dpow_scan_task array for [(nonce bytes or None, nonce_len, ntz, worker_byte, worker_bits, k_begin, k_end)]
    with every output byte set to 0xA5, and what keeps its nonces alive."""
    arr = (_lib.ScanTaskC * len(specs))()
    ctypes.memset(arr, 0xA5, ctypes.sizeof(arr))
    keep = []
    for c, (nonce, nlen, ntz, wb, wbits, k0, k1) in zip(arr, specs):
        buf = ctypes.create_string_buffer(nonce, max(len(nonce), 1)) if nonce is not None else None
        keep.append(buf)
        c.nonce = ctypes.addressof(buf) if buf is not None else None
        c.nonce_len, c.ntz, c.worker_byte, c.worker_bits, c.k_begin, c.k_end = nlen, ntz, wb, wbits, k0, k1
    return arr, keep


GOOD = (b"\x01\x02\x03\x04", 4, 1, 0, 0, 0, 4)


def _out(n=256):
    out = (_lib.ScanHitC * n)()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    return out


@pytest.mark.parametrize("bad, code", [
    ((b"\x01\x02\x03\x04", 4, 1, 256, 0, 0, 4), EINVAL),                       # worker_byte > 255
    ((b"\x01\x02\x03\x04", 4, 1, 0, 0, 5, 4), EINVAL),                         # k_begin > k_end
    ((bytes(_lib.DPOW_MAX_NONCE + 1), _lib.DPOW_MAX_NONCE + 1, 1, 0, 0, 0, 4), EINVAL),  # nonce too long
    ((None, 4, 1, 0, 0, 0, 4), EINVAL),                                        # NULL nonce with a length
    ((b"\x01\x02\x03\x04", 4, 1, 0, 0, 0, DPOW_K_LIMIT + 1), ERANGE),          # k_end beyond DPOW_K_LIMIT
], ids=["worker_byte", "k_order", "nonce_len", "nonce_null", "k_limit"])
@pytest.mark.parametrize("where", [0, 2])
def test_argument_errors_leave_everything_untouched(bad, code, where):
    """The tasks' own errors come before the context's: a NULL context reaches every one of them."""
    specs = [GOOD, GOOD, GOOD]
    specs[where] = bad
    arr, keep = _tasks(specs)
    before = ctypes.string_at(arr, ctypes.sizeof(arr))
    out, n_out, st = _out(), ctypes.c_size_t(77), _lib.BatchStats(7, 7, 7, 7.0)
    assert distpow.lib().dpow_scan_batch(None, arr, 3, out, 256, ctypes.byref(n_out), ctypes.byref(st)) == code
    assert ctypes.string_at(arr, ctypes.sizeof(arr)) == before
    assert ctypes.string_at(out, ctypes.sizeof(out)) == b"\xa5" * ctypes.sizeof(out) and n_out.value == 77
    assert (st.launches, st.candidates) == (7, 7)
    del keep


def test_call_argument_errors():
    L = distpow.lib()
    arr, keep = _tasks([GOOD])
    before = ctypes.string_at(arr, ctypes.sizeof(arr))
    out, n_out = _out(), ctypes.c_size_t(77)
    pn = ctypes.byref(n_out)
    assert L.dpow_scan_batch(None, None, 1, out, 256, pn, None) == EINVAL
    assert L.dpow_scan_batch(None, arr, 0, out, 256, pn, None) == EINVAL
    assert L.dpow_scan_batch(None, arr, _lib.DPOW_BATCH_MAX + 1, out, 256, pn, None) == EINVAL
    assert L.dpow_scan_batch(None, arr, 1, None, 256, pn, None) == EINVAL
    assert L.dpow_scan_batch(None, arr, 1, out, 256, None, None) == EINVAL
    assert L.dpow_scan_batch(None, arr, 1, out, 255, pn, None) == EINVAL
    assert b"max_hits" in L.dpow_last_error()
    assert L.dpow_scan_batch(None, arr, 1, out, 256, pn, None) == EINVAL  # a NULL context, the rest being good
    assert b"ctx is NULL" in L.dpow_last_error()
    assert ctypes.string_at(arr, ctypes.sizeof(arr)) == before and n_out.value == 77
    del keep


def test_the_task_struct_is_the_headers():
    """dpow_scan_task: 7 input words (the three 32-bit ones padded to 16 bytes), k_done, status, first_hit, n_hits."""
    T = _lib.ScanTaskC
    assert (T.ntz.offset, T.k_begin.offset, T.k_done.offset, T.status.offset, T.first_hit.offset,
            T.n_hits.offset) == (16, 32, 48, 56, 64, 72)
    assert ctypes.sizeof(T) == 80
