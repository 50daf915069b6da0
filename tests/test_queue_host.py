"""Host side of the task queue (dpow_queue_*), no GPU needed: the entry points exist and refuse bad
arguments before any GPU work, and the launch planner (dpow_queue_plan) keeps its policy
(DESIGN.md "Task queue"): with one age it is the batch's round plan, with mixed ages every task
gets its ceiling, the launch stays within its budget and the oldest tasks get what is left."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import distpow
from distpow import _lib
from distpow.worker import Worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# csrc/batch.h, csrc/queue.h
FIRST, CAP, MIN_SLICE, BLOCKS, MIN_GROUP, MAX_GROUP = 1 << 20, 1 << 28, 256, 4096, 256, 16384
SPREAD, MAX_BLOCKS = 16, 32768

QUEUE_SYMBOLS = ["dpow_queue_open", "dpow_queue_close", "dpow_queue_submit", "dpow_queue_cancel", "dpow_queue_next",
                 "dpow_queue_wait", "dpow_queue_stats", "dpow_queue_plan", "dpow_worker_set_queue"]

DT = np.dtype([("launch", "<u4"), ("task", "<u4"), ("i_begin", "<u8"), ("i_end", "<u8"), ("group", "<u4"),
               ("rows", "<u4")])


def pow2_floor(x):
    return 1 << (x.bit_length() - 1) if x else 0


def pow2_ceil(x):
    return 1 if x <= 1 else pow2_floor(x - 1) << 1


def budget_of(age):
    return min(FIRST << (2 * min(age, 8)), CAP)


def launch_budget(ages):
    b = [budget_of(a) for a in ages]
    return min(max(b), SPREAD * min(b))


def ceiling_of(age, n, bd):
    """A task's share of a batch of n tasks at its own age, within this launch's budget."""
    return max(pow2_floor(min(budget_of(age), bd) // n), MIN_SLICE)


def plan(left, age):
    blocks, bd = distpow.queue_plan(left, age)
    a = np.frombuffer(blocks, dtype=DT) if len(blocks) else np.zeros(0, dtype=DT)
    return a, bd


def check_blocks(a, n):
    """The blocks tile each task's slice [0, slice) exactly once, ascending within a task, none
    above kBatchMaxGroup, early ordinals of every task before later ordinals of any; returns the
    slices."""
    assert len(a) <= MAX_BLOCKS
    group = int(a["group"][0])
    assert (a["group"] == group).all() and MIN_GROUP <= group <= MAX_GROUP and group & (group - 1) == 0
    size = (a["i_end"] - a["i_begin"]).astype(np.int64)
    assert (size > 0).all() and (size <= group).all()
    assert (a["launch"] == 0).all()
    ordinal = (a["i_begin"] // np.uint64(group)).astype(np.int64)
    assert (a["i_begin"] % np.uint64(group) == 0).all()
    assert (np.diff(ordinal) >= 0).all()                       # by ordinal first ...
    same = np.diff(ordinal) == 0
    assert (np.diff(a["task"].astype(np.int64))[same] > 0).all()   # ... then by task
    slices = np.zeros(n, dtype=np.int64)
    order = np.lexsort((a["i_begin"], a["task"]))
    s = a[order]
    first = np.r_[True, s["task"][1:] != s["task"][:-1]]
    assert (s["i_begin"][first] == 0).all()
    assert (s["i_begin"][1:][~first[1:]] == s["i_end"][:-1][~first[1:]]).all()   # gap-free, ascending
    np.add.at(slices, s["task"], (s["i_end"] - s["i_begin"]).astype(np.int64))
    counts = np.bincount(a["task"], minlength=n)
    assert (a["rows"] == counts[a["task"]]).all()
    return slices, group


def declared_functions():
    names = set()
    for h in ("dpow.h", "dpow_worker.h"):
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names |= set(re.findall(r"\b(dpow_[a-z0-9_]+)\s*\(", src))
    return names


def test_header_and_library_have_the_queue_entry_points():
    names = declared_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", distpow.LIB_PATH]).decode()
    exported = set(re.findall(r"\s[TW]\s+(dpow_[a-z0-9_]+)$", out, flags=re.M))
    L = distpow.lib()
    for sym in QUEUE_SYMBOLS:
        assert sym in names, sym
        assert sym in exported, sym
        assert getattr(L, sym).argtypes is not None
    assert ctypes.sizeof(_lib.QueueResultC) == 64
    assert distpow.EAGAIN == -8
    src = open(os.path.join(ROOT, "include", "dpow.h")).read()
    assert re.search(r"#define\s+DPOW_EAGAIN\s+\(-8\)", src)


def test_bad_arguments_are_codes_not_crashes():
    L = distpow.lib()
    t = ctypes.c_uint64(0)
    ok = (b"\x01\x02\x03\x04", 4, 3, 0, 0, 0, 8, distpow.DPOW_NO_HIT, 0)
    # the task's own errors come first: they show without a queue
    assert L.dpow_queue_submit(None, b"\x01", 1, 2, 0, 0, 9, 8, distpow.DPOW_NO_HIT, 0, ctypes.byref(t)) == distpow.EINVAL
    assert "k_begin > k_end" in _lib.last_error() and "dpow_queue_submit" in _lib.last_error()
    assert L.dpow_queue_submit(None, b"\x01", 1, 2, 0, 0, 0, distpow.DPOW_K_LIMIT + 1, distpow.DPOW_NO_HIT, 0,
                               ctypes.byref(t)) == distpow.ERANGE
    assert L.dpow_queue_submit(None, b"\x01", 1, 2, 256, 0, 0, 8, distpow.DPOW_NO_HIT, 0, ctypes.byref(t)) == distpow.EINVAL
    assert "worker_byte" in _lib.last_error()
    assert L.dpow_queue_submit(None, bytes(1025), 1025, 2, 0, 0, 0, 8, distpow.DPOW_NO_HIT, 0,
                               ctypes.byref(t)) == distpow.EINVAL
    assert "DPOW_MAX_NONCE" in _lib.last_error()
    assert L.dpow_queue_submit(None, None, 4, 2, 0, 0, 0, 8, distpow.DPOW_NO_HIT, 0, ctypes.byref(t)) == distpow.EINVAL
    assert "nonce is NULL" in _lib.last_error()
    assert L.dpow_queue_submit(None, *ok, ctypes.byref(t)) == distpow.EINVAL       # a good task, no queue
    assert "NULL argument" in _lib.last_error()
    assert t.value == 0
    r = _lib.QueueResultC()
    assert L.dpow_queue_cancel(None, 1) == distpow.EINVAL
    assert L.dpow_queue_next(None, ctypes.byref(r), 0) == distpow.EINVAL
    assert L.dpow_queue_wait(None, 1, ctypes.byref(r), 0) == distpow.EINVAL
    assert L.dpow_queue_stats(None, None, None, None) == distpow.EINVAL
    assert L.dpow_worker_set_queue(None, 1) == distpow.EINVAL
    L.dpow_queue_close(None)   # no-op
    assert L.dpow_queue_open(0, None) == distpow.EINVAL
    # the planner
    left = (ctypes.c_uint64 * 2)(5, 0)
    age = (ctypes.c_uint32 * 2)(0, 0)
    bd = ctypes.c_uint64()
    assert L.dpow_queue_plan(None, age, 1, None, 0, ctypes.byref(bd)) == distpow.EINVAL
    assert L.dpow_queue_plan(left, None, 1, None, 0, ctypes.byref(bd)) == distpow.EINVAL
    assert L.dpow_queue_plan(left, age, 1, None, 0, None) == distpow.EINVAL
    assert L.dpow_queue_plan(left, age, 0, None, 0, ctypes.byref(bd)) == distpow.EINVAL
    assert L.dpow_queue_plan(left, age, _lib.DPOW_BATCH_MAX + 1, None, 0, ctypes.byref(bd)) == distpow.EINVAL
    assert L.dpow_queue_plan(left, age, 2, None, 0, ctypes.byref(bd)) == distpow.EINVAL   # a task with nothing left
    assert L.dpow_queue_plan(left, age, 1, None, 0, ctypes.byref(bd)) == 1 and bd.value == FIRST
    with pytest.raises(ValueError):
        distpow.queue_plan([1, 2], [0])


def test_open_fails_loudly_without_a_device():
    if distpow.device_count() > 0:
        with distpow.TaskQueue(0) as q:
            assert q.stats()[1:] == (0, 0)
        return
    with pytest.raises(distpow.DpowError) as e:
        distpow.TaskQueue(0)
    assert e.value.code == distpow.EHIP and "no HIP device" in str(e.value)
    with pytest.raises(distpow.DpowError) as e:
        Worker(0, queue=True)
    assert e.value.code == distpow.EHIP


def batch_slice(r, n):
    return max(pow2_floor(min(FIRST << (2 * min(r, 8)), CAP) // n), MIN_SLICE)


@pytest.mark.parametrize("n", [1, 2, 3, 16, 255, 256, 1000, 4096])
def test_same_age_plan_is_the_batch_round(n):
    """P1: tasks of one age get batch_round's slices and group -- dpow_batch_plan's launch `age` for
    windows that have that much left at that round."""
    for age in range(7):
        before = sum(batch_slice(r, n) for r in range(age))      # what every task has behind it at that round
        s_a = batch_slice(age, n)
        for short in (None, 1, 255, 256, 257):
            left = [3 * s_a + 17] * n
            if short is not None:
                left[n // 2] = short
            # worker_bits 8: one thread byte per k, so local indices are k
            ref, launches = distpow.batch_plan([(0, before + x, 8) for x in left])
            ref = np.frombuffer(ref, dtype=DT)
            ref = ref[ref["launch"] == age]
            assert len(ref) == n and (ref["i_begin"] == before).all(), (n, age, short)
            a, bd = plan(left, [age] * n)
            slices, group = check_blocks(a, n)
            want = (ref["i_end"] - ref["i_begin"]).astype(np.int64)
            assert (slices[ref["task"]] == want).all(), (n, age, short)
            assert group == int(ref["group"][0]), (n, age, short, group)
            assert bd == budget_of(age)
            assert (slices == np.minimum(np.array(left), s_a)).all()


MIXED = {
    "one old among fresh": [5] + [0] * 50,
    "ages 0..8": list(range(9)),
    "one old among 4095 fresh": [0] * 4095 + [8],
}


@pytest.mark.parametrize("case", sorted(MIXED))
@pytest.mark.parametrize("short", [False, True])
def test_mixed_ages(case, short):
    ages = MIXED[case]
    n = len(ages)
    left = [1 << 40] * n
    if short:   # some tasks end inside their ceiling
        left[0], left[n // 2] = 100, 257
    a, bd = plan(left, ages)
    slices, group = check_blocks(a, n)
    assert bd == launch_budget(ages)
    assert bd <= SPREAD * min(budget_of(x) for x in ages) and bd <= CAP
    for i in range(n):
        assert slices[i] >= min(left[i], ceiling_of(ages[i], n, bd)), (i, ages[i])
        assert slices[i] <= left[i]
    assert slices.sum() <= bd + n * MIN_SLICE
    oldest = max(ages)
    younger = sum(int(slices[i]) for i in range(n) if ages[i] != oldest)
    n_old = sum(1 for x in ages if x == oldest)
    for i in range(n):
        if ages[i] == oldest and left[i] > bd:
            assert slices[i] >= pow2_floor((bd - younger) // n_old), (i, slices[i])
            assert 2 * slices[i] * n_old > bd - younger          # the power-of-two floor: at least half
    assert len(a) <= MAX_BLOCKS


def test_fresh_task_keeps_the_launch_short():
    """A launch that holds a fresh task hashes at most 2^24 candidates; old tasks alone grow to the cap."""
    a, bd = plan([1 << 40] * 3, [0, 6, 8])
    assert bd == 1 << 24
    a, bd = plan([1 << 40] * 3, [5, 6, 8])
    assert bd == CAP


def test_replay_fresh_arrivals_beside_one_old_task():
    """A fresh task arrives before each of 40 launches beside one old task: every task's covered
    range is gap-free and ascending, and the old task gets at least an even split of each launch."""
    fresh_len = 64 * 256
    tasks = [{"left": 1 << 44, "age": 0, "pos": 0, "cover": []}]   # the old task first
    even = 0
    finished = 0
    for launch in range(40):
        tasks.append({"left": fresh_len, "age": 0, "pos": 0, "cover": []})
        live = [t for t in tasks if t["left"] > 0]
        a, bd = plan([t["left"] for t in live], [t["age"] for t in live])
        slices, group = check_blocks(a, len(live))
        even += bd // len(live)
        for t, s in zip(live, slices):
            s = int(s)
            assert 0 < s <= t["left"]
            t["cover"].append((t["pos"], t["pos"] + s))
            t["pos"] += s
            t["left"] -= s
            t["age"] += 1
            finished += t["left"] == 0
        assert len(live) <= 3          # a fresh task is over within two launches
    for t in tasks:
        assert t["cover"][0][0] == 0
        assert all(b[0] == a_[1] and b[1] > b[0] for a_, b in zip(t["cover"], t["cover"][1:]))
    assert finished >= 39
    assert tasks[0]["pos"] >= even, (tasks[0]["pos"], even)
