"""A CPU restatement of dpow_scan_batch_device's contract, shared by test_scan_many_dev_host.py and
test_gpu_scan_many_dev.py: what a launch's placed descriptors mean for the tasks, and a whole call's
statuses, k_done, rows and total from the tasks' hit lists.  The launches come from
distpow.census_plan, the batched census's planner, which test_census_many_host.py pins on its own;
nothing here calls the entry point under test."""
import numpy as np

import distpow

NO_ROW = None


def windows_of(tasks):
    """[(k_begin, k_end, worker_bits)] of ScanTasks."""
    return [(t.k_begin, t.k_end, t.worker_bits) for t in tasks]


def launches_of(windows, cap=0):
    """The call's launches: a list of descriptor lists [(task, i_begin, i_end), ...]."""
    if not any(kb < ke for kb, ke, _ in windows):
        return []
    blocks, n_launches = distpow.census_plan(windows, cap)
    out = [[] for _ in range(n_launches)]
    for b in blocks:
        out[b.launch].append((b.task, b.i_begin, b.i_end))
    return out


def settle_model(blocks, n_fit, i_begin, i_end, i_done, next_row, unfinished):
    """(i_done, next_row, row_block, status) after the first n_fit of `blocks` [(task, lo, hi)] were
    placed.  Stated from the outcome, not as the library's walk: a task's progress is the furthest end
    among its placed descriptors; the rows settled are those from next_row up to the last task that a
    placed descriptor begins, each naming the first such descriptor of a task at or behind it."""
    n = len(i_begin)
    placed = blocks[:n_fit]
    done = list(i_done)
    for t in range(n):
        ends = [hi for task, _, hi in placed if task == t]
        if ends:
            done[t] = max(ends)
    begun = [(task, b) for b, (task, lo, _) in enumerate(placed) if lo == i_begin[task]]
    row_block = [NO_ROW] * n
    if begun:
        last = max(task for task, _ in begun)
        for j in range(next_row, last + 1):
            row_block[j] = min(b for task, b in begun if task >= j)
        next_row = last + 1
    status = [distpow.EXHAUSTED if done[t] == i_end[t] else unfinished for t in range(n)]
    return done, next_row, row_block, status


def call_model(tasks, hits, max_hits, cap=0):
    """One dpow_scan_batch_device call over `tasks` (ScanTasks) whose complete hit lists are
    `hits[i]` (global indices, increasing: a list, or a numpy array where the lists are long): (results,
    rows, segments) -- results[i] = (status, k_done), rows the n + 1 row pointers, segments[i] the global
    indices the call lists for task i, a leading slice of hits[i].  A partition's local index rises with
    the global one, so a descriptor's hits are found by bisection."""
    n = len(tasks)
    rbits = [distpow.remainder_bits(t.worker_bits) for t in tasks]
    i_begin = [t.k_begin << r for t, r in zip(tasks, rbits)]
    i_end = [t.k_end << r for t, r in zip(tasks, rbits)]
    done = list(i_begin)

    def local(i, g):  # the local indices of the global indices g of task i
        g = np.asarray(g, dtype=np.uint64)
        return ((g >> np.uint64(8)) << np.uint64(rbits[i])) | (g & np.uint64((1 << rbits[i]) - 1))

    def below(i, x):  # how many of task i's hits lie below local index x
        return int(np.searchsorted(locs[i], np.uint64(x), side="left"))

    locs = [local(i, hits[i]) for i in range(n)]
    assert all(bool((x[1:] > x[:-1]).all()) for x in locs)
    room, cut = max_hits, False
    for blocks in launches_of(windows_of(tasks), cap):
        for task, lo, hi in blocks:
            c = below(task, hi) - below(task, lo)
            if c > room:
                cut = True
                break
            room -= c
            done[task] = hi
        if cut:
            break
    segments = [hits[i][:below(i, done[i])] for i in range(n)]
    rows = [0]
    for s in segments:
        rows.append(rows[-1] + len(s))
    results = [(distpow.EXHAUSTED, t.k_end) if done[i] == i_end[i] else (distpow.MORE, done[i] >> rbits[i])
               for i, t in enumerate(tasks)]
    return results, rows, segments
