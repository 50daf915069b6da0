"""GPU: the batched device scan's own kernels (scan_many_mask_kernel, scan_many_place_kernel,
scan_many_rows_kernel, scan_many_depth_kernel and the retirement prefix of csrc/md5_scan_many_dev.hip),
its host cut (csrc/scan_many_dev.cpp) and digest_many_kernel (csrc/md5_digest_many.hip) behind it, at
every layout edge, every group size, all ten prefix rounds and page cuts in later launches and inside
tasks.

The order of the list is geometry, as the device scan's is (tests/test_gpu_scan_dev_walk.py): the word
4 s + wave of a descriptor's 256-word slot, the `steps` count behind the loop, the last workgroup's
prefix over up to 20480 totals in rounds of 2048.  wave_inclusive_scan and the prefix rounds are a second
copy of md5_scan_dev.hip's, and tests/test_gpu_scan_many_dev.py reaches groups 256, 1024 and 16384, three
rounds and one-launch cuts.  Every assertion here is an equality with hashlib, arithmetic, the digest
kernel (W.window_depths_cuda), Miner.scan_cuda, Miner.scan_many or the CPU restatement of the paging
contract (_scan_many_dev_model.call_model); none compares the unit with itself.
tests/test_scan_many_dev_walk_cases.py shows on the CPU that families M and X are what they name.

1. test_edges: the 39 sets of tests/test_gpu_listing_walk.py, one scan_batch_cuda call per set at N = 1
   and one at N = 3: statuses, rows, indices and depths per task are hashlib's.  At N = 1 the list goes
   on to digests_many_cuda without leaving the GPU: all 16 digest bytes of every entry are hashlib's,
   the depths the scan's, nothing shallow, and with N raised to 2 each task's shallow count is its
   depth-1 entries by hashlib -- digest_many_kernel on seams made by real hit lists of tasks whose
   layouts differ inside a wave.  One set per family again under a launch budget of 256 candidates.
2. test_group_sizes: family M -- per group 512 to 16384 one call of five tasks (4100 descriptors, three
   rounds; last descriptors ragged across steps with a half wave, shorter than a step, one step, and
   one step whose wave 3 has 33 lanes; an empty task; one- and two-block nonces; 32, 256 and 1
   candidates per k) and three calls at group 256 of 2047, 2048 and 2049 descriptors -- largest first
   and smallest first on one context, each at N = 3, 1, 0 (sparse first: a call's sparse launch sits
   on the dense bitmap and totals of the call before it; the device-scan walk's docstring has the
   mutant that showed why).  N = 0: every index of every partition, built arithmetically.  N = 1
   and 3: the indices whose depth by the digest kernel is at least N.  The rows are the same counts'
   sums.  At groups 512 and 4096 the N = 3 list is also Miner.scan_many's.
3. test_all_prefix_rounds: family X, 20416 descriptors in ten rounds, 4096 tasks.  N = 3: the large
   task's segment is Miner.scan_cuda's, the 4095 small ones Miner.scan_many's, the rows their counts'
   sums; then digests_many_cuda bisects 4097 rows: depths the scan's, nothing shallow, the entry counts
   the row differences, the small tasks' digests hashlib's.  N = 1 behind it: 1.7e7 entries and dense
   totals in every round.
4. test_stale_slot_words: a dense call at group 16384 sets every word of 8192 slots; the g = 512 call
   at N = 3 and its 96-index task alone on the same fresh context read none of them.
5. test_cut_in_a_later_launch, test_cut_inside_a_task_at_a_large_group: every page's statuses,
   k_done, rows and list are call_model's; a cut in the third launch of a call that still places one
   descriptor from it (a non-zero base with fewer descriptors placed than the launch has), and cuts
   strictly inside multi-descriptor tasks whose group falls as the call shrinks.

Every test prints its wall time (pytest -s).  On an MI355X pytest reports 4.3 s for the 45 tests run alone
(context and hashlib's lists included; the process takes 6.0 s) beside the device-scan walk's 4.4 s for
46 tests.  Inside the tests: test_edges 1.2 s for the 39 sets, 0.66 s of it the first set's (hashlib
builds family A's lists there when this file runs alone), 10 to 30 ms a set behind it (three or four
calls and hashlib's digests of the N = 1 hits; the calls themselves 3 to 12 ms a set);
test_group_sizes 0.35 s and 0.04 s for 27 calls each, the reference of 1.3e8 candidates in the first, a
call 0.3 ms (m2048 at N = 3 and 1) to 0.46 ms (its 8.4e6 entries at N = 0); test_all_prefix_rounds
0.36 s (0.28 s in another run) -- at N = 3 references 86 ms (9 ms), the call 4.8 ms for 65894 hits,
digests_many_cuda 1.6 ms; at N = 1 references 0.14 s (Miner.scan_many's 65000 host hits), the call
5.4 ms for 16778247 entries -- so the N = 1 pass is under half of its test and a thirtieth of the
file, and stays whole; test_stale_slot_words 13 ms; test_cut_in_a_later_launch 82 ms for 4 pages;
test_cut_inside_a_task_at_a_large_group 0.18 s for 33 and 29 pages and scan_many_cuda's pages.  What dominates is hashlib (the edge
lists and digests) and Python (call_model and the planner per page, 2.5 ms a page), not the GPU.

Shown to bite on five deliberately wrong libraries (built outside the tree, one run each over this file
and tests/test_gpu_scan_many_dev.py; every one stays in bounds by construction: it changes register
values, reads fewer words or makes a prefix smaller, and every list store stays clamped to max_hits):
  1. ScanManyMaskGroup keeps no ballot of a wave's last step when that step is partial and not step 0.
     Fails test_group_sizes[descending, ascending] -- every m-call at N = 0 (t0 is 32 entries short: the
     half wave of its last descriptor is the only partial step behind a step 0) and those at N = 1
     where the half wave has a hit -- and passes the other 43; tests/test_gpu_scan_many_dev.py passes on
     it.
  2. scan_many_place_kernel rounds n_words down to a multiple of 4 when it is above 4.  Fails
     test_group_sizes[descending, ascending] on the m-calls (the entries not placed are whatever the
     buffer held, and the call's own check refuses the list), passes the other 43;
     tests/test_gpu_scan_many_dev.py fails test_readme_tasks on it, through the same check, and passes
     its other 14.
  3. scan_many_mask_retire loses the prefix carry from the fourth round on.  Fails
     test_all_prefix_rounds ("row pointers that do not ascend to the total"), test_stale_slot_words (the
     dense call's 8192 descriptors are four rounds; the depth launch's count refuses the list) and
     test_cut_inside_a_task_at_a_large_group (the later pages' launches fall to smaller groups and more
     than 6144 descriptors, and the host's cut finds that the prefix does not end at the total);
     passes the other 42, family M's 4100 descriptors among them, rightly.
     tests/test_gpu_scan_many_dev.py passes on it: it has three rounds at the most.
  4. batch_hash_at, shared by the generic kernels: every lane takes the second block's state when any
     lane of its wave needs it.  Fails test_edges[A-0..6, B-0..6, G-0..6], as the other copies did in
     tests/test_gpu_listing_walk.py, and F-0..6 through the depth and digest kernels, whose waves hold
     hits from both sides of an edge; passes B-7, F-7, all controls and the other 6 tests.
     tests/test_gpu_scan_many_dev.py passes on it.
  5. digest_many_kernel: a wave that meets a seam gives all its entries its first entry's task.  Fails
     test_edges on all 39 sets and test_all_prefix_rounds; passes the other 5, which do not call it, and
     tests/test_gpu_scan_many_dev.py, which does not either.
"""
import time

import numpy as np
import pytest
import torch

import _batch_walk_cases as W
import distpow
from distpow import EXHAUSTED, MORE, ScanTask
from _digests_many_cases import hashlib_of
from _scan_many_dev_model import call_model, launches_of, windows_of
from test_gpu_listing_walk import IDS, SETS, _cases, _key, _still_usable

pytestmark = pytest.mark.gpu

MIN_HITS = distpow.SCAN_DEVICE_MIN_HITS   # 16384: the smallest max_hits
ROUND = W.SCAN_DEV_PREFIX_ROUND
H_NTZ = (3, 1, 0)                         # sparse first (part 2 of the docstring)
CAP_ENV = "DPOW_DIAG_SCAN_MANY_DEV_CAP"
CAPPED_SETS = ("A-1", "B-7", "F-7", "G-1")


def _dev(miner):
    return torch.device("cuda", miner.device)


def _cum(counts):
    rows = [0]
    for c in counts:
        rows.append(rows[-1] + c)
    return rows


def _scan_tasks(cases, ntz):
    return [ScanTask(c.task.nonce, ntz, c.task.worker_byte, c.task.worker_bits, c.task.k_begin, c.task.k_end)
            for c in cases]


# ---- 1. layout edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SETS, ids=IDS)
def test_edges(miner, monkeypatch, which):
    """One call per set: every hit of every task with its depth, the rows and, through
    digest_many_kernel, the digests are hashlib's."""
    monkeypatch.delenv(CAP_ENV, raising=False)
    cases = _cases(which)
    name = IDS[SETS.index(which)]
    room = max(MIN_HITS, sum((c.task.k_end - c.task.k_begin) << (8 - c.wbits) for c in cases))
    t0, n_hits = time.perf_counter(), 0
    for ntz in (1, 3):
        tasks = _scan_tasks(cases, ntz)
        want = [[(g, tz) for g, tz in W.depths_of(c) if tz >= ntz] for c in cases]
        want_rows = _cum(len(x) for x in want)
        want_idx, want_dep = [g for x in want for g, _ in x], [tz for x in want for _, tz in x]
        res, idx, dep, rows = miner.scan_batch_cuda(tasks, max_hits=room)
        assert res == [(EXHAUSTED, t.k_end) for t in tasks], (name, ntz)
        assert rows.tolist() == want_rows == miner.last_scan_many_device_rows, (name, ntz)
        got_idx, got_dep = idx.tolist(), dep.tolist()
        for j, c in enumerate(cases):         # per task, so that a failure names the window
            a, b = want_rows[j], want_rows[j + 1]
            assert (got_idx[a:b], got_dep[a:b]) == (want_idx[a:b], want_dep[a:b]), (ntz,) + _key(c)
        assert miner.last_scan_many_device_stats.rounds == 1
        n_hits += len(want_idx)
        if ntz != 1:
            continue
        # the list goes on to the digests of many nonces, rows and hits never leaving the GPU
        dig, dep2, shallow = miner.digests_many_cuda(tasks, idx, rows)
        assert torch.equal(dep2, dep) and shallow == [0] * len(tasks), name
        assert miner.last_digest_many_entries == [len(x) for x in want]
        got_dig = dig.cpu().numpy().tobytes()
        for j, c in enumerate(cases):
            a, b = want_rows[j], want_rows[j + 1]
            assert got_dig[16 * a:16 * b] == hashlib_of(c.task.nonce, want_idx[a:b])[0], _key(c)
        _, dep3, shallow2 = miner.digests_many_cuda(_scan_tasks(cases, 2), idx, rows, want_digests=False)
        assert torch.equal(dep3, dep) and shallow2 == [sum(1 for _, tz in x if tz == 1) for x in want], name
        if name in CAPPED_SETS:               # launch seams inside the tasks and between them
            n_launches = len(launches_of(windows_of(tasks), 256))
            assert n_launches > 1
            monkeypatch.setenv(CAP_ENV, "256")
            res, idx, dep, rows = miner.scan_batch_cuda(tasks, max_hits=room)
            monkeypatch.delenv(CAP_ENV)
            assert miner.last_scan_many_device_stats.rounds == n_launches, name
            assert res == [(EXHAUSTED, t.k_end) for t in tasks] and rows.tolist() == want_rows, name
            assert (idx.tolist(), dep.tolist()) == (want_idx, want_dep), name
    print(f"scan_batch_cuda {name}: {len(cases)} tasks, {n_hits} hits in 2 calls (N = 1, 3) and the digests of the "
          f"first, {(time.perf_counter() - t0) * 1e3:.1f} ms")
    _still_usable(miner)


# ---- the reference of families M and X ----------------------------------------------------------------
_DEPTHS = {}


def _depths(miner, w):
    """The reference of a task's window, once per process and never changed: the depth of every
    candidate in index order by the digest kernel (W.window_depths_cuda)."""
    if w.name not in _DEPTHS:
        _DEPTHS[w.name] = W.window_depths_cuda(miner, w.nonce, w.wb, w.wbits, w.k_begin, w.k_end)
        assert _DEPTHS[w.name].numel() == w.total
    return _DEPTHS[w.name]


_NOT_VACUOUS = set()


def _reference_is_not_vacuous(miner, call):
    """From the reference alone, before the unit is consulted: every task but the empty one has a hit at
    N = 1 in its first descriptor and in its last, ragged one."""
    if call.name in _NOT_VACUOUS:
        return
    for w, last in zip(call.windows, call.lasts):
        if w.total:
            d = _depths(miner, w)
            first = min(call.group, w.total)
            assert bool((d[:first] >= 1).any()) and bool((d[w.total - last:] >= 1).any()), w.name
    _NOT_VACUOUS.add(call.name)


def _expected(miner, call, ntz):
    """(rows, idx, depths) the call must give at N = ntz: per task the global indices of its candidates
    of depth >= ntz in order (at N = 0 every one, built arithmetically), task after task."""
    dev = _dev(miner)
    idx, dep, counts = [], [], []
    for w in call.windows:
        every, d = W.window_indices_cuda(w.wb, w.wbits, w.k_begin, w.total, dev), _depths(miner, w)
        keep = d >= ntz
        idx.append(every if ntz == 0 else every[keep])
        dep.append(d if ntz == 0 else d[keep])
        counts.append(idx[-1].numel())
    assert ntz != 0 or counts == [w.total for w in call.windows]
    return _cum(counts), torch.cat(idx), torch.cat(dep)


def _scan_whole(miner, call, ntz, m=None):
    """One call with room for every candidate: (idx, depths, rows as a host list)."""
    m = m or miner
    tasks = call.tasks(ntz)
    res, idx, dep, rows = m.scan_batch_cuda(tasks, max_hits=max(call.total if ntz == 0 else call.total // 8, MIN_HITS))
    st = m.last_scan_many_device_stats
    assert res == [(EXHAUSTED, t.k_end) for t in tasks], (call.name, ntz)
    assert (st.rounds, st.candidates) == (1, call.total), (call.name, ntz)
    assert rows.tolist() == m.last_scan_many_device_rows, (call.name, ntz)
    return idx, dep, rows.tolist()


# ---- 2. every group size, many tasks to a launch ------------------------------------------------------
@pytest.mark.parametrize("order", ["descending", "ascending"])
def test_group_sizes(miner, order):
    """Every call of family M at N = 3, 1 and 0, largest first or smallest first."""
    fam = sorted(W.family_m(), key=lambda c: c.total, reverse=order == "descending")
    assert len(fam) == 9
    t0, wrong, lines = time.perf_counter(), [], []
    for c in fam:
        _reference_is_not_vacuous(miner, c)
        for ntz in H_NTZ:
            want_rows, want_idx, want_dep = _expected(miner, c, ntz)
            t1 = time.perf_counter()
            try:
                idx, dep, rows = _scan_whole(miner, c, ntz)
            except distpow.DpowError as e:     # the call's own check refused its list: wrong too, and the walk goes on
                wrong.append(f"{c.name}/N{ntz}: {str(e)[-60:]}")
                continue
            dt = time.perf_counter() - t1
            # (the depths: the digest kernel against itself, it says only that depths and entries belong together)
            if not (rows == want_rows and torch.equal(idx, want_idx) and torch.equal(dep, want_dep)):
                wrong.append(f"{c.name}/N{ntz}: rows {rows}, expected {want_rows}")
            lines.append(f"{c.name}/N{ntz} {want_rows[-1]} hits {dt * 1e3:.2f} ms")
            if ntz == 3 and c.name in ("m512", "m4096"):
                ref = miner.scan_many(c.tasks(3))
                if (idx.tolist(), dep.tolist(), rows) != ([h.global_idx for hs in ref for h in hs],
                                                          [h.tz for hs in ref for h in hs], _cum(map(len, ref))):
                    wrong.append(f"{c.name}/N3: rows {rows}, Miner.scan_many's {_cum(map(len, ref))}")
            del idx, dep, want_idx, want_dep
    print(f"family M {order}: {len(fam)} calls x N = 3, 1, 0 in {time.perf_counter() - t0:.3f} s (the reference "
          f"included where first)\n  " + "\n  ".join(lines))
    assert not wrong, "\n".join([f"{len(wrong)} wrong calls:"] + wrong)
    _still_usable(miner)


# ---- 3. all ten rounds of the prefix --------------------------------------------------------------------
def _x_reference(miner, x, ntz, room):
    """Family X at N = ntz from Miner.scan_cuda (the large task) and one Miner.scan_many call (the 4095
    small ones): (rows, idx, depths, the small tasks' hit lists by array position)."""
    dev = _dev(miner)
    large = x.windows[W.X_LARGE_AT]
    l_idx, l_dep = miner.scan_cuda(large.nonce, ntz, large.wb, large.wbits, large.k_begin, large.k_end, max_hits=room)
    assert miner.last_scan_device_stats.rounds == 1
    tasks = x.tasks(ntz)
    small = miner.scan_many(tasks[:W.X_LARGE_AT] + tasks[W.X_LARGE_AT + 1:])
    small = small[:W.X_LARGE_AT] + [None] + small[W.X_LARGE_AT:]
    counts = [l_idx.numel() if hs is None else len(hs) for hs in small]

    def flat(part, field, dtype):
        return torch.tensor([getattr(h, field) for hs in part for h in hs], dtype=dtype, device=dev)

    idx = torch.cat([flat(small[:W.X_LARGE_AT], "global_idx", torch.int64), l_idx,
                     flat(small[W.X_LARGE_AT + 1:], "global_idx", torch.int64)])
    dep = torch.cat([flat(small[:W.X_LARGE_AT], "tz", torch.uint8), l_dep,
                     flat(small[W.X_LARGE_AT + 1:], "tz", torch.uint8)])
    return _cum(counts), idx, dep, small, l_idx


def test_all_prefix_rounds(miner):
    """Family X: 20416 descriptors, ten rounds, small and large totals alternating across them."""
    x = W.family_x()
    large = x.windows[W.X_LARGE_AT]
    t0 = time.perf_counter()
    want_rows, want_idx, want_dep, small, l_idx = _x_reference(miner, x, 3, 1 << 20)
    t_ref3 = time.perf_counter() - t0
    # Not vacuous, from the reference alone: hits in at least nine of the ten rounds' descriptor ranges.
    # Descriptor d of the large task is descriptor 2047 + d of the launch; small task j is descriptor j
    # before it and j + 16320 behind it (tests/test_scan_many_dev_walk_cases.py).
    local = ((l_idx >> 8) << large.rbits) | (l_idx & ((1 << large.rbits) - 1))
    per_round = torch.bincount((W.X_LARGE_AT + (local - (large.k_begin << large.rbits)) // x.group) // ROUND,
                               minlength=10).tolist()
    for j, hs in enumerate(small):
        if hs is not None:
            per_round[(j if j < W.X_LARGE_AT else j + large.n_blocks - 1) // ROUND] += len(hs)
    assert len(per_round) == 10 and sum(1 for n in per_round if n) >= 9, per_round

    tasks = x.tasks(3)
    t1 = time.perf_counter()
    res, idx, dep, rows = miner.scan_batch_cuda(tasks)
    t_scan3 = time.perf_counter() - t1
    st = miner.last_scan_many_device_stats
    assert (st.rounds, st.candidates) == (1, 1 << 28)
    assert res == [(EXHAUSTED, t.k_end) for t in tasks]
    assert rows.tolist() == want_rows == miner.last_scan_many_device_rows
    assert torch.equal(idx, want_idx) and torch.equal(dep, want_dep)
    a, b = want_rows[W.X_LARGE_AT], want_rows[W.X_LARGE_AT + 1]
    assert torch.equal(idx[a:b], l_idx) and b - a > 60000          # the large task's segment is Miner.scan_cuda's

    t1 = time.perf_counter()
    dig, dep2, shallow = miner.digests_many_cuda(tasks, idx, rows)
    t_dig = time.perf_counter() - t1
    assert torch.equal(dep2, dep) and shallow == [0] * len(tasks)
    assert miner.last_digest_many_entries == [q - p for p, q in zip(want_rows, want_rows[1:])]
    got_dig, n_small = dig.cpu().numpy().tobytes(), 0
    for j, hs in enumerate(small):
        if hs:
            p, q = want_rows[j], want_rows[j + 1]
            assert got_dig[16 * p:16 * q] == hashlib_of(tasks[j].nonce, [h.global_idx for h in hs])[0], j
            n_small += len(hs)
    assert n_small >= 100
    n3 = want_rows[-1]
    del dig, dep2, idx, dep, want_idx, want_dep

    # N = 1: 1.7e7 entries, every total of every round dense
    t1 = time.perf_counter()
    want_rows, want_idx, want_dep, small, l_idx = _x_reference(miner, x, 1, x.total // 8)
    t_ref1 = time.perf_counter() - t1
    tasks = x.tasks(1)
    t1 = time.perf_counter()
    res, idx, dep, rows = miner.scan_batch_cuda(tasks, max_hits=x.total // 8)
    t_scan1 = time.perf_counter() - t1
    assert res == [(EXHAUSTED, t.k_end) for t in tasks]
    assert rows.tolist()[-1] == want_rows[-1] == idx.numel() > 16_000_000   # 2^24 expected, sigma 4000
    assert rows.tolist() == want_rows and torch.equal(idx, want_idx) and torch.equal(dep, want_dep)
    print(f"family X: N = 3 {n3} hits by round {per_round}: references {t_ref3:.3f} s, call "
          f"{t_scan3 * 1e3:.2f} ms, digests_many_cuda {t_dig * 1e3:.2f} ms; N = 1 {idx.numel()} hits: references "
          f"{t_ref1:.3f} s, call {t_scan1 * 1e3:.2f} ms; {time.perf_counter() - t0:.3f} s in all")
    _still_usable(miner)


# ---- 4. stale words of a slot -----------------------------------------------------------------------------
def test_stale_slot_words(miner):
    """A short ragged descriptor in a slot that a dense 16384-index descriptor filled on the same
    context.  (The references come from the session's context, the calls from a fresh one.)"""
    c = W.family_m_call("m512")
    _reference_is_not_vacuous(miner, c)
    alone = W.ScanCall("m512/t2 alone", 256, (c.windows[2],), (96,))
    want = {(call.name, ntz): _expected(miner, call, ntz) for call, ntz in ((c, 3), (alone, 3), (alone, 1))}
    assert want[alone.name, 1][0][-1] >= 1
    dense = ScanTask(b"\x01\x02\x03\x04", 0, 0, 0, 1, 1 + ((2 * 16384 * 4096) >> 8))
    blocks, = launches_of(windows_of([dense]))
    assert len(blocks) == 8192 and all(hi - lo == 16384 for _, lo, hi in blocks)
    t0 = time.perf_counter()
    with distpow.Miner(0) as m:
        res, idx, _, rows = m.scan_batch_cuda([dense], max_hits=1 << 27, want_depths=False)
        assert res == [(EXHAUSTED, dense.k_end)] and rows.tolist() == [0, 1 << 27]
        assert torch.equal(idx, W.window_indices_cuda(0, 0, 1, 1 << 27, _dev(m)))
        del idx
        for call, ntz in ((c, 3), (alone, 3), (alone, 1)):
            idx, dep, rows = _scan_whole(miner, call, ntz, m)
            want_rows, want_idx, want_dep = want[call.name, ntz]
            assert rows == want_rows and torch.equal(idx, want_idx) and torch.equal(dep, want_dep), (call.name, ntz)
        _still_usable(m)
    print(f"dense 2^27 at group 16384, then m512 at N = 3 and its 96-index task alone: {time.perf_counter() - t0:.3f} s")
    _still_usable(miner)


# ---- 5. page cuts ---------------------------------------------------------------------------------------------
def _walk_pages(miner, tasks, hits, max_hits, cap=0, limit=80):
    """Pages `tasks` (whose complete hit lists are the numpy arrays `hits`) with max_hits: every page's
    statuses, k_done, rows and list are call_model's.  -> (pages as [(results, rows)], per-task lists)."""
    k = [t.k_begin for t in tasks]
    got, pages = [[] for _ in tasks], []
    while True:
        page = [ScanTask(t.nonce, t.num_trailing_zeros, t.worker_byte, t.worker_bits, k[i], t.k_end)
                for i, t in enumerate(tasks)]
        rest = [h[np.searchsorted(h, np.uint64(k[i] << 8)):] for i, h in enumerate(hits)]
        e_res, e_rows, e_seg = call_model(page, rest, max_hits, cap)
        res, idx, dep, rows = miner.scan_batch_cuda(page, max_hits=max_hits)
        assert res == e_res and rows.tolist() == e_rows == miner.last_scan_many_device_rows, len(pages)
        assert np.array_equal(idx.cpu().numpy().astype(np.uint64), np.concatenate(e_seg)), len(pages)
        pages.append((res, e_rows))
        for i in range(len(tasks)):
            got[i].append(e_seg[i])
            k[i] = res[i][1]
        assert len(pages) < limit
        if all(r == EXHAUSTED for r, _ in res):
            return pages, [np.concatenate(g) for g in got]


def test_cut_in_a_later_launch(miner, monkeypatch):
    """Launches of 8192 candidates, room for 16384 entries, N = 0.  The first launch is 156 short of
    its budget (a task of 100, then a long task cut at a multiple of 256) and the second 42 (the next
    task is 96 long), so the third begins with a descriptor of 96 that fits the 198 entries of room
    left and goes on with whole ones that do not: the place launch runs with a non-zero base over
    fewer descriptors than the mask launch had."""
    tasks = [ScanTask(b"\x05" * 4, 0, 200, 8, 33, 33 + 100), ScanTask(b"\x06" * 55, 0, 77, 8, 65001, 65001 + 16086),
             ScanTask(b"\x07" * 56, 0, 5, 3, 255, 258), ScanTask(b"\x08" * 63, 0, 2, 3, 7, 7 + 1029)]
    hits = [np.array([k << 8 | tb for k in range(t.k_begin, t.k_end) for tb in W.thread_bytes(t.worker_byte, t.worker_bits)],
                     dtype=np.uint64) for t in tasks]
    assert [len(h) for h in hits] == [100, 16086, 96, 32928] and 2.9 * MIN_HITS < sum(map(len, hits)) < 3.1 * MIN_HITS
    launches = launches_of(windows_of(tasks), 8192)
    assert [sum(hi - lo for _, lo, hi in b) for b in launches[:3]] == [8192 - 156, 8192 - 42, 96 + 7936]
    assert launches[2][0] == (2, 255 << 5, 258 << 5) and launches[2][1][0] == 3
    monkeypatch.setenv(CAP_ENV, "8192")
    t0 = time.perf_counter()
    pages, got = _walk_pages(miner, tasks, hits, MIN_HITS, cap=8192)
    dt = time.perf_counter() - t0
    # the first page: three launches, the third cut behind its first descriptor
    assert pages[0] == ([(EXHAUSTED, 133), (EXHAUSTED, 65001 + 16086), (EXHAUSTED, 258), (MORE, 7)],
                        [0, 100, 16186, 16282, 16282])
    assert all(np.array_equal(g, h) for g, h in zip(got, hits)) and len(pages) >= 4
    print(f"cap 8192, max_hits 16384 at N = 0: {len(pages)} pages, rows {[r for _, r in pages]}, {dt * 1e3:.1f} ms")
    _still_usable(miner)


def test_cut_inside_a_task_at_a_large_group(miner):
    """Family M's g = 2048 call at N = 1 in pages: every page is a new call from the tasks' k_done whose
    launch, group and cut are its own."""
    c = W.family_m_call("m2048")
    _reference_is_not_vacuous(miner, c)
    tasks = c.tasks(1)
    want_rows, want_idx, want_dep = _expected(miner, c, 1)
    flat = want_idx.cpu().numpy().astype(np.uint64)
    hits = [flat[a:b] for a, b in zip(want_rows, want_rows[1:])]
    lines = []
    for max_hits in (MIN_HITS, MIN_HITS + 2047):
        t0 = time.perf_counter()
        pages, got = _walk_pages(miner, tasks, hits, max_hits)
        dt = time.perf_counter() - t0
        assert all(np.array_equal(g, h) for g, h in zip(got, hits))
        inside = {i for res, _ in pages for i, (st, kd) in enumerate(res) if st == MORE and tasks[i].k_begin < kd < tasks[i].k_end}
        assert {0, 3} <= inside, inside          # a cut strictly inside t0 and one inside t3
        lines.append(f"max_hits {max_hits}: {len(pages)} pages, cuts inside tasks {sorted(inside)}, {dt * 1e3:.1f} ms")
    t0 = time.perf_counter()
    idx, dep, rows = miner.scan_many_cuda(tasks, max_hits=MIN_HITS)
    assert rows.tolist() == want_rows and torch.equal(idx, want_idx) and torch.equal(dep, want_dep)
    print(f"m2048 at N = 1, {want_rows[-1]} hits: " + "; ".join(lines) +
          f"; scan_many_cuda {(time.perf_counter() - t0) * 1e3:.1f} ms")
    _still_usable(miner)
