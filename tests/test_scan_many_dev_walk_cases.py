"""Families M and X of tests/_batch_walk_cases.py are what they claim under the batched device scan's
own planner -- shown through distpow.census_plan alone (_scan_many_dev_model.launches_of), the restated
wave steps (scan_dev_wave_steps) and hashlib, no GPU.  tests/test_gpu_scan_many_dev_walk.py runs them
against lists from other kernels, so a call that missed its group, its ragged descriptors or its
prefix rounds would pin nothing.

That walk also runs the sets of tests/test_gpu_listing_walk.py (families A, B, F, G and their controls).
tests/test_listing_walk_cases.py's test_every_window_is_one_descriptor_from_its_begin already shows them
under census_plan -- every task of a set is one descriptor from its window's begin, family F's whole
descriptors from it -- and census_plan is this unit's planner (csrc/scan_many_dev.cpp runs
many_next), so nothing of that is repeated here; its vacuity conditions for those sets are
test_the_device_scan_tests_cannot_pass_vacuously's."""
import collections
import hashlib
import os
import random
import re

import distpow
from distpow import EXHAUSTED, MORE, ScanTask
from distpow._lib import DPOW_BATCH_MAX

import _batch_walk_cases as W
from _scan_many_dev_model import call_model, launches_of, windows_of
from test_listing_walk_cases import CSRC, _constant

ROUND = W.SCAN_DEV_PREFIX_ROUND


def _launch(call):
    """The call's one launch as [(task, i_begin, i_end)], after the checks every call shares."""
    launches = launches_of(windows_of(call.tasks(1)))
    assert len(launches) == 1, call.name
    blocks = launches[0]
    assert len(blocks) == call.n_descriptors, call.name
    assert [b[0] for b in blocks] == sorted(b[0] for b in blocks)          # task after task
    per_task = collections.defaultdict(list)
    for task, lo, hi in blocks:
        per_task[task].append((lo, hi))
    for j, w in enumerate(call.windows):
        mine = per_task[j]
        assert len(mine) == w.n_blocks, w.name
        if not mine:
            assert w.total == 0 and call.lasts[j] == 0
            continue
        assert mine[0][0] == w.k_begin << w.rbits and mine[-1][1] == w.k_end << w.rbits, w.name
        assert all(a[1] == b[0] for a, b in zip(mine, mine[1:])), w.name
        assert all(hi - lo == call.group for lo, hi in mine[:-1]), w.name   # whole descriptors: exactly g
        assert mine[-1][1] - mine[-1][0] == call.lasts[j], w.name
    return blocks


def test_the_constants_are_the_sources():
    assert _constant("md5_scan_many_dev.hip", "kScanManyPrefixPer") * W.SCAN_DEV_STEP == ROUND == 2048
    src = open(os.path.join(CSRC, "md5_scan_many.h")).read()
    assert re.search(r"kScanManyMaxBlocks = \(uint32_t\)\(kBatchCap / kBatchMaxGroup\) \+ DPOW_BATCH_MAX;", src)
    assert W.SCAN_DEV_SLICE // W.SCAN_DEV_MAX_GROUP + DPOW_BATCH_MAX == W.SCAN_MANY_MAX_BLOCKS == 20480 == 10 * ROUND
    assert re.search(r"kScanManyDevSlotWords = kBatchMaxGroup / 64;",
                     open(os.path.join(CSRC, "md5_scan_many_dev.h")).read())
    assert W.X_TASKS == DPOW_BATCH_MAX and distpow.SCAN_DEVICE_MIN_HITS == W.SCAN_DEV_MAX_GROUP


def test_family_m_is_one_launch_at_every_group_size():
    fam = W.family_m()
    assert [c.name for c in fam] == [f"m{g}" for g in W.H_GROUPS] + ["b2047", "b2048", "b2049"]
    assert len({w.nonce for c in fam for w in c.windows}) == sum(len(c.windows) for c in fam)
    for c in fam:
        assert W.scan_dev_geometry(c.total)[0] == c.group, c.name           # the launch's group is the call's
        blocks = _launch(c)
        for w in c.windows:
            assert w.k_begin % 2 == 1, w.name
            assert w.wb != 0 if w.wbits else w.wb == 0, w.name
            assert w.wb < 1 << w.wbits
        rounds = -(-len(blocks) // ROUND)
        steps = [W.scan_dev_wave_steps(n) for n in c.lasts]
        if c.name.startswith("m"):
            g, s = c.group, 1 if c.group == 512 else c.group // 512
            assert 4096 * g <= c.total < 8192 * g and c.total == 4096 * g + 256 * s + 673
            assert [(w.wbits, len(w.nonce), w.total) for w in c.windows] == \
                [(3, 4, 1500 * g + 256 * s + 96), (0, 9, 0), (3, 55, 96), (0, 56, 2000 * g + 256), (8, 63, 596 * g + 225)]
            assert c.lasts == (256 * s + 96, 0, 96, 256, 225)
            assert [w.n_blocks for w in c.windows] == [1501, 0, 1, 2001, 597]
            assert (len(blocks), rounds) == (4100, 3) and len(blocks) > 4096
            # unequal step counts, and a partial last step where claimed
            assert steps == [[(s + 1, 64), (s + 1, 32), (s, 64), (s, 64)], [(0, 0)] * 4,
                             [(1, 64), (1, 32), (0, 0), (0, 0)], [(1, 64)] * 4, [(1, 64), (1, 64), (1, 64), (1, 33)]]
            assert W.scan_dev_wave_steps(g) == [(g // 256, 64)] * 4 and s + 1 <= g // 256
            assert distpow.batch_candidate(c.windows[3].nonce, 0, 0, c.windows[3].k_begin << 8)[2] == 2
            # the round boundaries behind descriptors 2047 and 4095 lie inside t3 and t4
            assert blocks[2047][0] == blocks[2048][0] == 3 and blocks[4095][0] == blocks[4096][0] == 4
        else:
            n = int(c.name[1:])
            assert c.group == 256 and c.total < 1 << 20 and len(blocks) == n and rounds == -(-n // 2048)
            assert [(w.wbits, len(w.nonce), w.n_blocks) for w in c.windows] == [(3, 4, 1000), (0, 56, 500), (8, 63, n - 1500)]
            assert c.lasts == (96, 256, 225)
            assert steps == [[(1, 64), (1, 32), (0, 0), (0, 0)], [(1, 64)] * 4, [(1, 64), (1, 64), (1, 64), (1, 33)]]
            if n == 2049:       # the second round begins inside the third task, with its ragged descriptor
                assert blocks[2047][0] == blocks[2048][0] == 2 and blocks[2048][1] != c.windows[2].k_begin
                assert blocks[2048][2] - blocks[2048][1] == 225


def test_family_x_is_ten_prefix_rounds():
    x = W.family_x()
    assert len(x.windows) == DPOW_BATCH_MAX and x.total == 1 << 28 == W.SCAN_DEV_SLICE
    assert W.scan_dev_geometry(x.total) == (16384, 16384) and x.group == 16384
    blocks = _launch(x)
    assert len(blocks) == x.n_descriptors == 20416 < W.SCAN_MANY_MAX_BLOCKS
    assert -(-len(blocks) // ROUND) == 10
    large = x.windows[W.X_LARGE_AT]
    assert W.X_LARGE_AT == 2047 and large.total == (1 << 28) - 4095 * 256 and large.n_blocks == 16321
    assert x.lasts[W.X_LARGE_AT] == 256 and large.k_begin % 2 == 1 and (large.wbits, large.wb) == (3, W.H_WB)
    # the large task's first descriptor is descriptor 2047, the last of the first round
    assert blocks[2047][:2] == (2047, large.k_begin << large.rbits) and blocks[2046][0] == 2046
    assert blocks[2047 + 16320] == (2047, (large.k_end << large.rbits) - 256, large.k_end << large.rbits)
    assert blocks[2047 + 16321][0] == 2048
    small = [w for j, w in enumerate(x.windows) if j != W.X_LARGE_AT]
    assert len({w.nonce for w in x.windows}) == DPOW_BATCH_MAX
    for j, w in enumerate(x.windows):
        if j != W.X_LARGE_AT:
            assert (w.wbits, w.wb, len(w.nonce), w.k_begin, w.k_end, x.lasts[j]) == (0, 0, 4, j % 300, j % 300 + 1, 256)
    assert len(small) == 4095
    # per round: rounds 0 and 9 hold small tasks alone (but for descriptor 2047), rounds 1 to 7 whole descriptors
    per_round = [sum(hi - lo for _, lo, hi in blocks[r * ROUND:(r + 1) * ROUND]) for r in range(10)]
    assert per_round[0] == 2047 * 256 + 16384 and per_round[9] == (20416 - 9 * 2048) * 256
    assert per_round[1:8] == [2048 * 16384] * 7 and sum(per_round) == 1 << 28


def _first_hit(w, ntz, lo, hi):
    """The first local index of [lo, hi) whose candidate has depth >= ntz by hashlib, or None."""
    base, zeros, R = hashlib.md5(w.nonce), "0" * ntz, 1 << w.rbits
    for i in range(lo, hi):
        h = base.copy()
        h.update(W.secret_of(((i >> w.rbits) << 8) | (w.wb << w.rbits) | (i & (R - 1))))
        if h.hexdigest().endswith(zeros):
            return i
    return None


def test_the_many_walk_cannot_pass_vacuously():
    """Where hashlib reaches.  Family M: every task other than the empty one has a hit at N = 1 in its
    last descriptor (96 to 8288 candidates: none with probability 2e-3 at the most, hence the seed) and
    in the first step of its first.  Family X: rounds 0 and 9 of the prefix are small tasks alone, about
    2000 x 256 candidates each and 125 of depth >= 3; the rounds between hold 3e7 candidates each, which
    the GPU test counts from its reference before it consults the unit."""
    for c in W.family_m():
        for w, last in zip(c.windows, c.lasts):
            if w.total == 0:
                continue
            lo, hi = w.k_begin << w.rbits, w.k_end << w.rbits
            assert _first_hit(w, 1, hi - last, hi) is not None, w.name
            assert _first_hit(w, 1, lo, lo + min(W.SCAN_DEV_STEP, w.total)) is not None, w.name
    x = W.family_x()
    for r, tasks in ((0, range(0, 2047)), (9, range(9 * 2048 - 16320, 4096))):
        assert all(j != W.X_LARGE_AT for j in tasks)
        assert any(_first_hit(x.windows[j], 3, x.windows[j].k_begin << 8, x.windows[j].k_end << 8) is not None
                   for j in tasks), r


def _call_model_by_loops(tasks, hits, max_hits, cap):
    """call_model as first written: a loop over every hit for every descriptor."""
    n = len(tasks)
    rbits = [distpow.remainder_bits(t.worker_bits) for t in tasks]
    done = [t.k_begin << r for t, r in zip(tasks, rbits)]
    locs = [[((g >> 8) << rbits[i]) | (g & ((1 << rbits[i]) - 1)) for g in hits[i]] for i in range(n)]
    room = max_hits
    for blocks in launches_of(windows_of(tasks), cap):
        for task, lo, hi in blocks:
            c = sum(1 for x in locs[task] if lo <= x < hi)
            if c > room:
                break
            room -= c
            done[task] = hi
        else:
            continue
        break
    segments = [[g for g, x in zip(hits[i], locs[i]) if x < done[i]] for i in range(n)]
    rows = [0]
    for s in segments:
        rows.append(rows[-1] + len(s))
    results = [(EXHAUSTED, t.k_end) if done[i] == t.k_end << rbits[i] else (MORE, done[i] >> rbits[i])
               for i, t in enumerate(tasks)]
    return results, rows, segments


def test_call_model_bisects_to_what_the_loops_give():
    """_scan_many_dev_model.call_model finds a descriptor's hits by bisection, so that the walk can page
    lists of 5e5 hits; on random sparse and dense lists it is the plain double loop's answer, for lists
    and for numpy arrays."""
    import numpy as np
    rnd = random.Random(W.M_SEED)
    tasks = [ScanTask(b"ab", 1, 5, 3, 7, 207), ScanTask(b"", 1, 0, 0, 9, 9), ScanTask(b"c", 1, 0, 0, 3, 23),
             ScanTask(b"d", 1, 200, 8, 1, 1500)]
    every = [[k << 8 | tb for k in range(t.k_begin, t.k_end) for tb in W.thread_bytes(t.worker_byte, t.worker_bits)]
             for t in tasks]
    cuts = set()
    # 6400, 0, 5120 and 1499 candidates: room for 3000, 7000 and 12000 of them ends in tasks 0, 2 and 3
    for rate, max_hits, cap in ((1.0, 3000, 0), (1.0, 7000, 2048), (1.0, 12000, 0), (0.3, 900, 0), (0.3, 512, 1024),
                                (0.05, 100, 256), (0.3, 10 ** 6, 0)):
        hits = [[g for g in e if rnd.random() < rate] for e in every]
        want = _call_model_by_loops(tasks, hits, max_hits, cap)
        assert call_model(tasks, hits, max_hits, cap) == want
        res, rows, seg = call_model(tasks, [np.array(h, dtype=np.uint64) for h in hits], max_hits, cap)
        assert (res, rows, [s.tolist() for s in seg]) == want
        cuts.add(tuple(r for r, _ in res))
    assert {(MORE, EXHAUSTED, MORE, MORE), (EXHAUSTED, EXHAUSTED, MORE, MORE), (EXHAUSTED,) * 3 + (MORE,),
            (EXHAUSTED,) * 4} <= cuts
