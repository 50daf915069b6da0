"""GPU: the scan and census kernels (csrc/md5_scan.hip, md5_scan_many.hip and the depth sink of
md5_census.h that md5_census.hip and md5_census_many.hip share) against hashlib at every layout
edge.

Each of the three carries its own copy of the loop round batch_candidate_words_at and
batch_md5_block: the clamp of a partial wave's inactive lanes to the range's last index, the
second block behind __any(nblk == 2u), the per-lane select of its state, and the hit or depth sink.
Their own test files hash dense windows whose waves are one-block or two-block throughout, on k
below 2^17.  Here the case families of tests/_batch_walk_cases.py are compared by equality -- a
scan returns every hit and a census every count in one call, so there is no walk -- with the lists
its depth reference derives from hashlib (tests/test_listing_walk_cases.py shows on the CPU that the
families reach what they name and that every window starts a workgroup's first wave):

  A  p = 54 - a: the block count changes from one to two at edge(a) = 256**a, at every k position
     of a 64-lane wave for worker_bits 3..8.
  B  worker_bits 8: every p = 0..63 with zero, one and two whole nonce blocks on 64 k across each
     edge(a) and on the last 64 k below DPOW_K_LIMIT (7-byte chunks, the pad in the `hi` word); the
     controls are family A's windows with no lane and with every lane two-block.
  F  worker_bits 0, 1 and 2 at every edge(a) and on the last three k below DPOW_K_LIMIT, where the
     local indices reach 2^63 - 257: p = 54 - a (48 at the top), 0, 47, 55 and 63.
  G  one partial wave that ends with the first two-block k: one-block lanes below the edge, the
     edge's lanes and the clamped inactive lanes two-block; the controls end before the edge.

Per (kernel, family, edge): Miner.scan_many and Miner.census_many in one call for the edge's tasks,
Miner.scan and Miner.census in one call (one launch) per window; the scans at N = 1 and at N = 3,
where the trailing_zero_nibbles recheck runs behind the D-word prefilter.  Miner.search_batch walks
families F and G too (walk_batch), which the batched search kernel had not seen either.  Every test
prints its wall time and calls (pytest -s) and ends with one golden search on the same context.

On an MI355X the 178 tests take 4.0 s together, 1.6 s of it opening the context and 1.3 s inside
the tests, most of that hashlib building the lists (once per process, in the first test that
needs a family).  Per test, the lists included where it is the first: scan_many 29-32 ms for
family A's 252 tasks, 11 ms for B's 192 (112 ms at one edge), 8-11 ms for F's 30, up to 10 ms for
G's 228, its two calls together; census_many 4-18 ms (A), 2 ms (B, F, G), one call; scan 11-22 ms
for A's 504 one-launch calls, 7 ms for B's 384, 2-3 ms for F's 60, 8 ms for G's 456; census 8-11 ms
for A's 252 calls, 5 ms (B), 2 ms (F), 5 ms (G); a search_batch walk 10-17 ms (F, 3-4 calls) and
3 ms (G, 8-11 calls).

Shown to bite on six deliberately wrong kernels (built outside the tree, one run each).  Every
lane taking the second block's state when any lane of its wave needs it, in each of the three
copies of the loop:
  md5_scan.hip       fails test_scan[A-0..6, B-0..6, G-0..6], passes the other 157 (B-7, both B
                     controls, F and the G controls among them); tests/test_gpu_scan.py passes on it
  md5_scan_many.hip  fails test_scan_many[A-0..6, B-0..6, G-0..6], passes the other 157;
                     tests/test_gpu_scan_many.py passes on it
  md5_census.h       fails test_census[...] and test_census_many[...] of A-0..6, B-0..6, G-0..6,
                     passes the other 136; tests/test_gpu_census.py and test_gpu_census_many.py pass on it
One further mutant per copy: the bit length taken from the wave's first lane (md5_scan.hip) fails
test_scan[A-0..6, B-0..6, G-0..6] and both B controls; the second block hashed only when the
wave's first lane needs it (md5_scan_many.hip) fails test_scan_many[A-0..6, B-0..6, G-0..6]; the
flush's first index built from the low 32 bits of the workgroup's begin (md5_census.h) fails
test_census and test_census_many at every edge from 256^4 (worker_bits 0: 256^3) up and at the
top of the range -- A-4..6, B-4..7, both B controls, F-3..7, G-4..6 and the G controls 4..6 -- and
the existing census files fail on that one too (their committed lists lie above local index 2^32).
Family F fails on no block-select mutant, rightly: at 64 to 256 candidates per k a wave never holds
two k, so F pins the wide partitions and the top of the range, not the select.
"""
import time

import pytest

import _batch_walk_cases as W
from distpow import FOUND, CensusTask, ScanTask

pytestmark = pytest.mark.gpu

PAGE = 1024   # max_hits of a one-window scan: no window has more candidates


def _families():
    ctl = W.family_b_controls()
    return {"A": W.family_a(), "B": W.family_b(), "Bnever": ctl["never"], "Balways": ctl["always"],
            "F": W.family_f(), "G": W.family_g(), "Gctl": W.family_g_controls()}


# (family, a); a control of family B is one set over every edge
SETS = ([("A", a) for a in range(7)] + [("B", a) for a in range(8)] + [("Bnever", None), ("Balways", None)] +
        [("F", a) for a in range(8)] + [("G", a) for a in range(7)] + [("Gctl", a) for a in range(7)])
IDS = [f if a is None else f"{f}-{a}" for f, a in SETS]
WIDE_OR_RAGGED = [(s, i) for s, i in zip(SETS, IDS) if s[0] in ("F", "G", "Gctl")]


def _cases(which):
    fam, a = which
    cases = [c for c in _families()[fam] if a is None or c.a == a]
    assert cases and max((c.task.k_end - c.task.k_begin) << (8 - c.wbits) for c in cases) <= 1024
    return cases


def _still_usable(miner):
    r = miner.search([1, 2, 3, 4], 3, 0, 0, 0, 1 << 12)
    assert (r.status, list(r.secret)) == (FOUND, [97])


def _key(c):
    return (c.a, c.p, c.d, c.task)


@pytest.mark.parametrize("which", SETS, ids=IDS)
def test_scan_many(miner, which):
    """scan_many_kernel: every hit of every window, with its depth and secret, is hashlib's."""
    cases = _cases(which)
    t0, n_hits = time.perf_counter(), 0
    for ntz in (1, 3):
        tasks = [ScanTask(c.task.nonce, ntz, c.task.worker_byte, c.task.worker_bits, c.task.k_begin, c.task.k_end)
                 for c in cases]
        got = miner.scan_many(tasks)
        assert len(got) == len(cases)
        for c, hits in zip(cases, got):
            assert hits == W.scan_hits_of(c, ntz), (ntz,) + _key(c)
        n_hits += sum(map(len, got))
    print(f"scan_many {which}: {len(cases)} tasks, {n_hits} hits in 2 calls (N = 1, 3), "
          f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
    _still_usable(miner)


@pytest.mark.parametrize("which", SETS, ids=IDS)
def test_census_many(miner, which):
    """census_many_kernel: all 33 counts, firsts, first depths and the deepest are hashlib's."""
    cases = _cases(which)
    t0 = time.perf_counter()
    got = miner.census_many([CensusTask(c.task.nonce, c.task.worker_byte, c.task.worker_bits, c.task.k_begin,
                                        c.task.k_end) for c in cases])
    assert len(got) == len(cases)
    for c, census in zip(cases, got):
        assert census == W.census_of(c), _key(c)
    print(f"census_many {which}: {len(cases)} tasks in 1 call, {(time.perf_counter() - t0) * 1e3:.1f} ms")
    _still_usable(miner)


@pytest.mark.parametrize("which", SETS, ids=IDS)
def test_scan(miner, which):
    """scan_kernel: one call and one launch per window, from the window's begin."""
    cases = _cases(which)
    t0, calls = time.perf_counter(), 0
    for c in cases:
        t = c.task
        for ntz in (1, 3):
            hits = miner.scan(t.nonce, ntz, t.worker_byte, t.worker_bits, t.k_begin, t.k_end, PAGE)
            calls += 1
            assert miner.last_scan_stats.launches == 1
            assert hits == W.scan_hits_of(c, ntz), (ntz,) + _key(c)
    print(f"scan {which}: {len(cases)} windows in {calls} calls (N = 1, 3), {(time.perf_counter() - t0) * 1e3:.1f} ms")
    _still_usable(miner)


@pytest.mark.parametrize("which", SETS, ids=IDS)
def test_census(miner, which):
    """census_kernel: one call and one launch per window, from the window's begin."""
    cases = _cases(which)
    t0 = time.perf_counter()
    for c in cases:
        t = c.task
        census = miner.census(t.nonce, t.worker_byte, t.worker_bits, t.k_begin, t.k_end)
        assert miner.last_census_stats.launches == 1
        assert census == W.census_of(c), _key(c)
    print(f"census {which}: {len(cases)} windows in {len(cases)} calls, {(time.perf_counter() - t0) * 1e3:.1f} ms")
    _still_usable(miner)


@pytest.mark.parametrize("which", [s for s, _ in WIDE_OR_RAGGED], ids=[i for _, i in WIDE_OR_RAGGED])
def test_search_batch_walk(miner, which):
    """batch_kernel on the families tests/test_gpu_batch_walk.py does not have: the top of the k
    range at 256 candidates per k, and the ragged waves."""
    cases = _cases(which)
    sb = W.Counted(miner)
    t0 = time.perf_counter()
    hits = W.walk_batch(sb, [c.task for c in cases], 1)
    dt = time.perf_counter() - t0
    for c, h in zip(cases, hits):
        assert h == c.hits, _key(c)
    print(f"search_batch {which}: {len(cases)} tasks, {sum(map(len, hits))} hits walked in {sb.calls} calls, "
          f"{dt * 1e3:.1f} ms")
    _still_usable(miner)
