"""GPU: the generic kernel of the batched search (csrc/md5_batch.hip, md5_batch.h, driven by
batch.cpp) against walked all-hits lists that do not come from this library.

tests/test_gpu_batch.py compares the first hit of each window with the oracle; a candidate behind
a chunk-length change, a lane on the other side of the block-count change inside its wave, a true
N = 9 hit the recheck drops or a hit on a seam of the round plan can be wrong there without a test
seeing it.  Here every hit of every window is compared, by equality, with lists from hashlib, the
C oracle or the committed fixtures (tests/_batch_walk_cases.py; tests/test_batch_walk_cases.py
shows on the CPU that the families reach what they name):

  A  N = 1, p = 54 - a: the block count changes from one to two at edge(a) = 256**a, placed at
     every k position of a 64-lane wave for worker_bits 3..8 (the per-lane select behind the
     second block, the bit length and the pad of each lane's own chunk length).
  B  N = 1, worker_bits 8 (a k is one candidate, so the walk decides every candidate on the GPU):
     every p = 0..63, with zero, one and two whole nonce blocks, on 64 k across each edge(a) and
     on the last 64 k below DPOW_K_LIMIT; the controls are family A's windows at p = 53 - a and
     55 - a, where no lane and every lane takes the second block.
  C  every listed N >= 8 hit of every layout (tests/golden/layout_deep_hits.json) and the deep
     hits of pow_golden.json: N = 8, N = 9 and N = tz + 1 round the hit at worker_bits 0, 3 and 8
     (the full D-word filter and the trailing_zero_nibbles recheck behind it).
  D  one, two and three 2^20-candidate tasks at N = 1 and 2: every workgroup of round 0 works on
     the same few tasks, most hold a hit and race on the atomicMin; the answer is the oracle's
     first hit.
  E  a hit on the last index of a workgroup's group and on the first of the next, on the last
     index of round 0's slice and the first of round 1's, and on the window's last k, with no hit
     before it by the oracle, at R = 1 and R = 256.

Every test prints its wall time and its search_batch calls (pytest -s) and ends with one golden
search on the same context.  On an MI355X the 25 tests take 2.7 s together, 1.6 s of it opening the
context and most of the rest hashlib building the lists (once per process).  Per test: a family-A
walk 10-11 ms for its 15-18 search_batch calls of at most 252 tasks, a family-B walk 4 ms for 10-13
calls of at most 192, a control 2-3 ms for 4 calls of 28, family C 0.4-0.9 ms for its one call of
639 tasks, family D 4-5 ms for 16 calls with the oracle's scans, family E 0.7 ms for 5 calls of 64.

Shown to bite on three deliberately wrong kernels (built outside the tree, one run each): every
lane taking the second block's state when any lane of its wave needs it fails A[0-6] and B[0-6]
and passes the controls, while tests/test_gpu_batch.py passes on it; a hit test without the
trailing_zero_nibbles recheck fails C[n9] and C[next]; the bit length taken from the wave's first
lane fails A[0-6], B[0-6] and both controls.
"""
import time

import pytest

import _batch_walk_cases as W
from distpow import FOUND

pytestmark = pytest.mark.gpu


def _still_usable(miner):
    r = miner.search([1, 2, 3, 4], 3, 0, 0, 0, 1 << 12)
    assert (r.status, list(r.secret)) == (FOUND, [97])


def _walk_equals(miner, cases, label):
    """The walked hits of every case's window are hashlib's list."""
    sb = W.Counted(miner)
    t = time.perf_counter()
    hits = W.walk_batch(sb, [c.task for c in cases], 1)
    dt = time.perf_counter() - t
    for c, h in zip(cases, hits):
        assert h == c.hits, (c.a, c.p, c.d, c.task)
    print(f"{label}: {len(cases)} tasks, {sum(map(len, hits))} hits walked in {sb.calls} search_batch calls, "
          f"{dt * 1e3:.0f} ms")
    _still_usable(miner)


@pytest.mark.parametrize("a", range(7))
def test_a_block_count_changes_inside_a_wave(miner, a):
    _walk_equals(miner, [c for c in W.family_a() if c.a == a], f"A edge 256^{a}")


@pytest.mark.parametrize("a", range(8))
def test_b_every_byte_position_at_every_edge(miner, a):
    _walk_equals(miner, [c for c in W.family_b() if c.a == a], f"B edge {'top' if a == W.TOP else f'256^{a}'}")


@pytest.mark.parametrize("name", ["never", "always"])
def test_b_controls(miner, name):
    _walk_equals(miner, W.family_b_controls()[name], f"B control, {name} two blocks")


@pytest.mark.parametrize("kind", ["n8", "n9", "next"])
def test_c_deep_hits_of_every_layout(miner, kind):
    tasks = [t for t in W.family_c() if t.kind == kind]
    t0 = time.perf_counter()
    res = miner.search_batch([t.task for t in tasks])
    dt = time.perf_counter() - t0
    for t, r in zip(tasks, res):
        assert W.got(r) == t.expected, (t, r)
    print(f"C {kind}: {len(tasks)} tasks ({sum(t.expected[0] == FOUND for t in tasks)} with a hit) in 1 search_batch "
          f"call, {dt * 1e3:.1f} ms")
    _still_usable(miner)


@pytest.mark.parametrize("b", [1, 2, 3])
def test_d_all_rows_on_one_task(miner, oracle, b):
    t0, calls = time.perf_counter(), 0
    for ntz in (1, 2):
        for batch in W.family_d()[b, ntz]:
            expected = [W.oracle_expect(oracle, t) for t in batch]
            assert all(e[0] == FOUND for e in expected)
            res = miner.search_batch(batch)
            calls += 1
            assert [W.got(r) for r in res] == expected, (batch, res)
            if b == 1:
                assert miner.last_batch_stats.rounds == 1
    print(f"D B = {b}: {calls} search_batch calls in {(time.perf_counter() - t0) * 1e3:.1f} ms "
          f"(the oracle's scans included)")
    _still_usable(miner)


@pytest.mark.parametrize("wbits", [8, 0])
def test_e_a_hit_on_each_seam(miner, oracle, wbits):
    cases = W.family_e(oracle, wbits)
    t0 = time.perf_counter()
    for c in cases:
        res = miner.search_batch(c.batch)
        assert [W.got(r) for r in res] == c.expected, (c.seam, c.probe, res[W.E_PROBE])
        assert res[W.E_PROBE].global_idx == c.hit
        rounds = miner.last_batch_stats.rounds
        assert rounds >= 2 if c.offset >= c.slice else rounds == 1, (c.seam, c.offset, c.slice, rounds)
    print(f"E R = {256 >> wbits}: {len(cases)} seams (slice {cases[0].slice}, group {cases[0].group}), "
          f"{len(cases)} search_batch calls in {(time.perf_counter() - t0) * 1e3:.1f} ms")
    _still_usable(miner)
