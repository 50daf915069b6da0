"""The depth reference and families F and G of tests/_batch_walk_cases.py are what they claim, and
the windows of families A, B and G land on the wave boundaries they were built for under the scan's
and the census's own planners -- shown from hashlib, the host copy of the kernels' candidate
assembly (distpow.batch_candidate) and the planners (distpow.scan_plan, census_plan, scan_slice)
alone, no GPU.  tests/test_gpu_listing_walk.py compares the scan and census kernels with these
lists by equality, so a family that misses its edge, or a reference that is wrong, would pin
nothing."""
import collections

import distpow
from distpow._lib import DPOW_BATCH_MAX, DPOW_K_LIMIT

import _batch_walk_cases as W

MIN_GROUP = 256   # local indices of the smallest workgroup range (csrc/batch.h kBatchMinGroup)


def _rbits(c):
    return 8 - c.wbits


def _nblk(c, k):
    """Block count of the window's candidates at k, from the host copy of the kernel's assembly."""
    t = c.task
    return distpow.batch_candidate(t.nonce, t.worker_byte, t.worker_bits, k << _rbits(c))[2]


def _families():
    ctl = W.family_b_controls()
    return {"A": W.family_a(), "B": W.family_b(), "B never": ctl["never"], "B always": ctl["always"],
            "F": W.family_f(), "G": W.family_g(), "G control": W.family_g_controls()}


def test_family_f_is_wide_partitions_at_every_edge_and_at_the_top():
    cases = W.family_f()
    assert len(cases) == 8 * 3 * 5 * 2 <= DPOW_BATCH_MAX
    keys = collections.Counter((c.a, c.wbits, c.p) for c in cases)
    assert set(keys) == {(a, wbits, p) for a in range(8) for wbits in (0, 1, 2) for p in W.f_positions(a)}
    assert set(keys.values()) == {2}                                   # nonce lengths p and p + 64
    assert {(c.a, c.wbits) for c in cases} == {(a, wbits) for a in range(8) for wbits in (0, 1, 2)}
    assert sum((c.task.k_end - c.task.k_begin) << _rbits(c) for c in cases) <= 240 * 1024
    for c in cases:
        t = c.task
        assert len(t.nonce) % 64 == c.p and t.worker_byte < 1 << c.wbits and t.num_trailing_zeros == 1
        assert (t.k_end - t.k_begin) << _rbits(c) <= 1024
        blocks = [_nblk(c, k) for k in range(t.k_begin, t.k_end)]
        if c.a == W.TOP:
            assert (t.k_begin, t.k_end) == (DPOW_K_LIMIT - 3, DPOW_K_LIMIT) and c.edge == DPOW_K_LIMIT
            last = (t.k_end << _rbits(c)) - 1                          # the window's last local index
            assert last == (DPOW_K_LIMIT << _rbits(c)) - 1
            if c.wbits == 0:                                           # the highest local index there is
                assert last == 2 ** 63 - 257
            # chunks of 7 bytes: two blocks from p = 48 on, throughout
            assert blocks == [2 if c.p >= 48 else 1] * 3
            assert len(W.secret_of(t.k_begin << 8)) == 8
            assert distpow.batch_candidate(t.nonce, t.worker_byte, c.wbits, last)[2] == blocks[-1]
        else:
            assert (t.k_begin, t.k_end) == (max(c.edge - 2, 0), c.edge + 2) and c.edge == W.edge(c.a)
            L = c.a + 1                                                # chunk length at the edge
            assert len(W.secret_of(c.edge << 8)) == 1 + L and len(W.secret_of((c.edge - 1) << 8)) == L
            assert _nblk(c, c.edge) == (2 if c.p + 1 + L > 55 else 1)
            assert _nblk(c, c.edge - 1) == (2 if c.p + L > 55 else 1)
            if c.p == 54 - c.a:                                        # the block-count change itself
                assert blocks == [1] * (c.edge - t.k_begin) + [2, 2]
    assert {c.p for c in cases if c.a == W.TOP} == {48, 0, 47, 55, 63}


def test_family_g_is_one_partial_wave_with_two_block_clamped_lanes():
    cases, ctl = W.family_g(), W.family_g_controls()
    per_a = sum(2 * ((64 >> (8 - wbits)) - 2) for wbits in W.G_WBITS)
    assert len(cases) == len(ctl) == 6 * per_a + 2 * len(W.G_WBITS) == 1378 <= DPOW_BATCH_MAX
    want = {(a, wbits, d) for a in range(1, 7) for wbits in W.G_WBITS for d in range(1, (64 >> (8 - wbits)) - 1)}
    want |= {(0, wbits, 1) for wbits in W.G_WBITS}
    for fam in (cases, ctl):
        keys = collections.Counter((c.a, c.wbits, c.d) for c in fam)
        assert set(keys) == want and set(keys.values()) == {2}         # nonce lengths p and p + 64
    for c, with_edge in [(c, True) for c in cases] + [(c, False) for c in ctl]:
        t = c.task
        assert c.p == 54 - c.a and len(t.nonce) % 64 == c.p and t.worker_byte < 1 << c.wbits
        assert (t.k_begin, t.k_end) == (c.edge - c.d, c.edge + with_edge) and t.num_trailing_zeros == 1
        n = (t.k_end - t.k_begin) << _rbits(c)
        assert 0 < n < 64                                              # never a full wave
        blocks = [_nblk(c, k) for k in range(t.k_begin, t.k_end)]
        # the inactive lanes hash the window's last index again: the edge's k in the family, a
        # one-block k in the control
        assert blocks == ([1] * c.d + [2] if with_edge else [1] * c.d)
    # the clamped lanes: from 1 (worker_bits 8, d = 62) to 62 (worker_bits 8, d = 1) of the 64
    idle = {64 - ((c.task.k_end - c.task.k_begin) << _rbits(c)) for c in cases}
    assert min(idle) == 1 and max(idle) == 62


def test_every_window_is_one_descriptor_from_its_begin():
    """The wave boundaries: a scan or census kernel's workgroup starts its waves at its descriptor's
    begin.  Every task of families A, B and G and their controls is exactly one descriptor
    [k_begin << rbits, k_end << rbits) under both planners with the call's own budgets, for the
    whole family in one call and for each edge's tasks alone; family F's tasks are whole descriptors
    from the window's begin.  Miner.scan's slice is larger than every window: one launch each."""
    for ntz in (1, 3):
        assert distpow.scan_slice(ntz) >= 1 << 18
    for name, fam in _families().items():
        subsets = [fam] + [[c for c in fam if c.a == a] for a in sorted({c.a for c in fam})]
        for cases in subsets:
            assert 0 < len(cases) <= DPOW_BATCH_MAX
            want = [(c.task.k_begin << _rbits(c), c.task.k_end << _rbits(c)) for c in cases]
            assert all(hi - lo < distpow.scan_slice(1) for lo, hi in want)
            plans = [distpow.scan_plan([(lo, hi, ntz) for lo, hi in want])[0] for ntz in (1, 3)]
            plans.append(distpow.census_plan([(c.task.k_begin, c.task.k_end, c.wbits) for c in cases])[0])
            for blocks in plans:
                per_task = collections.defaultdict(list)
                for b in blocks:
                    per_task[b.task].append((b.i_begin, b.i_end))
                assert sorted(per_task) == list(range(len(cases)))
                for j, (lo, hi) in enumerate(want):
                    d = per_task[j]
                    if name != "F":
                        assert d == [(lo, hi)], (name, j)
                        continue
                    assert d[0][0] == lo and d[-1][1] == hi, (name, j)
                    assert all(x[1] == y[0] for x, y in zip(d, d[1:]))
                    assert all((e - b) % MIN_GROUP == 0 for b, e in d[:-1]) and len(d) <= 4


def test_the_gpu_tests_cannot_pass_vacuously():
    """Hits come at rate 1/16 at N = 1 and a depth of at least 3 at rate 1/4096; each condition is
    stated with what those rates let expect."""
    # Family A, 225792 candidates: about 55 of depth >= 3, through the census's LDS path on waves
    # that hold both block counts.
    deep = sum(1 for c in W.family_a() for _, tz in W.depths_of(c) if tz >= 3)
    # Family G, about 42000 candidates below the edges: about 2600 hits among the one-block lanes of
    # a wave whose other lanes are two-block; the edge's k is 1 to 16 candidates, so about a sixth
    # of the 1378 windows have a hit on it.
    g = W.family_g()
    below = sum(1 for c in g for h in c.hits if h >> 8 < c.edge)
    on_edge = sum(any(h >> 8 == c.edge for h in c.hits) for c in g)
    print(f"family A: {deep} candidates of depth >= 3; family G: {below} hits below the edges, {on_edge} windows "
          f"with a hit on the edge's k")
    assert deep >= 30
    assert below >= 1000 and on_edge >= 25
    # Family F: a hit on both sides of every edge.  A side is 64 to 512 candidates (the one k below
    # edge(0), or two k): none with probability 1.6e-2 to 4e-15 -- the seed offset is chosen so that
    # every window passes.  At the top the two sides are the last k and the two before it.
    for c in W.family_f():
        split = DPOW_K_LIMIT - 1 if c.a == W.TOP else c.edge
        assert any(h >> 8 < split for h in c.hits) and any(h >> 8 >= split for h in c.hits), (c.a, c.wbits, c.p)
    # the controls of G are not empty either
    assert sum(len(c.hits) for c in W.family_g_controls()) >= 1000


def test_the_derived_references_agree():
    """The depth reference lists every candidate once in index order, and filtering it at N = 1
    gives the hit lists the families were built with (window_hits); the ScanHit lists and the
    Census derived from it are self-consistent."""
    for name, fam in _families().items():
        for c in fam:
            t = c.task
            pairs = W.depths_of(c)
            tbs = W.thread_bytes(t.worker_byte, t.worker_bits)
            assert [g for g, _ in pairs] == [k << 8 | tb for k in range(t.k_begin, t.k_end) for tb in tbs]
            assert [g for g, tz in pairs if tz >= 1] == c.hits, (name, t)
    for c in W.family_a()[::97] + W.family_f()[::11] + W.family_g()[::53]:
        pairs = W.depths_of(c)
        for g, tz in pairs[::17]:
            assert tz == W.tz_of(c.task.nonce, g)
        for n in (1, 3):
            hits = W.scan_hits_of(c, n)
            assert [h.global_idx for h in hits] == [g for g, tz in pairs if tz >= n]
            assert all(h.secret == W.secret_of(h.global_idx) == distpow.secret_from_index(h.global_idx) and
                       h.tz == W.tz_of(c.task.nonce, h.global_idx) for h in hits)
        cen = W.census_of(c)
        assert cen.count_ge[0] == len(pairs) and cen.first_ge[0] == pairs[0][0] and cen.first_tz[0] == pairs[0][1]
        assert cen.deepest == max(tz for _, tz in pairs)
        for d in range(W.D):
            at = [(g, tz) for g, tz in pairs if tz >= d]
            assert cen.count_ge[d] == len(at)
            assert (cen.first_ge[d], cen.first_tz[d]) == (at[0] if at else (None, 0))
        assert cen.merged(distpow.Census.empty()) == cen               # self-consistent by the library's own check
