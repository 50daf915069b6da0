"""The case families of tests/_batch_walk_cases.py are what they claim -- shown from hashlib, the C
oracle and the round planner alone, no GPU: tests/test_gpu_batch_walk.py compares the batched
search kernel with these lists by equality, so a family that misses its edge would pin nothing.
Also the batched walk itself, driven by the oracle, returns hashlib's lists."""
import collections

import distpow
from distpow import EXHAUSTED, FOUND
from distpow._lib import DPOW_BATCH_MAX, DPOW_K_LIMIT

import _batch_walk_cases as W


def _rbits(wbits):
    return 8 - wbits


def _nblk(c, k):
    """Block count of the window's candidate at k, from the host copy of the kernel's assembly."""
    t = c.task
    return distpow.batch_candidate(t.nonce, t.worker_byte, t.worker_bits, k << _rbits(t.worker_bits))[2]


def test_family_a_puts_the_block_count_change_inside_a_wave():
    cases = W.family_a()
    assert len(cases) == 1764 <= DPOW_BATCH_MAX
    keys = collections.Counter((c.a, c.wbits, c.d) for c in cases)
    want = {(a, wbits, d) for a in range(7) for wbits in range(3, 9) for d in range(1, (64 >> (8 - wbits)) + 1)}
    assert set(keys) == want and set(keys.values()) == {2}           # nonce lengths p and p + 64
    assert sum((c.task.k_end - c.task.k_begin) << _rbits(c.wbits) for c in cases) == 225792
    mixed = collections.defaultdict(set)
    for c in cases:
        t, per = c.task, 64 >> (8 - c.wbits)
        assert c.p == 54 - c.a and len(t.nonce) % 64 == c.p and t.worker_byte < 1 << c.wbits
        assert t.k_begin == max(c.edge - c.d, 0) and t.k_end == t.k_begin + 2 * per      # two waves
        assert t.k_begin < c.edge < t.k_end
        assert _nblk(c, c.edge - 1) == 1 and _nblk(c, c.edge) == 2
        assert _nblk(c, t.k_begin) == 1 and _nblk(c, t.k_end - 1) == 2
        pos = c.edge - t.k_begin           # the edge's k position from the first wave's first k
        if pos < per:                      # both block counts among the 64 indices of the first wave
            assert (c.edge - 1 - t.k_begin) // per == (c.edge - t.k_begin) // per == 0
        mixed[c.a, c.wbits].add(pos % per)
    for (a, wbits), positions in mixed.items():
        per = 64 >> (8 - wbits)
        # every k position of a wave (position 0: the wave behind is two-block throughout); below
        # edge(0) = 1 there is only k = 0, so there the edge is always the wave's second k
        assert positions == ({1} if a == 0 else set(range(per))), (a, wbits)
    behind = sum(any(g >> 8 >= c.edge for g in c.hits) for c in cases)
    before = sum(any(g >> 8 < c.edge for g in c.hits) for c in cases)
    empty = sum(not c.hits for c in cases)
    print(f"family A: {behind} of {len(cases)} tasks with a hit at or behind the edge, {before} with one before "
          f"it, {empty} empty windows, at most {max(len(c.hits) for c in cases)} hits")
    assert behind >= 0.95 * len(cases)
    assert empty <= 0.02 * len(cases)


def test_family_b_covers_every_byte_position_at_every_edge():
    cases = W.family_b()
    assert len(cases) == 8 * 64 * 3
    assert {(c.a, c.p) for c in cases} == {(a, p) for a in range(8) for p in range(64)}
    assert {c.p >> 2 for c in cases} == set(range(16))                 # every W0 the kernel branches on
    assert {len(c.task.nonce) // 64 for c in cases} == {0, 1, 2}
    for c in cases:
        t = c.task
        assert t.worker_bits == 8 and t.num_trailing_zeros == 1 and t.k_end - t.k_begin == 64
        assert len(t.nonce) % 64 == c.p
        if c.a == W.TOP:
            assert t.k_end == c.edge == DPOW_K_LIMIT
        else:
            assert t.k_begin == max(c.edge - 32, 0) and t.k_begin < c.edge < t.k_end
            L = (c.edge.bit_length() + 7) // 8                          # chunk length at the edge
            assert _nblk(c, c.edge) == (2 if c.p + 1 + L > 55 else 1)
            assert _nblk(c, c.edge - 1) == (2 if c.p + L > 55 else 1)
    inner = [c for c in cases if c.a != W.TOP]
    both = sum(any(g >> 8 < c.edge for g in c.hits) and any(g >> 8 >= c.edge for g in c.hits) for c in inner)
    empty = sum(not c.hits for c in inner)
    top = [c for c in cases if c.a == W.TOP]
    print(f"family B: {both} of {len(inner)} tasks with hits on both sides of the edge, {empty} empty windows; "
          f"{sum(bool(c.hits) for c in top)} of {len(top)} top-of-range tasks with a hit")
    assert len(inner) == 1344 and both >= 0.70 * len(inner)
    k0 = [bool(c.hits) and c.hits[0] >> 8 == 0 for c in cases if c.a == 0]    # k = 0: the empty chunk
    assert sum(k0) >= 120 and k0.count(False) >= 50
    assert sum(bool(c.hits) for c in top) >= 0.95 * len(top)           # 64 candidates at N = 1: 1 - (15/16)^64


def test_family_b_controls_never_and_always_take_the_second_block():
    ctl = W.family_b_controls()
    for name, nblk in (("never", 1), ("always", 2)):
        cases = ctl[name]
        assert len(cases) == 7 * 2 * 2 and {c.a for c in cases} == set(range(7))
        for c in cases:
            assert c.wbits == 3 and c.p == (53 if nblk == 1 else 55) - c.a
            assert c.task.k_begin < c.edge < c.task.k_end
            assert {_nblk(c, k) for k in range(c.task.k_begin, c.task.k_end)} == {nblk}
        assert sum(any(g >> 8 >= c.edge for g in c.hits) for c in cases) >= 0.9 * len(cases)


def test_family_c_reaches_every_case_of_the_fixture():
    tasks, cases = W.family_c(), W.deep_cases()
    layout = [c for c in cases if c["source"] == "layout"]
    assert len(layout) == 78 and sum(len(c["hits"]) for c in layout) == 205
    assert sum(1 for c in layout for _, tz in c["hits"] if tz >= 9) == 78
    n_hits = sum(len(c["hits"]) for c in cases)
    assert len(tasks) == n_hits * 9 and len(tasks) <= DPOW_BATCH_MAX
    assert {t.case for t in tasks} == {c["name"] for c in cases}
    assert {len(c["nonce"]) for c in layout} >= set(range(64)) | {69, 115, 190}
    golden = [c for c in cases if c["source"] == "golden"]
    assert len(golden) == 8 and max(tz for c in golden for _, tz in c["hits"]) == 10
    for nblk in (1, 2):
        assert any(t.tz == 8 and t.nblk == nblk for t in tasks)
    for t in tasks:
        assert 0 < t.task.k_end - t.task.k_begin <= 16
        want = {"n8": 8, "n9": 9, "next": t.tz + 1}[t.kind]
        assert t.task.num_trailing_zeros == want
        if t.expected[0] == FOUND:     # every expected hit is a listed one, hashed again here
            assert W.tz_of(t.task.nonce, t.expected[1]) >= want
    by = collections.Counter((t.kind, t.expected[0]) for t in tasks)
    assert by["n8", EXHAUSTED] == 0 and by["n8", FOUND] == n_hits * 3
    # N = 9: a window round a tz = 8 entry is exhausted (a kernel without the recheck reports the
    # entry), one round a deeper entry returns it (a kernel whose recheck rejects too much does not)
    assert by["n9", EXHAUSTED] >= 3 * 100 and by["n9", FOUND] >= 3 * 78
    assert all(t.expected == W.found(t.g) for t in tasks if t.kind == "n8" or (t.kind == "n9" and t.tz >= 9))
    assert all(t.expected == W.NO_HIT for t in tasks if t.kind == "next")    # no k holds two listed hits
    assert {t.task.worker_bits for t in tasks} == {0, 3, 8}


def test_family_d_is_one_round_for_a_lone_task():
    fam = W.family_d()
    assert set(fam) == {(b, n) for b in (1, 2, 3) for n in (1, 2)}
    for (b, n), batches in fam.items():
        assert len(batches) == 8 and len({t.nonce for batch in batches for t in batch}) == 8 * b
        for batch in batches:
            assert len(batch) == b
            assert all(t.k_end - t.k_begin == 4096 and t.worker_bits == 0 and t.num_trailing_zeros == n for t in batch)
            entries, launches = distpow.batch_plan([(t.k_begin, t.k_end, 0) for t in batch])
            first = [e for e in entries if e.launch == 0]
            if b == 1:       # the whole window is round 0, one workgroup per 256 candidates
                assert launches == 1 and (first[0].rows, first[0].group) == (4096, 256)
            assert all(e.rows * len(first) >= 2048 for e in first)


def test_family_e_realises_every_seam(oracle):
    for wbits in (8, 0):
        R = 256 >> wbits
        cases = W.family_e(oracle, wbits)
        assert [c.seam for c in cases] == list(W.SEAMS)
        for c in cases:
            p, s, grp = c.probe, c.slice, c.group
            assert len(c.batch) == W.E_BATCH and W.round0_of(c.batch) == (s, grp)
            assert (p.k_end - p.k_begin) * R == W.E_WINDOW >= 2 * s and s % grp == 0 and grp % R == 0
            # the offset: the hit's local index (k * R + its place among the thread bytes) from i_begin
            i_hit = (c.hit >> 8) * R + W.thread_bytes(p.worker_byte, wbits).index(c.hit & 0xFF)
            assert c.offset == i_hit - p.k_begin * R
            seam = {"group": grp, "slice": s}.get(c.seam.split("-")[0])
            if c.seam == "last":
                assert c.hit >> 8 == p.k_end - 1 and c.offset >= s
            elif c.seam.endswith("-1"):     # the last k below the seam (R = 1: the last index)
                assert c.offset < seam <= c.offset - c.offset % R + R
            else:                           # the first k at the seam (R = 1: the seam itself)
                assert c.offset - c.offset % R == seam
            if R == 1 and c.seam != "last":
                assert c.offset == {"group-1": grp - 1, "group": grp, "slice-1": s - 1, "slice": s}[c.seam]
            # the hit-free prefix, by the oracle alone: the window's first hit is the chosen one,
            # and it is a hit by hashlib
            r = oracle.mine_window(list(p.nonce), W.E_NTZ, p.worker_byte, wbits, p.k_begin, p.k_end)
            assert r is not None and r[1] == c.hit and W.tz_of(p.nonce, c.hit) >= W.E_NTZ
            assert c.expected[W.E_PROBE] == W.found(c.hit)
            # the fillers: fixed 4-k windows, done within round 0
            for j, t in enumerate(c.batch):
                if j != W.E_PROBE:
                    assert t.k_end - t.k_begin == 4 and 4 * 256 <= s
        assert len({tuple((t.nonce, t.k_begin) for j, t in enumerate(c.batch) if j != W.E_PROBE) for c in cases}) == 1


def test_oracle_driven_walk_returns_the_hashlib_lists(oracle):
    """walk_batch is sound: with a search_batch built on oracle.mine_window it returns, for
    family A and the top-of-range windows of family B, exactly hashlib's lists."""
    calls = []

    def search_batch(tasks):
        calls.append(len(tasks))
        return W.oracle_search_batch(oracle)(tasks)

    cases = W.family_a() + [c for c in W.family_b() if c.a == W.TOP]
    hits = W.walk_batch(search_batch, [c.task for c in cases], 1)
    assert hits == [c.hits for c in cases]
    assert calls[0] == len(cases) and calls == sorted(calls, reverse=True)     # tasks only ever drop out
    assert len(calls) <= max(len(c.hits) for c in cases) + 1
