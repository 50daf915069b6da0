"""The depth reference and families F and G of tests/_batch_walk_cases.py are what they claim, and
the windows of families A, B and G land on the wave boundaries they were built for under the scan's
and the census's own planners -- shown from hashlib, the host copy of the kernels' candidate
assembly (distpow.batch_candidate) and the planners (distpow.scan_plan, census_plan, scan_slice)
alone, no GPU.  tests/test_gpu_listing_walk.py compares the scan and census kernels with these
lists by equality, so a family that misses its edge, or a reference that is wrong, would pin
nothing.

The device scan (tests/test_gpu_scan_dev_walk.py) runs the same sets, so the last tests show the same
for it from a restatement of its geometry (_batch_walk_cases.scan_dev_geometry, pinned to the sources'
constants here and to the library's behaviour on the GPU), and that family H, which holds no hashes,
reaches every group size, the ragged last group and the prefix rounds it names."""
import collections
import os
import re

import distpow
from distpow._lib import DPOW_BATCH_MAX, DPOW_K_LIMIT

import _batch_walk_cases as W
from test_gpu_listing_walk import IDS, SETS, _cases as set_cases

MIN_GROUP = 256   # local indices of the smallest workgroup range (csrc/batch.h kBatchMinGroup)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed-proof-of-work_amd",
                    "csrc")


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


# ---- the device scan (tests/test_gpu_scan_dev_walk.py) --------------------------------------------
def _constant(header, name):
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"\b%s\s*=\s*([^,;]+)[,;]" % name, text)
    assert m, (header, name)
    expr = re.sub(r"\b(\d+)(?:ull|u)\b", r"\1", m.group(1))
    assert re.fullmatch(r"[\d\s<()]+", expr), expr                     # a number or a shift of numbers
    return eval(expr)


def test_scan_dev_geometry_constants_are_the_sources():
    assert _constant("batch.h", "kBatchBlocks") == W.SCAN_DEV_BLOCKS == 4096
    assert _constant("batch.h", "kBatchMinGroup") == W.SCAN_DEV_MIN_GROUP == 256
    assert _constant("batch.h", "kBatchMaxGroup") == _constant("md5_scan_dev.h", "kScanDevMaxGroup") == \
        W.SCAN_DEV_MAX_GROUP == 16384
    assert _constant("md5_scan_dev.h", "kScanDevSlice") == _constant("batch.h", "kBatchCap") == W.SCAN_DEV_SLICE == 1 << 28
    assert _constant("dpow_common.h", "kBlockThreads") == W.SCAN_DEV_STEP == 256
    assert _constant("md5_scan_dev.hip", "kScanPrefixPer") * W.SCAN_DEV_STEP == W.SCAN_DEV_PREFIX_ROUND == 2048
    # the rule itself: clamp(pow2_floor(total / 4096), 256, 16384), the last group short
    src = open(os.path.join(CSRC, "batch.cpp")).read()
    assert re.search(r"pow2_floor\(total / kBatchBlocks\), kBatchMinGroup\),\s*kBatchMaxGroup\)", src)
    geo = W.scan_dev_geometry
    assert [geo(t) for t in (1, 256, 257, (1 << 20) - 1)] == [(256, 1), (256, 1), (256, 2), (256, 4096)]
    assert [geo(t)[0] for t in (1 << 20, (1 << 21) - 1, 1 << 21, 3 << 25, (1 << 26) - 1, 1 << 26, 1 << 28)] == \
        [256, 256, 512, 16384, 8192, 16384, 16384]
    assert geo(1 << 28) == (16384, 16384) and geo((1 << 21) + 352) == (512, 4097)
    assert W.scan_dev_slices(7, 7) == [] and W.scan_dev_slices(32, (5 << 27) + 32) == \
        [(32, (1 << 28) + 32, 16384, 16384), ((1 << 28) + 32, (2 << 28) + 32, 16384, 16384),
         ((2 << 28) + 32, (5 << 27) + 32, 16384, 8192)]


def test_every_edge_window_is_one_slice_of_small_groups_from_its_begin():
    """The device scan's waves start at the slice's begin, and a slice at the call's: every window of
    every family is one slice at group 256 of one to four workgroups, so its waves hold the local
    indices the families were built round, as in the scan's and the census's descriptors above."""
    seen = set()
    for which in SETS:
        for c in set_cases(which):
            lo, hi = c.task.k_begin << _rbits(c), c.task.k_end << _rbits(c)
            slices = W.scan_dev_slices(lo, hi)
            assert len(slices) == 1 and slices[0][:3] == (lo, hi, MIN_GROUP), (which, c.task)
            assert 1 <= slices[0][3] <= 4 and hi - lo <= 1024
            seen.add(slices[0][3])
    assert seen == {1, 2, 3, 4}


def test_the_device_scan_tests_cannot_pass_vacuously():
    """Per set of tests/test_gpu_scan_dev_walk.py: a window with a hit at N = 1 on each side of its
    edge, where its windows have two sides (the controls of G end below the edge, and below
    DPOW_K_LIMIT there is one side); at N = 3, a rate of 1/4096, over the sets together."""
    deep = 0
    for which, name in zip(SETS, IDS):
        cases = set_cases(which)
        deep += sum(1 for c in cases for _, tz in W.depths_of(c) if tz >= 3)
        two_sided = [c for c in cases if c.task.k_begin < c.edge < c.task.k_end]
        assert bool(two_sided) == (which[0] != "Gctl" and which != ("B", W.TOP) and which != ("F", W.TOP)), name
        if two_sided:
            assert any(any(h >> 8 < c.edge for h in c.hits) and any(h >> 8 >= c.edge for h in c.hits)
                       for c in two_sided), name
        else:
            # (the controls at edge(0) are ten windows of k = 0 alone, 1 to 16 candidates each)
            assert sum(len(c.hits) for c in cases) >= 1, name
    print(f"{deep} candidates of depth >= 3 in the sets together")
    assert deep >= 100


def test_family_h_reaches_every_group_size_ragged_across_steps():
    """From the restated geometry alone (nothing is hashed): each window is one slice of the group it
    names; the g-windows have 4097 workgroups, odd and three rounds of the prefix (g512b6145: 6145 and
    four), and a last group whose waves 0 and 1 run s + 1 steps, wave 1's last with 32 active lanes, and
    waves 2 and 3 run s."""
    fam = W.family_h()
    assert [w.name for w in fam] == [f"g{g}" for g in W.H_GROUPS] + ["b2047", "b2048", "b2049r", "g1024w0n56", "g512b6145"]
    assert W.H_GROUPS == (512, 1024, 2048, 4096, 8192, 16384)
    assert len({w.nonce for w in fam}) == 2 and len({w.k_begin for w in fam}) == len(fam)
    for w in fam:
        R = 1 << w.rbits
        lo, hi = w.k_begin << w.rbits, w.k_end << w.rbits
        assert W.scan_dev_slices(lo, hi) == [(lo, hi, w.group, w.n_blocks)], w.name
        assert w.k_begin != 0 and w.k_begin % max(w.group // R, 2) != 0 and w.k_end < 1 << 22
        last = W.scan_dev_wave_steps(w.total - (w.n_blocks - 1) * w.group)
        full = W.scan_dev_wave_steps(w.group)
        assert full == [(w.group // 256, 64)] * 4
        rounds = -(-w.n_blocks // W.SCAN_DEV_PREFIX_ROUND)
        if w.name == "g1024w0n56":
            assert (w.wbits, len(w.nonce), w.group, w.n_blocks, rounds) == (0, 56, 1024, 4097, 3)
            assert w.total == 4096 * 1024 + 768 and last == [(3, 64)] * 4
            assert distpow.batch_candidate(w.nonce, w.wb, w.wbits, lo)[2] == 2      # two final blocks
            continue
        assert (w.wbits, w.wb, len(w.nonce), R) == (3, W.H_WB, 4, 32)
        if w.name.startswith("g"):
            many = w.name == "g512b6145"       # the third round's carry reaches groups that are placed from
            assert w.s == (1 if w.group == 512 else w.group // 512)
            assert w.total == (6144 if many else 4096) * w.group + 256 * w.s + 96
            assert (w.n_blocks, rounds, w.n_blocks % 2) == ((6145, 4, 1) if many else (4097, 3, 1))
            assert last == [(w.s + 1, 64), (w.s + 1, 32), (w.s, 64), (w.s, 64)]
            assert 2 <= w.group // 256 <= 64 and w.s + 1 <= w.group // 256     # the steps fit a wave's lanes
        else:
            assert w.group == 256 and w.total < 1 << 20
            assert (w.n_blocks, w.total, rounds) == {"b2047": (2047, 2047 * 256, 1), "b2048": (2048, 2048 * 256, 1),
                                                     "b2049r": (2049, 2048 * 256 + 96, 2)}[w.name]
            assert last == ([(1, 64), (1, 32), (0, 0), (0, 0)] if w.name == "b2049r" else [(1, 64)] * 4)
    # the window whose page cut falls inside its second slice
    w = W.second_slice_window()
    lo, hi = w.k_begin << w.rbits, w.k_end << w.rbits
    assert W.scan_dev_slices(lo, hi) == [(lo, lo + (1 << 28), 16384, 16384), (lo + (1 << 28), hi, 512, 4097)]
    assert w.total == (1 << 28) + (1 << 21) + 352 and (w.group, w.n_blocks) == (512, 4097)
    assert W.scan_dev_wave_steps(352) == [(2, 64), (2, 32), (1, 64), (1, 64)]


def test_second_slice_cuts_differ():
    """tests/test_gpu_scan_dev_walk.py cuts the second slice with room for 0, 1 and 40 of its hits: by
    hashlib over the slice's first 2^18 local indices (about 64 hits at N = 3), the slice begins with
    empty groups, so a room of 0 advances without placing anything, and the three rooms end at two
    different k at least."""
    w = W.second_slice_window()
    k2 = w.k_begin + ((1 << 28) >> w.rbits)
    hits = W.window_hits(w.nonce, 3, w.wb, w.wbits, k2, k2 + ((1 << 18) >> w.rbits))
    totals = collections.Counter(((g >> 8) - k2 << w.rbits | g & 31) // w.group for g in hits)
    assert len(hits) > 40
    cuts = []
    for room in (0, 1, 40):
        n_fit = s = 0
        while s + totals[n_fit] <= room:
            s += totals[n_fit]
            n_fit += 1
        cuts.append(n_fit)
    print(f"{len(hits)} hits in the first 512 groups of the second slice; rooms 0, 1, 40 take {cuts} groups")
    assert cuts[0] >= 1 and len(set(cuts)) >= 2 and max(cuts) < 512
