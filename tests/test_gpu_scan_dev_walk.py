"""GPU: the device scan's own kernels (scan_mask_kernel, scan_place_kernel and the retirement prefix of
csrc/md5_scan_dev.hip) and its host cut (csrc/scan_dev.cpp) at every layout edge, every group size
and page cuts in the middle of a slice.

The order of the device scan's list is not sorted: it is geometry -- the bitmap word a wave-step's
ballot goes to, ((lo - i_begin) >> 6) + 4 lane + wave, gathered over up to 64 steps in lane registers;
the `steps` count behind the loop; the last workgroup's prefix in rounds of 2048 totals.  A wrong word
index or a lost carry gives a list that is ascending, inside the window, plausible and wrong, and the
call's own check (order, depth >= N, 16 samples) passes on it with good odds.  tests/test_gpu_scan_dev.py
runs at group 256 and, on exact powers of two, at group 16384 only.  Every assertion here is an
equality with hashlib, arithmetic, the digest kernel or Miner.scan; none compares the device scan
with itself.

1. test_edges: the sets of tests/test_gpu_listing_walk.py (families A, B, F, G and their controls of
   tests/_batch_walk_cases.py), every window through Miner.scan_cuda at N = 1 and 3: indices and depths
   are hashlib's.  A window is one slice at group 256 from its own begin
   (tests/test_listing_walk_cases.py), so the waves fall where the families were built for them.
2. test_group_sizes: family H -- groups 512 to 16384 with 4097 workgroups (three rounds of the
   prefix) and a last group ragged across steps, 2047, 2048 and 2048.375 groups of 256, and a
   two-block window at 256 candidates per k -- once in descending and once in ascending size on one
   context, so a slice sits on the stale bitmap words and totals of a larger one and the reverse.
   N = 0: the list is every index of the partition, built arithmetically.  N = 1 and 3: the indices
   whose depth, by the digest kernel over the window's arithmetic index list (Miner.digests_cuda, 2^22
   entries a call), is at least N.  The digest kernel shares the hash with the mask kernel and none of
   its geometry: it gathers one listed candidate per lane.  The hash is pinned to hashlib by part 1 and
   by tests/test_gpu_digests.py, so the depth comparison of this part is the digest kernel against
   itself (the call's depths are the same kernel's over the same entries) and index equality is the
   content.  At groups 512 and 4096 the N = 3 list is also Miner.scan's: another kernel, a host MD5
   per hit.
3. test_paging_middle_group, test_first_page_pins_the_group, test_cut_inside_second_slice: the exact
   status, entry count and k_done of every page, from the reference's per-group totals, the restated
   geometry (a page is a new call from k_done with a group of its own) and distpow.scan_device_cut or
   a brute-force loop; a cut inside the second slice of a call, the case that places nothing from
   that slice included.

Every test prints its wall time (pytest -s).  On an MI355X the 46 tests take 4.4 s alone (process,
context and hashlib's lists included) beside the listing walk's 178 tests in 4 s.  Inside the tests:
test_edges 0.83 s for the 39 sets (1.31 s in another run; A 35-38 ms a set of 504 calls, B 25-26 ms of
384, F 5 ms of 60, G and its controls 26-28 ms of 456) against 0.25-0.26 s for the listing walk's
test_scan over the same sets -- 3.2 to 5.3 times.  The time is per call, 75-135 us against 24 us, not
hashing: a scan_cuda call allocates two tensors, waits for torch's stream, queues the mask launch and
waits for its record, queues the place, depth and check launches, a copy and a memset, waits for the
stream, and the test copies both lists to the host; Miner.scan is one launch and one wait.
test_group_sizes 0.04 s and 0.03 s for 33 calls each, the reference of 2.1e8 candidates in the first
(0.5 s where it was the first torch work of the process); a call 0.10 ms (2^19 candidates) to 0.75,
0.83 and 1.64 ms (g16384 at N = 3, 1, 0: 6.7e7 candidates, 6.7e7 entries at N = 0).
test_paging_middle_group 2.5 and 2.2 ms for 17 and 16 pages; test_cut_inside_second_slice 33 ms of
Miner.scan for 66125 hits and 9 ms for its six calls.

Shown to bite on five deliberately wrong libraries (built outside the tree, one run each; every one
stays in bounds by construction: it changes register values, reads fewer words or makes a prefix
smaller, and every list store stays clamped to max_hits):
  1. scan_mask_kernel keeps no ballot of a wave's last step when that step is partial and not step 0.
     Fails test_group_sizes[descending, ascending] -- every g-window at N = 0 (32 entries short) and
     those at N = 1 where the half wave has a hit -- and passes the other 44;
     tests/test_gpu_scan_dev.py passes on it.
  2. scan_place_kernel rounds n_words down to a multiple of 4 when it is above 4.  Fails
     test_group_sizes[descending, ascending] on the g-windows at N = 0 and 1 (the entries not placed
     are whatever the buffer held, and the call's own check refuses the list), passes the other 44;
     tests/test_gpu_scan_dev.py passes on it.
  3. The retirement loses the prefix carry from the third round on.  Fails test_group_sizes[both]
     on g512b6145 alone -- with 4097 workgroups the third round's only entry is prefix[4096], which
     no workgroup places from -- and, through the host's "the prefix does not end at the total",
     test_paging_middle_group[both], test_first_page_pins_the_group[both] and
     test_cut_inside_second_slice; passes the other 39.  tests/test_gpu_scan_dev.py sees this one
     too: test_slice_seams (16384 workgroups) and test_paging_long_list_against_digests_and_census.
  4. The retirement takes the stale total behind an odd launch's last one into the slice's total.
     Fails test_group_sizes[both] (b2049r and the windows behind a dense slice; with N ascending
     inside a window, as this test first had it, the stale total was a sparse slice's and almost
     always 0: hence N = 3, 1, 0), test_edges[F-6], and the five paging tests as in 3; passes the
     other 38.  tests/test_gpu_scan_dev.py fails two tests on it.
  5. batch_hash_at, shared by all eight generic kernels: every lane takes the second block's state
     when any lane of its wave needs it.  Fails test_edges[A-0..6, B-0..6, G-0..6], as the other
     copies did in tests/test_gpu_listing_walk.py, and here F-0..6 as well: the mask kernel's waves
     hold one k of family F, but the depths come from the digest kernel over the placed hits, whose
     waves hold hits from both sides of the edge.  Passes B-7, F-7 and all controls, the other 18 tests
     and tests/test_gpu_scan_dev.py.
"""
import time

import pytest
import torch

import _batch_walk_cases as W
import distpow
from distpow import EXHAUSTED, MORE
from test_gpu_listing_walk import IDS, SETS, _cases, _key, _still_usable

pytestmark = pytest.mark.gpu

MIN_HITS = distpow.SCAN_DEVICE_MIN_HITS   # 16384: the smallest max_hits
# Sparse first: a window's N = 3 slice sits on the dense N = 0 bitmap and totals of the window before
# it, and its own N = 0 slice on its sparse ones.
H_NTZ = (3, 1, 0)


# ---- 1. layout edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SETS, ids=IDS)
def test_edges(miner, which):
    """scan_mask_kernel and scan_place_kernel: every hit of every window with its depth is hashlib's,
    one slice per call."""
    cases = _cases(which)
    t0, calls, n_hits = time.perf_counter(), 0, 0
    for c in cases:
        t = c.task
        pairs = W.depths_of(c)
        for ntz in (1, 3):
            idx, dep = miner.scan_cuda(t.nonce, ntz, t.worker_byte, t.worker_bits, t.k_begin, t.k_end, max_hits=MIN_HITS)
            calls += 1
            st = miner.last_scan_device_stats
            assert (st.rounds, st.candidates) == (1, (t.k_end - t.k_begin) << (8 - c.wbits)), (ntz,) + _key(c)
            want = ([g for g, tz in pairs if tz >= ntz], [tz for _, tz in pairs if tz >= ntz])
            assert (idx.tolist(), dep.tolist()) == want, (ntz,) + _key(c)
            n_hits += len(want[0])
    print(f"scan_cuda {which}: {len(cases)} windows, {n_hits} hits in {calls} calls (N = 1, 3), "
          f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
    _still_usable(miner)


# ---- 2. every group size, ragged across steps ---------------------------------------------------------
_DEPTHS = {}


def _depths(miner, w):
    """The reference of a window, once per process and never changed: the depth of every candidate
    in index order (W.window_depths_cuda)."""
    if w.name not in _DEPTHS:
        _DEPTHS[w.name] = W.window_depths_cuda(miner, w.nonce, w.wb, w.wbits, w.k_begin, w.k_end)
        assert _DEPTHS[w.name].numel() == w.total
    return _DEPTHS[w.name]


def _expected(miner, w, ntz, first=0):
    """The global indices of the window's candidates of depth >= ntz from local offset `first` on, in
    order: a device tensor.  At N = 0 nothing is hashed."""
    dev = torch.device("cuda", miner.device)
    every = W.window_indices_cuda(w.wb, w.wbits, w.k_begin, w.total - first, dev, first)
    return every if ntz == 0 else every[_depths(miner, w)[first:] >= ntz]


def _scan_whole(miner, w, ntz):
    """One call with room for every candidate: (idx, depths)."""
    r, idx, dep, k_done = miner.scan_cuda_page(w.nonce, ntz, w.wb, w.wbits, w.k_begin, w.k_end,
                                               max_hits=max(w.total if ntz == 0 else w.total // 8, MIN_HITS))
    st = miner.last_scan_device_stats
    assert (r, k_done, st.rounds, st.candidates) == (EXHAUSTED, w.k_end, 1, w.total), (w.name, ntz)
    return idx, dep


@pytest.mark.parametrize("order", ["descending", "ascending"])
def test_group_sizes(miner, order):
    """Every window of family H at N = 3, 1 and 0, largest first or smallest first."""
    fam = sorted(W.family_h(), key=lambda w: w.total, reverse=order == "descending")
    assert len(fam) == 11
    t0, wrong, lines = time.perf_counter(), [], []
    for w in fam:
        for ntz in H_NTZ:
            t1 = time.perf_counter()
            try:
                idx, dep = _scan_whole(miner, w, ntz)
            except distpow.DpowError as e:     # the call's own check refused its list: wrong too, and the walk goes on
                wrong.append((w.name, ntz, str(e), None))
                continue
            dt = time.perf_counter() - t1
            want = _expected(miner, w, ntz)
            if ntz == 0:
                assert want.numel() == w.total
            ok = torch.equal(idx, want)
            # (the digest kernel against itself: it says only that depths and entries belong together)
            ok_dep = ok and torch.equal(dep, _depths(miner, w)[_depths(miner, w) >= ntz])
            if not (ok and ok_dep):
                wrong.append((w.name, ntz, idx.numel(), want.numel()))
            lines.append(f"{w.name}/N{ntz} {want.numel()} hits {dt * 1e3:.2f} ms")
            if ntz == 3 and w.name in ("g512", "g4096"):
                ref = miner.scan(w.nonce, 3, w.wb, w.wbits, w.k_begin, w.k_end)
                if (idx.tolist(), dep.tolist()) != ([h.global_idx for h in ref], [h.tz for h in ref]):
                    wrong.append((w.name, "Miner.scan", idx.numel(), len(ref)))
            del idx, dep, want
    print(f"family H {order}: {len(fam)} windows x N = 3, 1, 0 in {time.perf_counter() - t0:.3f} s (the reference "
          f"included where first)\n  " + "\n  ".join(lines))
    assert not wrong, wrong      # (window, N, entries, expected entries)
    _still_usable(miner)


# ---- 3. page cuts ---------------------------------------------------------------------------------------
def _pages_expected(miner, w, ntz, max_hits):
    """[(status, entries, k_done)] of paging the window with `max_hits`, from the reference's per-group
    totals: each page is a call from the last k_done, whose slice, group and cut are its own."""
    hit = (_depths(miner, w) >= ntz)
    pages, first = [], 0
    while True:
        (lo, hi, group, n_blocks), = W.scan_dev_slices(first, w.total)
        pad = torch.zeros(n_blocks * group, dtype=torch.int32, device=hit.device)
        pad[:hi - lo] = hit[lo:hi]
        prefix, s = [], 0
        for t in pad.view(n_blocks, group).sum(1).tolist():
            s += t
            prefix.append(s)
        if s <= max_hits:
            pages.append((EXHAUSTED, s, w.k_end))
            return pages
        n_fit = distpow.scan_device_cut(prefix, max_hits)
        assert 0 < n_fit < n_blocks and (n_fit * group) % (1 << w.rbits) == 0
        first += n_fit * group
        pages.append((MORE, prefix[n_fit - 1], w.k_begin + (first >> w.rbits)))


@pytest.mark.parametrize("max_hits", [MIN_HITS, MIN_HITS + 1024 - 1])
def test_paging_middle_group(miner, max_hits):
    """The ragged group-1024 window at N = 1 in pages: the group falls to 512 and 256 as the window
    left shrinks, and every page's status, entry count and k_done are the reference's."""
    w = W.family_h_window("g1024")
    want_pages = _pages_expected(miner, w, 1, max_hits)
    assert len(want_pages) >= 12 and [p[0] for p in want_pages] == [MORE] * (len(want_pages) - 1) + [EXHAUSTED]
    t0, got, idxs, k = time.perf_counter(), [], [], w.k_begin
    for _ in want_pages:
        r, idx, dep, k = miner.scan_cuda_page(w.nonce, 1, w.wb, w.wbits, k, w.k_end, max_hits=max_hits)
        got.append((r, idx.numel(), k))
        idxs.append(idx)
        if r != MORE:
            break
    dt = time.perf_counter() - t0
    assert got == want_pages
    assert torch.equal(torch.cat(idxs), _expected(miner, w, 1))
    print(f"g1024 at N = 1, max_hits {max_hits}: {len(got)} pages, {sum(n for _, n, _ in got)} hits, {dt * 1e3:.1f} ms")
    _still_usable(miner)


@pytest.mark.parametrize("g", [512, 8192])
def test_first_page_pins_the_group(miner, g):
    """N = 0: every group holds g entries, so room for 16384 + g - 1 takes 16384 / g whole groups.  A
    library whose group were g / 2 would return 16384 + g / 2 entries: the restated rule is the
    library's."""
    w = W.family_h_window(f"g{g}")
    r, idx, dep, k_done = miner.scan_cuda_page(w.nonce, 0, w.wb, w.wbits, w.k_begin, w.k_end, max_hits=MIN_HITS + g - 1)
    assert (r, idx.numel(), k_done) == (MORE, MIN_HITS, w.k_begin + (MIN_HITS >> w.rbits))
    dev = torch.device("cuda", miner.device)
    assert torch.equal(idx, W.window_indices_cuda(w.wb, w.wbits, w.k_begin, MIN_HITS, dev))
    _still_usable(miner)


def test_cut_inside_second_slice(miner):
    """A call of two slices whose room ends inside the second: 2^28 local indices at group 16384 placed
    whole, then the leading groups of 4097 groups of 512 that fit, by brute force over Miner.scan's
    list.  With no room left the call takes the second slice's leading empty groups and places
    nothing from it."""
    w = W.second_slice_window()
    t0 = time.perf_counter()
    ref = [h.global_idx for h in miner.scan(w.nonce, 3, w.wb, w.wbits, w.k_begin, w.k_end)]
    t_ref = time.perf_counter() - t0
    dev = torch.device("cuda", miner.device)
    ref_t = torch.tensor(ref, dtype=torch.int64, device=dev)
    (lo1, hi1, g1, nb1), (lo2, hi2, g2, nb2) = W.scan_dev_slices(w.k_begin << w.rbits, w.k_end << w.rbits)
    assert (g1, nb1, g2, nb2) == (16384, 16384, 512, 4097)

    def local(g):     # the local index of a global one of this partition
        assert (g & 0xFF) >> w.rbits == w.wb
        return (g >> 8) << w.rbits | (g & ((1 << w.rbits) - 1))

    h1 = sum(1 for g in ref if local(g) < hi1)
    totals = [0] * nb2
    for g in ref[h1:]:
        totals[(local(g) - lo2) // g2] += 1
    assert h1 >= MIN_HITS and 40 < sum(totals) == len(ref) - h1 and totals[0] == 0
    want = {}
    for r in (0, 1, 40):
        n_fit = s = 0
        for t in totals:          # brute force: the leading groups whose hits fit r
            if s + t > r:
                break
            n_fit, s = n_fit + 1, s + t
        want[r] = (s, (lo2 + n_fit * g2) >> w.rbits)
    assert want[0][0] == 0 and want[0][1] > lo2 >> w.rbits and len({k for _, k in want.values()}) >= 2
    t0 = time.perf_counter()
    for r, (placed, k_cut) in want.items():
        st, idx, dep, k_done = miner.scan_cuda_page(w.nonce, 3, w.wb, w.wbits, w.k_begin, w.k_end, max_hits=h1 + r)
        assert (st, miner.last_scan_device_stats.rounds, idx.numel(), k_done) == (MORE, 2, h1 + placed, k_cut), r
        assert torch.equal(idx, ref_t[:h1 + placed]), r
        st, idx2, dep2, k_done = miner.scan_cuda_page(w.nonce, 3, w.wb, w.wbits, k_cut, w.k_end, max_hits=MIN_HITS)
        assert (st, k_done) == (EXHAUSTED, w.k_end) and torch.equal(idx2, ref_t[h1 + placed:]), r
    print(f"two slices at N = 3: {len(ref)} hits, {h1} in the first slice, cuts {want}; Miner.scan {t_ref:.3f} s, "
          f"six calls {time.perf_counter() - t0:.3f} s")
    _still_usable(miner)
