"""GPU: the census (dpow_census_window, Miner.census) -- for every depth d how many candidates of a
window end in at least d '0' characters, and the first of them.

Every assertion is equality with something that is not the census: a Python loop over hashlib
(dense windows, partial waves and steps), the committed CPU-scanned hit lists
(tests/golden/layout_deep_hits.json), the specialised search kernels (first_ge[d] is what
Miner.search returns at d) and the scan (count_ge[d] is the length of its list).

Each test prints its time (pytest -s).
"""
import ctypes
import hashlib
import json
import os
import random
import threading
import time

import pytest

import distpow
from distpow import CANCELLED, DPOW_K_LIMIT, EINVAL, ERANGE, EXHAUSTED, FOUND, Census
from distpow import _lib

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_deep_hits.json")) as _f:
    CASES = {c["name"]: c for c in json.load(_f)["cases"]}
NAMES = list(CASES)
D = _lib.CENSUS_DEPTHS


def _secret_of(g):
    out, k = [g & 0xFF], g >> 8
    while k:
        out.append(k & 0xFF)
        k >>= 8
    return bytes(out)


def _thread_bytes(wb, wbits):
    """worker.go:302-316."""
    rbits = 8 - wbits % 9
    return sorted(((wb << rbits) | i) & 0xFF for i in range(1 << rbits))


def _nonce(n, salt=0):
    rnd = random.Random(1000 * n + salt)
    return bytes(rnd.randrange(256) for _ in range(n))


def _depths(nonce, wb, wbits, k0, k1):
    """The reference's enumeration (k outer, threadByte inner) with hashlib: [(global index, depth)]."""
    base, tbs, out = hashlib.md5(bytes(nonce)), _thread_bytes(wb, wbits), []
    for k in range(k0, k1):
        for tb in tbs:
            h = base.copy()
            h.update(_secret_of(k << 8 | tb))
            hx = h.hexdigest()
            out.append((k << 8 | tb, 32 - len(hx.rstrip("0"))))
    return out


def _census_of(pairs, d_from=0):
    """The census of [(global index, depth)] in index order, from depth d_from up, as a Census."""
    count, first, tz = [0] * D, [None] * D, [0] * D
    for g, t in pairs:
        for d in range(d_from, t + 1):
            count[d] += 1
            if first[d] is None:
                first[d], tz[d] = g, t
    return Census(tuple(count), tuple(first), tuple(tz), max((d for d in range(D) if count[d]), default=0))


def _same_from(c, exp, d_from):
    return (c.count_ge[d_from:], c.first_ge[d_from:], c.first_tz[d_from:]) == \
           (exp.count_ge[d_from:], exp.first_ge[d_from:], exp.first_tz[d_from:])


DENSE = {(0, 0): {"k0": (0, 300), "k64k": (65496, 65576)}, (5, 3): {"k0": (0, 2400), "k64k": (64336, 66736)}}


@pytest.mark.parametrize("window", ["k0", "k64k"])
@pytest.mark.parametrize("part", [(0, 0), (5, 3)], ids=["all", "wb5of8"])
@pytest.mark.parametrize("nlen", [0, 4, 47, 48, 55, 56, 63, 64, 119])
def test_dense_equals_hashlib(miner, nlen, part, window):
    """One and two final blocks, a midstate, the 55/56 edge; k = 0 and the chunk lengths 1 -> 2 -> 3.
    All 33 counts, firsts and depths; every window holds a depth >= 3, so the LDS path runs."""
    (wb, wbits), (k0, k1) = part, DENSE[part][window]
    pairs = _depths(_nonce(nlen), wb, wbits, k0, k1)
    assert len(pairs) == (k1 - k0) * (256 >> wbits) <= 76800
    assert any(t >= 3 for _, t in pairs)
    exp = _census_of(pairs)
    t = time.perf_counter()
    got = miner.census(_nonce(nlen), wb, wbits, k0, k1)
    dt = time.perf_counter() - t
    assert got == exp
    print(f"len {nlen} part {part} k [{k0}, {k1}): deepest {got.deepest}, {got.count_ge[3]} at >= 3, {dt:.3f} s")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_partial_waves_and_steps(miner, n):
    """Partition (167, 8) has one candidate per k: windows that end inside a wave and inside a step.
    A clamped inactive lane counted once would show as a count one too high."""
    nonce = _nonce(4, 1)
    exp = _census_of(_depths(nonce, 167, 8, 3, 3 + n))
    assert exp.count_ge[0] == n
    assert miner.census(nonce, 167, 8, 3, 3 + n) == exp


def _listed(case, wb=0, wbits=0):
    tbs = set(_thread_bytes(wb, wbits))
    return sorted((g, tz) for g, tz in case["hits"] if (g & 0xFF) in tbs)


@pytest.mark.parametrize("name", NAMES)
def test_committed_lists(miner, name):
    """The CPU-scanned list of every layout's window: counts, firsts and depths for d = 8..32."""
    c = CASES[name]
    exp = _census_of(_listed(c), 8)
    t = time.perf_counter()
    got = miner.census(c["nonce"], 0, 0, c["k_begin"], c["k_end"])
    dt = time.perf_counter() - t
    assert _same_from(got, exp, 8)
    assert got.count_ge[0] == (c["k_end"] - c["k_begin"]) * 256
    if c["hits"]:
        assert got.deepest == max(tz for _, tz in c["hits"])
    print(f"{name}: {len(c['hits'])} listed, deepest {got.deepest}, {miner.last_census_stats.launches} launches "
          f"in {dt * 1e3:.1f} ms ({miner.last_census_stats.kernel_ms:.1f} ms of kernel)")


@pytest.mark.parametrize("name", ["len04", "len51", "b2w12s0"])
def test_committed_lists_by_partition(miner, name):
    """workerBits 3: each partition's census is the fixture's filtered by owner, and the 8 sum to the whole."""
    c = CASES[name]
    t = time.perf_counter()
    whole = miner.census(c["nonce"], 0, 0, c["k_begin"], c["k_end"])
    total = [0] * D
    for wb in range(8):
        exp = sorted((g, tz) for g, tz in c["hits"] if (g & 255) >> 5 == wb)
        assert exp == _listed(c, wb, 3)
        got = miner.census(c["nonce"], wb, 3, c["k_begin"], c["k_end"])
        assert _same_from(got, _census_of(exp, 8), 8)
        total = [a + b for a, b in zip(total, got.count_ge)]
    assert tuple(total) == whole.count_ge
    print(f"{name}: the window and its 8 partitions in {time.perf_counter() - t:.2f} s")


@pytest.mark.parametrize("nlen", [4, 50])
def test_specialised_kernels_and_scan_agree_off_the_fixtures(miner, nlen):
    """Fresh windows no fixture covers: first_ge[d] is Miner.search's answer at every d, and
    count_ge[d] the length of the scan's list."""
    k0, k1 = 1 << 24, (1 << 24) + (1 << 21)
    t = time.perf_counter()
    for seed in range(2):
        nonce = _nonce(nlen, 9000 + seed)
        c = miner.census(nonce, 0, 0, k0, k1)
        assert c.count_ge[0] == (k1 - k0) * 256
        for d in range(1, c.deepest + 1):
            r = miner.search(nonce, d, 0, 0, k0, k1)
            assert (r.status, r.global_idx, r.secret) == (FOUND, c.first_ge[d], c.secret(d)), d
        if c.deepest < 32:
            assert miner.search(nonce, c.deepest + 1, 0, 0, k0, k1).status == EXHAUSTED
        for d in range(5, c.deepest + 1):
            hits = miner.scan(nonce, d, 0, 0, k0, k1)
            assert len(hits) == c.count_ge[d], d
            assert (hits[0].global_idx, hits[0].tz) == (c.first_ge[d], c.first_tz[d]), d
        print(f"len {nlen} seed {seed}: deepest {c.deepest}, count_ge[5..] {c.count_ge[5:c.deepest + 1]}")
    print(f"len {nlen}: 2 windows in {time.perf_counter() - t:.2f} s")


def test_launch_seams_and_merge(miner, golden):
    """Two launches, the second short: the census is the merge of its parts at the seam and off it."""
    nonce, k_end = [1, 2, 3, 4], (1 << 20) + (1 << 12) + 3
    t = time.perf_counter()
    whole = miner.census(nonce, 0, 0, 0, k_end)
    assert miner.last_census_stats.launches == 2
    assert miner.last_census_stats.candidates == whole.count_ge[0] == k_end * 256
    for k1 in (1 << 20, (1 << 20) - 1, (1 << 19) + 1):
        assert miner.census(nonce, 0, 0, 0, k1).merged(miner.census(nonce, 0, 0, k1, k_end)) == whole, k1
    e = next(e for e in golden["first_hits"] if e["nonce"] == nonce and e["ntz"] == 6)
    assert e["global_idx"] == 2532284 == whole.first_ge[6]
    assert whole.secret(6) == bytes(e["secret"])
    assert whole.count_ge[6] == len(miner.scan(nonce, 6, k_end=k_end))
    print(f"counts {whole.count_ge[:whole.deepest + 1]} in {time.perf_counter() - t:.2f} s")


def test_cancel_raised_on_entry(miner):
    miner.cancel()
    try:
        r, c, k_done = miner.census_page([1, 2, 3, 4], 0, 0, 7, 64)
    finally:
        miner.clear_cancel()
    assert (r, c, k_done) == (CANCELLED, Census.empty(), 7)
    assert miner.last_census_stats.launches == 0


def test_cancel_mid_census(miner, golden):
    nonce, k_end, out = [1, 2, 3, 4], 1 << 30, {}

    def run():
        out["r"] = miner.census_page(nonce, 0, 0, 0, k_end)
        out["t_end"] = time.perf_counter()

    th = threading.Thread(target=run)
    th.start()
    time.sleep(0.05)
    t_cancel = time.perf_counter()
    miner.cancel()
    th.join(timeout=30)
    miner.clear_cancel()
    assert not th.is_alive()
    r, c, k_done = out["r"]
    print(f"census cancel latency {(out['t_end'] - t_cancel) * 1e3:.2f} ms at k {k_done}, "
          f"{miner.last_census_stats.launches} launches")
    assert r == CANCELLED and 0 <= k_done < k_end
    assert c.count_ge[0] == k_done * 256
    # what it returned is the complete census of [0, k_done): the searches' answers below k_done
    for d in range(1, 5):
        s = miner.search(nonce, d, 0, 0, 0, max(k_done, 1))
        if k_done and s.status == FOUND:
            assert c.first_ge[d] == s.global_idx, d
        else:
            assert c.first_ge[d] is None, d
    e = next(e for e in golden["first_hits"] if e["nonce"] == nonce and e["ntz"] == 6)
    res = miner.mine(nonce, 6)
    assert (res.status, res.global_idx, list(res.secret)) == (FOUND, e["global_idx"], e["secret"])


def test_argument_errors(miner):
    L = distpow.lib()
    c, kd = _lib.CensusC(), ctypes.c_uint64()
    pc, pk = ctypes.byref(c), ctypes.byref(kd)
    nonce = b"\x01\x02\x03\x04"

    def call(nonce=nonce, nlen=4, wb=0, k0=0, k1=4, out=pc, k_done=pk):
        return L.dpow_census_window(miner._ctx, nonce, nlen, wb, 0, k0, k1, out, k_done, None)

    assert call(out=None) == EINVAL
    assert call(k_done=None) == EINVAL
    assert call(nonce=None) == EINVAL
    assert call(wb=256) == EINVAL
    assert call(k0=5) == EINVAL
    assert call(nonce=bytes(_lib.DPOW_MAX_NONCE + 1), nlen=_lib.DPOW_MAX_NONCE + 1) == EINVAL
    assert call(k1=DPOW_K_LIMIT + 1) == ERANGE
    assert L.dpow_census_window(None, nonce, 4, 0, 0, 0, 4, pc, pk, None) == EINVAL
    # an empty window is exhausted without a launch
    assert miner.census_page(nonce, 0, 0, 9, 9) == (EXHAUSTED, Census.empty(), 9)
    assert miner.last_census_stats.launches == 0
    # the context is still usable, and a census leaves dpow_stats alone
    miner.reset_stats()
    assert call() == EXHAUSTED and kd.value == 4
    assert Census._from_c(c) == _census_of(_depths(nonce, 0, 0, 0, 4))
    st = miner.stats()
    assert (st.searches, st.launches, st.candidates) == (0, 0, 0)


def test_node_slot_attached_is_refused(miner):
    class Slot(ctypes.Structure):
        """dpow_node_slot (include/dpow.h)."""
        _fields_ = [("best", ctypes.c_uint64), ("stop", ctypes.c_uint32), ("pad", ctypes.c_uint32 * 13)]

    slot = Slot()
    addr = ctypes.addressof(slot)
    distpow.lib().dpow_node_slot_reset(addr)
    miner.attach_node(addr)
    try:
        with pytest.raises(distpow.DpowError) as e:
            miner.census([1, 2, 3, 4], k_end=8)
        assert e.value.code == EINVAL
    finally:
        miner.attach_node(None)
    c = miner.census([1, 2, 3, 4], k_end=1)
    assert (c.count_ge[0], c.first_ge[0]) == (256, 0)
