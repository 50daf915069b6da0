"""GPU: the scan (dpow_scan, Miner.scan) -- every hit of a window, in index order, with depths.

Every assertion is equality with something that does not come from the scan: a Python loop over
hashlib (dense windows, every candidate at N = 0), the committed CPU-scanned hit lists
(tests/golden/layout_deep_hits.json) as whole lists, and the specialised search kernels, which
must return every scanned hit of a fresh window when started at or before it.  The N = 0 tests are
the test of the hit sink's ordering: a lost, duplicated or stale entry shows as a wrong index.

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
from distpow import CANCELLED, DPOW_K_LIMIT, EINVAL, ERANGE, EXHAUSTED, FOUND, MORE, ScanHit
from distpow import _lib

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_deep_hits.json")) as _f:
    CASES = {c["name"]: c for c in json.load(_f)["cases"]}
NAMES = list(CASES)


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


def _reference(nonce, ntz, wb, wbits, k0, k1):
    """The reference's enumeration (k outer, threadByte inner) with hashlib: every hit as a ScanHit."""
    base, tbs, out = hashlib.md5(bytes(nonce)), _thread_bytes(wb, wbits), []
    for k in range(k0, k1):
        for tb in tbs:
            sec = _secret_of(k << 8 | tb)
            h = base.copy()
            h.update(sec)
            hx = h.hexdigest()
            tz = 32 - len(hx.rstrip("0"))
            if tz >= ntz:
                out.append(ScanHit(k << 8 | tb, tz, sec))
    return out


def _nonce(n, salt=0):
    rnd = random.Random(1000 * n + salt)
    return bytes(rnd.randrange(256) for _ in range(n))


_REF = {}


def _ref_cached(nlen, wb, wbits, k0, k1):
    """All candidates of a window with their depths, computed once and filtered per N."""
    key = (nlen, wb, wbits, k0, k1)
    if key not in _REF:
        _REF[key] = _reference(_nonce(nlen), 0, wb, wbits, k0, k1)
    return _REF[key]


@pytest.mark.parametrize("window", [(0, 300), (65536 - 40, 65536 + 40)], ids=["k0", "k64k"])
@pytest.mark.parametrize("part", [(0, 0), (5, 3)], ids=["all", "wb5of8"])
@pytest.mark.parametrize("nlen", [0, 4, 47, 48, 55, 56, 63, 64, 119])
def test_dense_equals_hashlib(miner, nlen, part, window):
    """One and two final blocks, a midstate, the 55/56 edge; k = 0 and the chunk lengths 1 -> 2 -> 3."""
    (wb, wbits), (k0, k1) = part, window
    every = _ref_cached(nlen, wb, wbits, k0, k1)
    assert len(every) == (k1 - k0) * (256 >> wbits) <= 76800
    t = time.perf_counter()
    for ntz in (1, 2):
        got = miner.scan(_nonce(nlen), ntz, wb, wbits, k0, k1)
        assert got == [h for h in every if h.tz >= ntz]
        assert got or ntz > 1
    print(f"len {nlen} part {part} k {window}: {time.perf_counter() - t:.3f} s")


@pytest.mark.parametrize("wb,wbits,k1", [(0, 0, 512), (167, 8, 4096)], ids=["wbits0", "wbits8"])
def test_every_candidate(miner, wb, wbits, k1):
    """N = 0: the answer is every index of the partition once, in order, each depth hashlib's."""
    nonce = _nonce(4, 1)
    t = time.perf_counter()
    got = miner.scan(nonce, 0, wb, wbits, 0, k1)
    t_scan = time.perf_counter() - t
    tbs = _thread_bytes(wb, wbits)
    assert [h.global_idx for h in got] == [k << 8 | tb for k in range(k1) for tb in tbs]
    assert len(got) == (131072 if wbits == 0 else 4096)
    assert got == _reference(nonce, 0, wb, wbits, 0, k1)
    print(f"{len(got)} candidates scanned in {t_scan:.3f} s")


def _listed(case, ntz, wb=0, wbits=0):
    tbs = set(_thread_bytes(wb, wbits))
    return [(g, tz) for g, tz in case["hits"] if tz >= ntz and (g & 0xFF) in tbs]


def _pairs(hits):
    for h in hits:
        assert h.secret == _secret_of(h.global_idx)
    return [(h.global_idx, h.tz) for h in hits]


@pytest.mark.parametrize("name", NAMES)
def test_committed_lists(miner, name):
    """The CPU-scanned list of every layout's window, as a whole: N = 8 and N = 9, with depths."""
    c = CASES[name]
    t = time.perf_counter()
    assert _pairs(miner.scan(c["nonce"], 8, 0, 0, c["k_begin"], c["k_end"])) == _listed(c, 8)
    assert _pairs(miner.scan(c["nonce"], 9, 0, 0, c["k_begin"], c["k_end"])) == _listed(c, 9)
    print(f"{name}: {len(c['hits'])} hits, two scans in {time.perf_counter() - t:.2f} s")


@pytest.mark.parametrize("name", ["len04", "len51", "b2w12s0"])
def test_committed_lists_by_partition(miner, name):
    """workerBits 3: each of the 8 partitions' lists is the fixture's filtered by owner."""
    c = CASES[name]
    t = time.perf_counter()
    for wb in range(8):
        exp = [(g, tz) for g, tz in c["hits"] if (g & 255) >> 5 == wb]
        assert exp == _listed(c, 8, wb, 3)
        assert _pairs(miner.scan(c["nonce"], 8, wb, 3, c["k_begin"], c["k_end"])) == exp
    print(f"{name}: 8 partitions in {time.perf_counter() - t:.2f} s")


@pytest.mark.parametrize("nlen", [4, 50])
def test_specialised_kernels_agree_off_the_fixtures(miner, nlen):
    """Fresh windows no fixture covers: every scanned hit is what Miner.search returns from its k
    and from behind the previous hit, and the rest of the window is exhausted."""
    k0, k1, ntz = 1 << 24, (1 << 24) + (1 << 21), 7
    t = time.perf_counter()
    used = 0
    for seed in range(32):  # seeds whose window has a hit (about 2 are expected per window)
        nonce = _nonce(nlen, 7000 + seed)
        hits = miner.scan(nonce, ntz, 0, 0, k0, k1)
        if not hits:
            continue
        used += 1
        prev_k = k0 - 1
        for h in hits:
            k = h.global_idx >> 8
            assert k0 <= k < k1 and h.tz >= ntz
            first = next(x for x in hits if x.global_idx >> 8 == k)  # the first hit of that k
            r = miner.search(nonce, ntz, 0, 0, k, k1)
            assert (r.status, r.global_idx, r.secret) == (FOUND, first.global_idx, first.secret)
            if k > prev_k:
                r = miner.search(nonce, ntz, 0, 0, prev_k + 1, k + 1)
                assert (r.status, r.global_idx, r.secret) == (FOUND, first.global_idx, first.secret)
            prev_k = k
        assert miner.search(nonce, ntz, 0, 0, prev_k + 1, k1).status == EXHAUSTED
        if used == 4:
            break
    assert used == 4
    print(f"len {nlen}: 4 windows in {time.perf_counter() - t:.2f} s")


def test_paging(miner):
    nonce = _nonce(4, 2)
    pages, k = [], 0
    for want in (1, 2, 3, 4):
        r, hits, k = miner.scan_page(nonce, 0, 0, 0, k, 5, max_hits=256)
        assert (r, k, len(hits)) == (MORE, want, 256)
        pages += hits
    r, hits, k = miner.scan_page(nonce, 0, 0, 0, k, 5, max_hits=256)
    assert (r, k, len(hits)) == (EXHAUSTED, 5, 256)
    pages += hits
    assert pages == _reference(nonce, 0, 0, 0, 0, 5)
    assert miner.scan(nonce, 0, 0, 0, 0, 5) == pages
    assert miner.scan(nonce, 0, 0, 0, 0, 5, max_hits=256) == pages
    with pytest.raises(distpow.DpowError) as e:
        miner.scan_page(nonce, 0, 0, 0, 0, 5, max_hits=255)
    assert e.value.code == EINVAL


def test_overflow_reruns_in_halves(miner, monkeypatch):
    """DPOW_DIAG_SCAN_CAP=256 shrinks the hit list, not the slice: the same list from more launches."""
    nonce = _nonce(4)
    monkeypatch.delenv("DPOW_DIAG_SCAN_CAP", raising=False)
    plain = miner.scan(nonce, 1, 0, 0, 0, 1024)
    launches = miner.last_scan_stats.launches
    monkeypatch.setenv("DPOW_DIAG_SCAN_CAP", "256")
    small = miner.scan(nonce, 1, 0, 0, 0, 1024)
    launches_small = miner.last_scan_stats.launches
    monkeypatch.delenv("DPOW_DIAG_SCAN_CAP")
    assert small == plain and len(plain) > 256
    assert launches_small > launches >= 1
    print(f"{len(plain)} hits: {launches} launches, {launches_small} with a 256-entry list")


def test_cancel_raised_on_entry(miner):
    miner.cancel()
    try:
        r, hits, k_done = miner.scan_page([1, 2, 3, 4], 2, 0, 0, 7, 64)
    finally:
        miner.clear_cancel()
    assert (r, hits, k_done) == (CANCELLED, [], 7)
    assert miner.last_scan_stats.launches == 0


def test_cancel_mid_scan(miner, golden):
    k_end, out = 1 << 30, {}

    def run():
        out["r"] = miner.scan_page([1, 2, 3, 4], 32, 0, 0, 0, k_end)
        out["t_end"] = time.perf_counter()

    th = threading.Thread(target=run)
    th.start()
    time.sleep(0.05)
    t_cancel = time.perf_counter()
    miner.cancel()
    th.join(timeout=30)
    miner.clear_cancel()
    assert not th.is_alive()
    r, hits, k_done = out["r"]
    print(f"scan cancel latency {(out['t_end'] - t_cancel) * 1e3:.2f} ms at k {k_done}, "
          f"{miner.last_scan_stats.launches} launches")
    assert r == CANCELLED and hits == [] and 0 <= k_done < k_end
    e = next(e for e in golden["first_hits"] if e["nonce"] == [1, 2, 3, 4] and e["ntz"] == 6)
    res = miner.mine([1, 2, 3, 4], 6)
    assert (res.status, res.global_idx, list(res.secret)) == (FOUND, e["global_idx"], e["secret"])


def test_argument_errors(miner):
    L = distpow.lib()
    arr = (_lib.ScanHitC * 256)()
    n, kd = ctypes.c_size_t(), ctypes.c_uint64()
    pn, pk = ctypes.byref(n), ctypes.byref(kd)
    nonce = b"\x01\x02\x03\x04"

    def call(nonce=nonce, nlen=4, wb=0, k0=0, k1=4, out=arr, max_hits=256, n_hits=pn, k_done=pk):
        return L.dpow_scan(miner._ctx, nonce, nlen, 1, wb, 0, k0, k1, out, max_hits, n_hits, k_done, None)

    assert call(out=None) == EINVAL
    assert call(n_hits=None) == EINVAL
    assert call(k_done=None) == EINVAL
    assert call(nonce=None) == EINVAL
    assert call(wb=256) == EINVAL
    assert call(k0=5) == EINVAL
    assert call(nonce=bytes(_lib.DPOW_MAX_NONCE + 1), nlen=_lib.DPOW_MAX_NONCE + 1) == EINVAL
    assert call(max_hits=255) == EINVAL
    assert call(k1=DPOW_K_LIMIT + 1) == ERANGE
    assert L.dpow_scan(None, nonce, 4, 1, 0, 0, 0, 4, arr, 256, pn, pk, None) == EINVAL
    # an empty window is exhausted without a launch; N > 32 scans and finds nothing
    assert miner.scan_page(nonce, 1, 0, 0, 9, 9) == (EXHAUSTED, [], 9)
    assert miner.last_scan_stats.launches == 0
    assert miner.scan_page(nonce, 33, 0, 0, 0, 64) == (EXHAUSTED, [], 64)
    assert miner.last_scan_stats.launches >= 1 and miner.last_scan_stats.candidates == 64 * 256
    # the context is still usable, and a scan leaves dpow_stats alone
    miner.reset_stats()
    assert call() == EXHAUSTED and kd.value == 4
    assert [h.global_idx for h in arr[:n.value]] == [h.global_idx for h in _reference(nonce, 1, 0, 0, 0, 4)]
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
            miner.scan([1, 2, 3, 4], 2, k_end=8)
        assert e.value.code == EINVAL
    finally:
        miner.attach_node(None)
    assert miner.scan([1, 2, 3, 4], 0, k_end=1)[0].global_idx == 0
