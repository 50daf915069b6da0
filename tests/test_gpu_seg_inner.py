"""GPU: the segment-inner kernels (md5_search_si.h search_body_si) find exactly what the
index-ordered kernels find.

The path is forced with DPOW_DIAG_SEG_INNER=1 (read at dpow_open), so N = 8 searches -- ~1 hit
per 2^32 candidates -- run it; the same searches with the knob at 0 run the index-ordered
kernels.  Every hit of a window is walked (each search resumes behind the last hit), so hits in
every segment, below and above unaligned window ends, are compared; the first one is checked
against the byte-wise oracle on the 4096 k before it.  One context is open at a time: a search
that starts within 100 ms of another context's use plans for a shared device (plan.h kYoungNs)
and would run short index-ordered launches.
"""
import ctypes
import threading
import time

import pytest

import distpow
from distpow import CANCELLED, EXHAUSTED, FOUND
from distpow._lib import LaunchTime

pytestmark = pytest.mark.gpu

SEG = 1 << 24
NONCE8 = [14, 186, 238, 163, 194, 216, 84, 90]  # 7 hits in the 4-segment window below
# name -> (nonce, ntz, worker_byte, worker_bits, k_begin, k_end)
CASES = {
    # 12 segments from an unaligned k at workerBits 0: 5.2e10 candidates
    # (the nonce: the first of random.Random(1)'s 4-byte nonces after [1,2,3,4], [2,2,2,2] and [5,6,7,8]
    # whose index-ordered search has hits in >= 8 of the 12 segments: 17 hits in 9; those have 7, 7, 6)
    "wb0": ([68, 32, 130, 60], 8, 0, 0, SEG + 12345, 13 * SEG + 12345),
    # 40 segments of 2^29 candidates from an unaligned k at workerBits 3
    "wb3": ([1, 2, 3, 4], 8, 5, 3, 3 * SEG + 777, 43 * SEG + 777),
    # R = 1: 400 segments of 2^24 candidates
    "wb8": ([1, 2, 3, 4], 8, 1, 8, SEG, 401 * SEG),
    # L = 5: k >> 24 carries across a byte
    "l5": ([2, 2, 2, 2], 8, 0, 0, (1 << 32) + 254 * SEG, (1 << 32) + 257 * SEG),
    # a window across k = 2^32 (two launches: the chunk length changes)
    "l45": ([1, 2, 3, 4], 8, 0, 0, (1 << 32) - 2 * SEG - 1000, (1 << 32) + 2 * SEG + 1000),
    # a second covered W0: an 8-byte nonce (W0 = 2)
    "w2": (NONCE8, 8, 0, 0, SEG + 5, 5 * SEG + 5),
}


def _secret_of(g):
    out, k = [g & 0xFF], g >> 8
    while k:
        out.append(k & 0xFF)
        k >>= 8
    return bytes(out)


def _kinds(m):
    """Launch kinds of the context's last search (dpow_diag_search_launches: 2 = segment-inner)."""
    t0 = ctypes.c_int64()
    buf = (LaunchTime * 32)()
    n = distpow.lib().dpow_diag_search_launches(m._ctx, ctypes.byref(t0), buf, 32)
    assert n >= 0
    return [x.kind for x in buf[:min(n, 32)]]


def _all_hits(miner, nonce, ntz, wb, wbits, k0, k1, cap=2000, kinds=None):
    """Every hit of a window, in order: repeated searches resuming after each hit."""
    hits, bound_k = [], k0
    rb = 8 - wbits % 9
    while bound_k < k1 and len(hits) < cap:
        r = miner.search(nonce, ntz, wb, wbits, bound_k, k1)
        if kinds is not None:
            kinds.append(_kinds(miner))
        if r.status != FOUND:
            assert r.status == EXHAUSTED
            break
        hits.append(r.global_idx)
        # resume at the same k for partitions with several thread bytes per k
        k = r.global_idx >> 8
        tbs = [((wb << rb) | j) & 255 for j in range(1 << rb)]
        for t in [t for t in tbs if t > (r.global_idx & 255)]:
            g = (k << 8) | t
            if distpow.verify(nonce, _secret_of(g), ntz):
                hits.append(g)
        bound_k = k + 1
    return hits


@pytest.fixture(scope="module")
def forced():
    """(the knob-1 miner, {case: hits of the knob-0 path}): the reference is computed once."""
    if distpow.device_count() == 0:
        pytest.fail("no HIP device visible: gpu tests must run on the GPU box")
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("DPOW_DIAG_SEG_INNER", "0")
        with distpow.Miner(0) as m0:
            ref = {}
            for name, c in CASES.items():
                kinds = []
                ref[name] = _all_hits(m0, *c, kinds=kinds)
                assert all(k != 2 for ks in kinds for k in ks), (name, kinds)
        mp.setenv("DPOW_DIAG_SEG_INNER", "1")
        m1 = distpow.Miner(0)
    finally:
        mp.undo()
    yield m1, ref
    m1.close()


@pytest.mark.parametrize("name", list(CASES))
def test_hit_set_equals_the_index_ordered_path(forced, oracle, name):
    m1, ref = forced
    nonce, ntz, wb, wbits, k0, k1 = CASES[name]
    kinds = []
    t = time.perf_counter()
    hits = _all_hits(m1, nonce, ntz, wb, wbits, k0, k1, kinds=kinds)
    print(f"{name}: {len(hits)} hits, {len(kinds)} searches in {time.perf_counter() - t:.2f} s, kinds {kinds[0]}")
    # the first search covers the whole window: every md5 launch of it is segment-inner
    assert kinds[0] and all(k == 2 for k in kinds[0]), kinds[0]
    assert len(kinds[0]) == 1 or (name == "l45" and len(kinds[0]) == 2)  # one launch per chunk length
    assert hits == ref[name] and hits, (name, hits, ref[name])
    assert hits == sorted(hits) and all(k0 <= g >> 8 < k1 for g in hits)
    k_hit = hits[0] >> 8
    exp = oracle.mine_window(nonce, ntz, wb, wbits, max(k0, k_hit - 4095), k_hit + 1)
    assert exp is not None and exp[1] == hits[0], (exp, hits[0])
    if name == "wb0":  # hits in most of the 12 segments: every segment's constants are exercised
        segs = {(g >> 8) >> 24 for g in ref[name]}
        assert len(segs) >= 8, sorted(segs)


def test_exhausted_window_ending_mid_segment_counts_exactly(forced):
    m1, _ = forced
    k0, k1 = SEG + 4096 + 17, 5 * SEG + (SEG >> 1)
    m1.reset_stats()
    r = m1.search([1, 2, 3, 4], 32, 0, 0, k0, k1)
    assert r.status == EXHAUSTED
    s = m1.stats()
    assert s.candidates == (k1 - k0) * 256 and s.launches == 1 and s.kernel_ms > 0
    assert _kinds(m1) == [2]


def test_bound_excludes_hits_at_or_above_it(forced):
    m1, ref = forced
    nonce, ntz, wb, wbits, k0, k1 = CASES["wb3"]
    g = ref["wb3"][0]
    r = m1.search(nonce, ntz, wb, wbits, k0, k1, bound=g)
    assert r.status == EXHAUSTED, r
    r = m1.search(nonce, ntz, wb, wbits, k0, k1, bound=g + 1)
    assert r.status == FOUND and r.global_idx == g
    if len(ref["wb3"]) > 1:  # a bound between two hits: the lower one, found out of index order or not
        r = m1.search(nonce, ntz, wb, wbits, k0, k1, bound=ref["wb3"][1])
        assert r.status == FOUND and r.global_idx == g


def test_cancel_mid_launch(forced):
    """A cancel 50 ms into one segment-inner launch of 255 segments (2^40 candidates) stops it.
    The latency is printed for comparison with the bench's cancel_latency_ms (the index-ordered
    kernel's); the poll interval -- once per poll_wb hashed wave-blocks -- is the same."""
    m1, _ = forced
    out = {}

    def run():
        out["r"] = m1.search([1, 2, 3, 4], 32, 0, 0, 1 << 24, 1 << 32)
        out["t_end"] = time.perf_counter()

    th = threading.Thread(target=run)
    th.start()
    time.sleep(0.05)
    t_cancel = time.perf_counter()
    m1.cancel()
    th.join(timeout=30)
    m1.clear_cancel()
    assert not th.is_alive()
    assert out["r"].status == CANCELLED
    assert _kinds(m1) == [2]
    print(f"segment-inner cancel latency {(out['t_end'] - t_cancel) * 1e3:.3f} ms")
    assert m1.search([1, 2, 3, 4], 3, 0, 0, 0, 1 << 10).status == FOUND
