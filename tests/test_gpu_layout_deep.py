"""GPU: the N >= 8 and N = 9 paths of every specialised layout <NBLK, W0, SH> of
md5_search_kernel.h against hit lists that do not come from this library.

tests/golden/layout_deep_hits.json lists, per layout, every N >= 8 hit of a workerBits = 0 window
with its trailing-zero count.  The lists are the CPU scanner's (tests/golden/fast_scan.c, whose
one- and two-final-block layouts gen_golden.py cross-checks against the byte-wise oracle), each
entry is re-hashed with hashlib and the cases are shown to cover all 72 layouts
(tests/test_layout_deep_golden.py).  What they reach that nothing else does: full_check -- the
re-hash of one lane's candidate through the non-pipelined md5_tail<NBLK, W0, SH, 1> with the
launch's segment additions -- in every layout; a wrong one rejects every true N >= 9 hit, which
the host's re-verification cannot see.  Every assertion is equality with the fixture.

Per case: the N = 8 walk of the window (D-equality or the two-block prefilter, the narrow SH = 3
kernels, a launch that spans two 2^24-k segments), an N = 32 pass that counts every candidate
once, the N = 9 search of the whole window and from the hit's own segment (non-zero and zero
segment addition), and the same at workerBits 3 (the general kernel: a wave-block's lanes span
several k) and 8 in the deep entry's partition.  The context is the default one, no DPOW_DIAG_*
knob: the four segment-inner layouts run their index-ordered kernels here, and no launch may be
segment-inner (kind 2), which tests/test_gpu_seg_inner_golden.py pins.

A window is at most two segments (8.6e9 candidates at workerBits 0).  On an MI355X the 234 tests
take 16 s together (1.6 s of it opening the context): per case the N = 8 walk 0.03-0.04 s and with
the N = 32 pass 0.07-0.08 s on a one-block layout, 0.07 s and 0.14-0.15 s on a two-block one; the
N = 9 searches and walk 0.03-0.18 s; the two partitions 0.01-0.02 s; the tiny ranges under 0.03 s.
Each test prints its time (pytest -s).
"""
import ctypes
import hashlib
import json
import os
import time

import pytest

import distpow
from distpow import EXHAUSTED, FOUND
from distpow._lib import LaunchTime

pytestmark = pytest.mark.gpu

SEG = 1 << 24
NTZ = 8
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_deep_hits.json")) as _f:
    CASES = {c["name"]: c for c in json.load(_f)["cases"]}
NAMES = list(CASES)


def _secret_of(g):
    out, k = [g & 0xFF], g >> 8
    while k:
        out.append(k & 0xFF)
        k >>= 8
    return bytes(out)


def _tz(nonce, g):
    h = hashlib.md5(bytes(nonce) + _secret_of(g)).hexdigest()
    return len(h) - len(h.rstrip("0"))


def _thread_bytes(wb, wbits):
    """worker.go:302-316 (gen_golden.thread_bytes)."""
    rbits = 8 - wbits % 9
    return [((wb << rbits) | i) & 0xFF for i in range(1 << rbits)]


def _expected(case, ntz=NTZ, wb=0, wbits=0, k0=None):
    """The list filtered to a partition, an N and a later begin."""
    tbs = set(_thread_bytes(wb, wbits))
    k0 = case["k_begin"] if k0 is None else k0
    return [g for g, tz in case["hits"] if tz >= ntz and (g & 0xFF) in tbs and k0 <= g >> 8]


def _kinds(m):
    """Kinds of the context's last search's launches (dpow_diag_search_launches: 2 = segment-inner)."""
    t0 = ctypes.c_int64()
    buf = (LaunchTime * 32)()
    n = distpow.lib().dpow_diag_search_launches(m._ctx, ctypes.byref(t0), buf, 32)
    assert 0 <= n <= 32
    return [x.kind for x in buf[:n]]


def _search(m, kinds, *args):
    r = m.search(*args)
    kinds += _kinds(m)
    return r


def _walk(m, kinds, nonce, ntz, wb, wbits, k0, k1):
    """Every hit of a window in index order: repeated searches, each resuming behind the last hit.
    The later thread bytes of a hit's k are hashed with hashlib."""
    tbs = _thread_bytes(wb, wbits)
    hits, k = [], k0
    while k < k1:
        r = _search(m, kinds, nonce, ntz, wb, wbits, k, k1)
        if r.status != FOUND:
            assert r.status == EXHAUSTED, r
            break
        g = r.global_idx
        assert r.secret == _secret_of(g) == distpow.secret_from_index(g), (g, r.secret)
        hits.append(g)
        hits += [(g >> 8) << 8 | t for t in sorted(tbs) if t > (g & 0xFF) and _tz(nonce, (g >> 8) << 8 | t) >= ntz]
        k = (g >> 8) + 1
    return hits


@pytest.fixture(scope="module")
def default_miner():
    """A context opened with no DPOW_DIAG_* knob in the environment (they are read at dpow_open)."""
    if distpow.device_count() == 0:
        pytest.fail("no HIP device visible: gpu tests must run on the GPU box")
    mp = pytest.MonkeyPatch()
    try:
        for name in [n for n in os.environ if n.startswith("DPOW_DIAG_")]:
            mp.delenv(name)
        m = distpow.Miner(0)
    finally:
        mp.undo()
    yield m
    m.close()


def _assert_found(r, g):
    assert r.status == FOUND and r.global_idx == g and r.secret == _secret_of(g), (r, g)


@pytest.mark.parametrize("name", NAMES)
def test_n8_walk_equals_the_list(default_miner, name):
    """N = 8, workerBits 0: the walked hits of the window are the list, the secrets are the indices'
    and an exhausted search of it counts every candidate once."""
    m, c, kinds = default_miner, CASES[name], []
    k0, k1 = c["k_begin"], c["k_end"]
    t = time.perf_counter()
    hits = _walk(m, kinds, c["nonce"], NTZ, 0, 0, k0, k1)
    t_walk = time.perf_counter() - t
    assert hits == [g for g, _ in c["hits"]] and hits
    m.reset_stats()
    r = _search(m, kinds, c["nonce"], 32, 0, 0, k0, k1)
    assert r.status == EXHAUSTED
    assert m.stats().candidates == (k1 - k0) * 256
    assert kinds and 2 not in kinds
    print(f"{name} <{c['nblk']},{c['w0']},{c['sh']}>: {len(hits)} hits walked in {t_walk:.2f} s, "
          f"with the N = 32 pass {time.perf_counter() - t:.2f} s")


@pytest.mark.parametrize("name", NAMES)
def test_n9_search_returns_the_first_deep_entry(default_miner, name):
    """full_check: an N = 9 search of the whole window returns the first entry with tz >= 9, past
    every tz = 8 entry before it (D-equality / prefilter false positives at N = 9), or EXHAUSTED when
    the list has none; the same from the begin of the hit's own segment, where the launch reaches it
    with a zero segment addition; the N = 9 walk gives every tz >= 9 entry."""
    m, c, kinds = default_miner, CASES[name], []
    exp = _expected(c, ntz=9)
    assert bool(exp) == c["deep"]
    t = time.perf_counter()
    r = _search(m, kinds, c["nonce"], 9, 0, 0, c["k_begin"], c["k_end"])
    if exp:
        _assert_found(r, exp[0])
        own = max(c["k_begin"], ((exp[0] >> 8) // SEG) * SEG)
        _assert_found(_search(m, kinds, c["nonce"], 9, 0, 0, own, c["k_end"]), exp[0])
        _assert_found(_search(m, kinds, c["nonce"], 9, 0, 0, exp[0] >> 8, (exp[0] >> 8) + 1), exp[0])
    else:
        assert r.status == EXHAUSTED, r
    assert _walk(m, kinds, c["nonce"], 9, 0, 0, c["k_begin"], c["k_end"]) == exp
    assert kinds and 2 not in kinds
    print(f"{name}: N = 9 -> {exp[:1]} behind {sum(1 for g, _ in c['hits'] if not exp or g < exp[0])} "
          f"shallower entries, {time.perf_counter() - t:.2f} s")


@pytest.mark.parametrize("name", NAMES)
def test_partitions_from_one_list(default_miner, name):
    """The partition of the deep entry (of the first entry where the list has no deep one) at
    workerBits 3 and 8, filtered from the one list: the N = 9 search and the N = 8 walk."""
    m, c, kinds = default_miner, CASES[name], []
    target = (_expected(c, ntz=9) or _expected(c))[0]
    t = time.perf_counter()
    for wbits in (3, 8):
        wb = (target & 0xFF) >> (8 - wbits)
        assert (target & 0xFF) in _thread_bytes(wb, wbits)
        exp9, exp8 = _expected(c, ntz=9, wb=wb, wbits=wbits), _expected(c, wb=wb, wbits=wbits)
        assert target in exp8 and (not c["deep"] or exp9[0] == target)
        r = _search(m, kinds, c["nonce"], 9, wb, wbits, c["k_begin"], c["k_end"])
        if exp9:
            _assert_found(r, exp9[0])
        else:
            assert r.status == EXHAUSTED, r
        assert _walk(m, kinds, c["nonce"], NTZ, wb, wbits, c["k_begin"], c["k_end"]) == exp8
    assert kinds and 2 not in kinds
    print(f"{name}: partitions of 8 and 256 in {time.perf_counter() - t:.2f} s")
