"""GPU: every segment-inner kernel (md5_search_si.h search_body_si) against hit lists that do
not come from this library.

tests/golden/seg_inner_hits.json lists every N >= 8 hit of nine workerBits = 0 windows with its
trailing-zero count.  The lists are the CPU scanner's (tests/golden/fast_scan.c, cross-checked
against the byte-wise oracle by gen_golden.py --seg-inner) and each entry is re-hashed with
hashlib (tests/test_seg_inner_golden.py).  They reach what tests/test_gpu_seg_inner.py leaves
open: the W0 = 0 and W0 = 3 kernels, midstate nonces (64 and 76 bytes), the N > 8 branch of
hash_wave_block_si on every layout, chunk lengths 6 and 7, the top of the k range, partitions
filtered from one list, and bounds that land while the launch runs.  Every assertion is equality
with the fixture or a golden.

The lists (entries / entries with tz >= 9 / segments): w0 40/1/48, w1 22/1/32, w2 61/3/64,
w3 15/1/16, m0 7/0/8, m3 5/0/8, l56 5/1/8, l67 12/0/8, top 6/0/8.  On an MI355X the 48 tests
take 31 s together: the walks 0.3-1.4 s each, the N = 9 searches 0.1-2.4 s (w2: 64 segments, three
N = 9 hits walked), a partition 0.02-0.3 s, the mid-launch bounds 0.3-3.3 s (32 segments at
workerBits 0, 12 bounded searches and two probes).

The path is forced with DPOW_DIAG_SEG_INNER=1 (read at dpow_open) except in the default-policy
test.  One context is open at a time (plan.h kYoungNs: a search that starts within 100 ms of
another context's use plans for a shared device).
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
from distpow import EXHAUSTED, FOUND
from distpow._lib import LaunchTime

pytestmark = pytest.mark.gpu

SEG = 1 << 24
NTZ = 8
WALK_SEGS = 16  # a walk costs about hits * window / 2: longer windows are walked this far only
NAMES = ["w0", "w1", "w2", "w3", "m0", "m3", "l56", "l67", "top"]
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_inner_hits.json")) as _f:
    CASES = {c["name"]: c for c in json.load(_f)["cases"]}


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


def _expected(case, ntz=NTZ, wb=0, wbits=0, k0=None, k1=None):
    """The list filtered to a partition, an N and a sub-window."""
    tbs = set(_thread_bytes(wb, wbits))
    k0 = case["k_begin"] if k0 is None else k0
    k1 = case["k_end"] if k1 is None else k1
    return [g for g, tz in case["hits"] if tz >= ntz and (g & 0xFF) in tbs and k0 <= g >> 8 < k1]


def _n_chunk_lengths(k0, k1):
    """Launches of a window at k >= 2^24: one per chunk length (the planner splits there)."""
    return ((k1 - 1).bit_length() + 7) // 8 - (k0.bit_length() + 7) // 8 + 1


def _launches(m):
    """(t0, launches) of the context's last search (dpow_diag_search_launches: kind 2 = segment-inner)."""
    t0 = ctypes.c_int64()
    buf = (LaunchTime * 32)()
    n = distpow.lib().dpow_diag_search_launches(m._ctx, ctypes.byref(t0), buf, 32)
    assert 0 <= n <= 32
    return t0.value, list(buf[:n])


def _kinds(m):
    return [x.kind for x in _launches(m)[1]]


def _decided_ns(m):
    """Absolute host time (steady clock = time.perf_counter_ns) at which the last search's status
    was final (dpow_diag_search_times[3])."""
    tl = (ctypes.c_int64 * 8)()
    assert distpow.lib().dpow_diag_search_times(m._ctx, tl) == 0
    return _launches(m)[0] + tl[3]


def _walk(m, nonce, ntz, wb, wbits, k0, k1, first_kinds=None):
    """Every hit of a window in index order: repeated searches, each resuming behind the last hit.
    The later thread bytes of a hit's k are hashed with hashlib."""
    tbs = _thread_bytes(wb, wbits)
    hits, k, first = [], k0, True
    while k < k1:
        r = m.search(nonce, ntz, wb, wbits, k, k1)
        if first and first_kinds is not None:
            first_kinds.extend(_kinds(m))
        first = False
        if r.status != FOUND:
            assert r.status == EXHAUSTED, r
            break
        g = r.global_idx
        assert r.secret == _secret_of(g) == distpow.secret_from_index(g), (g, r.secret)
        hits.append(g)
        hits += [(g >> 8) << 8 | t for t in sorted(tbs) if t > (g & 0xFF) and _tz(nonce, (g >> 8) << 8 | t) >= ntz]
        k = (g >> 8) + 1
    return hits


class _Contexts:
    """One open context at a time: the forced one (knob 1) or the default-policy one (knob unset)."""

    def __init__(self):
        self.which, self.m = None, None

    def use(self, which):
        if self.which != which:
            self.close()
            mp = pytest.MonkeyPatch()
            try:
                if which == "forced":
                    mp.setenv("DPOW_DIAG_SEG_INNER", "1")
                else:
                    mp.delenv("DPOW_DIAG_SEG_INNER", raising=False)
                self.m = distpow.Miner(0)
            finally:
                mp.undo()
            self.which = which
        return self.m

    def close(self):
        if self.m is not None:
            self.m.close()
        self.which, self.m = None, None


@pytest.fixture(scope="module")
def ctxs():
    if distpow.device_count() == 0:
        pytest.fail("no HIP device visible: gpu tests must run on the GPU box")
    c = _Contexts()
    yield c
    c.close()


@pytest.fixture
def forced(ctxs):
    return ctxs.use("forced")


def test_default_policy_selects_segment_inner_at_n10(ctxs, golden):
    """Knob unset: [1,2,3,4] at N = 10 over segments 395 ... 398 is one segment-inner launch (plan.h:
    4 segments at N = 10) and returns the N = 10 deep golden (segment 397, chunk length 5)."""
    m = ctxs.use("default")
    e = next(x for x in golden["deep_hits"] if x["nonce"] == [1, 2, 3, 4] and x["ntz"] == 10)
    g10 = e["global_idx"]
    assert g10 == 1705794008571 and (g10 >> 8) // SEG == 397 and len(_secret_of(g10)) == 6
    r = m.search([1, 2, 3, 4], 10, 0, 0, 395 * SEG, 399 * SEG)
    assert _kinds(m) == [2]
    assert r.status == FOUND and r.global_idx == g10 and list(r.secret) == e["secret"]


@pytest.mark.parametrize("name", [n for n in NAMES if n != "w1"])
def test_layout_walk_equals_the_list(forced, name):
    """N = 8, workerBits 0: the walked hits of the window (its first 16 segments) are the list, the
    secrets are the indices' and an exhausted search of it counts every candidate once."""
    c = CASES[name]
    k0, k1 = c["k_begin"], min(c["k_end"], c["k_begin"] + WALK_SEGS * SEG)
    n_launch = _n_chunk_lengths(k0, k1)
    assert n_launch == (2 if name in ("l56", "l67") else 1)
    kinds = []
    t = time.perf_counter()
    hits = _walk(forced, c["nonce"], NTZ, 0, 0, k0, k1, first_kinds=kinds)
    print(f"{name}: {len(hits)} hits walked in {time.perf_counter() - t:.2f} s, kinds {kinds}")
    # a search that finds its hit in the first of two launches may return before it queues the second
    assert kinds and kinds == [2] * len(kinds) and len(kinds) <= n_launch
    assert hits == _expected(c, k0=k0, k1=k1) and hits
    forced.reset_stats()
    r = forced.search(c["nonce"], 32, 0, 0, k0, k1)
    assert r.status == EXHAUSTED
    s = forced.stats()
    assert s.candidates == (k1 - k0) * 256 and s.launches == n_launch
    assert _kinds(forced) == [2] * n_launch


def _n9_after_8(hits):
    seen8 = False
    for _, tz in hits:
        if tz == 8:
            seen8 = True
        elif seen8 and tz >= 9:
            return True
    return False


def _n9_walked():
    """Per W0 the first case with an N = 9 entry behind a D == 0 false positive."""
    out = {}
    for n in NAMES:
        if _n9_after_8(CASES[n]["hits"]):
            out.setdefault((len(CASES[n]["nonce"]) % 64) // 4, n)
    return out


def test_every_w0_has_an_n9_walk():
    assert sorted(_n9_walked()) == [0, 1, 2, 3] and _n9_walked()[1] == "w1"


@pytest.mark.parametrize("name", NAMES)
def test_n9_rejects_the_d_equality_false_positives(forced, golden, name):
    """The N > 8 branch of hash_wave_block_si (full_check with the segment delta, then on to the
    next slot): an N = 9 search returns the first entry with tz >= 9, past every tz = 8 entry
    before it, or EXHAUSTED when the list has none."""
    c = CASES[name]
    exp = _expected(c, ntz=9)
    r = forced.search(c["nonce"], 9, 0, 0, c["k_begin"], c["k_end"])
    kinds = _kinds(forced)
    assert kinds and kinds == [2] * len(kinds) and len(kinds) <= _n_chunk_lengths(c["k_begin"], c["k_end"])
    if exp:
        assert r.status == FOUND and r.global_idx == exp[0] and r.secret == _secret_of(exp[0]), (r, exp)
    else:
        assert r.status == EXHAUSTED and len(kinds) == _n_chunk_lengths(c["k_begin"], c["k_end"]), r
    if name == "w1":
        e = next(x for x in golden["deep_hits"] if x["nonce"] == [1, 2, 3, 4] and x["ntz"] == 9)
        assert r.global_idx == e["global_idx"] and list(r.secret) == e["secret"]
    if name in _n9_walked().values():
        assert _walk(forced, c["nonce"], 9, 0, 0, c["k_begin"], c["k_end"]) == exp


@pytest.mark.parametrize("wb", range(8))
def test_partitions_of_8_from_one_list(forced, wb):
    c = CASES["w1"]
    kinds = []
    hits = _walk(forced, c["nonce"], NTZ, wb, 3, c["k_begin"], c["k_end"], first_kinds=kinds)
    assert kinds == [2]
    assert hits == _expected(c, wb=wb, wbits=3)
    assert all((g & 0xFF) >> 5 == wb for g in hits)


def test_partitions_of_256_from_one_list(forced):
    """workerBits 8 (one thread byte per worker), the thread bytes of 6 entries spread over the window."""
    c = CASES["w1"]
    n = len(c["hits"])
    for i in range(6):
        tb = c["hits"][i * (n - 1) // 5][0] & 0xFF
        kinds = []
        hits = _walk(forced, c["nonce"], NTZ, tb, 8, c["k_begin"], c["k_end"], first_kinds=kinds)
        assert kinds == [2]
        assert hits == _expected(c, wb=tb, wbits=8) and hits, (tb, hits)


@pytest.mark.parametrize("wb,wbits,segs", [(3, 9, 8), (1, 10, WALK_SEGS), (2, 10, WALK_SEGS)])
def test_quirk_partitions_from_one_list(forced, wb, wbits, segs):
    """workerBits % 9 (worker.go:302): 9 is every thread byte, 10 is halves, worker_byte 2 wrapping
    to the lower one.  The first hit over the whole window, the walk over its first segments."""
    c = CASES["w1"]
    assert _thread_bytes(3, 9) == list(range(256)) and _thread_bytes(2, 10) == list(range(128))
    assert _thread_bytes(1, 10) == list(range(128, 256))
    exp = _expected(c, wb=wb, wbits=wbits)
    r = forced.search(c["nonce"], NTZ, wb, wbits, c["k_begin"], c["k_end"])
    assert _kinds(forced) == [2]
    assert r.status == FOUND and r.global_idx == exp[0] and r.secret == _secret_of(exp[0])
    k1 = c["k_begin"] + segs * SEG
    assert _walk(forced, c["nonce"], NTZ, wb, wbits, c["k_begin"], k1) == _expected(c, wb=wb, wbits=wbits, k1=k1)


def test_first_hit_of_the_whole_window(forced):
    c = CASES["w1"]
    r = forced.search(c["nonce"], NTZ, 0, 0, c["k_begin"], c["k_end"])
    assert _kinds(forced) == [2]
    g = c["hits"][0][0]
    assert r.status == FOUND and r.global_idx == g and r.secret == _secret_of(g)


# ---- bounds that land while the launch runs (the `lower` branch of the kernel's poll) ----

def _bound_choices(wbits):
    """4 x (worker_byte, window start k, h): h is the partition's first hit of [start, k_end), in a
    later segment than start, with at least 3 segments of window; start is behind the partition's
    previous hit (the window's begin for its first)."""
    c = CASES["w1"]
    out = []
    for wb in range(1 << wbits):
        if wbits and wb == 0:
            continue  # partitions with base_tb > 0: a bound below the first thread byte exists
        hs = _expected(c, wb=wb, wbits=wbits)
        for j, h in enumerate(hs):
            start = (hs[j - 1] >> 8) + 1 if j else c["k_begin"]
            if (h >> 8) // SEG > start // SEG and c["k_end"] - start >= 3 * SEG:
                out.append((wb, start, h))
    assert len(out) >= 4, out
    return [out[i * (len(out) - 1) // 3] for i in range(4)]


@pytest.fixture(scope="module")
def board():
    from distpow.node import NodeBoard
    b = NodeBoard.local()
    yield b
    b.close()


def _search_with_node_post(m, board, args, post, delay_ns):
    """-> (result, scheduled post time, decided time).  The post lands on the attached slot at
    t_post from the library's poster thread (dpow_diag_node_post_at)."""
    L = distpow.lib()
    slot = board.begin()
    L.dpow_node_slot_reset(slot)
    m.attach_node(slot)
    try:
        t_post = time.perf_counter_ns() + delay_ns
        L.dpow_diag_node_post_at(slot, post, t_post)
        r = m.search(*args)
        t_dec = _decided_ns(m)
        while board.best(slot) > post:  # a post timed behind the search's end: before the slot's reuse
            assert time.perf_counter_ns() < t_post + 2_000_000_000
    finally:
        m.attach_node(None)
        board.end()
    return r, t_post, t_dec


def _search_with_thread_bound(m, args, post, delay_ns):
    """-> (result, search call's begin, bound call's begin, bound call's end, decided time)."""
    out = {}

    def run():
        out["t_s0"] = time.perf_counter_ns()
        out["r"] = m.search(*args)

    th = threading.Thread(target=run)
    t_start = time.perf_counter_ns()
    th.start()
    left = t_start + delay_ns - time.perf_counter_ns()
    if left > 0:
        time.sleep(left * 1e-9)
    t_b0 = time.perf_counter_ns()
    m.bound(post)
    t_b1 = time.perf_counter_ns()
    th.join(timeout=30)
    assert not th.is_alive()
    return out["r"], out["t_s0"], t_b0, t_b1, _decided_ns(m)


@pytest.mark.parametrize("path", ["node", "thread"])
@pytest.mark.parametrize("wbits,ji", [(wbits, ji) for wbits in (0, 3) for ji in range(4)])
def test_bound_lowered_while_the_launch_runs(forced, board, wbits, ji, path):
    """A bound P that arrives at a random moment of a segment-inner launch whose first hit is h
    (through an attached node slot, or dpow_search_bound from another thread).

    P above h -- h + 1, below the partition's first thread byte of the next k, the next k, h + a
    random distance -- must give FOUND h whenever it lands: the launch is trimmed to P's segment
    (seg_limit_of) and must not lose h.

    The delay is uniform over the window's launch time (a plain ntz = 32 search of it) and, a
    second time, over the time of the search that finds h.

    P = h and P below h give EXHAUSTED when P is in place before the search decides, as
    test_search_returns_at_covered_bound_vs_oracle asserts for a bound posted before the start.
    search.cpp allows these other outcomes, and no more:
      - the post lands after consume()'s last look (poll_node at its top, the ext_bound load
        beside `sn.best >= eb`): FOUND h.  Observable: the post's time against the decided time
        (dpow_diag_search_times[3]); within kMarginNs (1 ms, 5 ms for the poster thread's
        scheduled time) before it either outcome is legal.
      - dpow_search_bound before the search opened its window (Search::open_bound_window in search_window: "no
        search in flight") applies to nothing: FOUND h.  Required when the call ended before the
        search call began; either outcome until the first md5 launch was queued.
      - P = h through the node slot: h is a hit of this partition, so when the watcher relays it to
        the early-hit word before the host polls the slot, poll_early verifies it, marks it as its
        own post (own_posted) and poll_node then does not take it for a bound: FOUND h.  Both
        outcomes are legal whenever it lands; through dpow_search_bound only EXHAUSTED is.
    After each, a small search on the same context still answers (stale mark, control ring)."""
    # the thread path times the bound call itself; the node path only knows the time the poster
    # thread was asked to post at, and that thread may wake late
    kMarginNs = 1_000_000 if path == "thread" else 5_000_000
    c = CASES["w1"]
    wb, start, h = _bound_choices(wbits)[ji]
    args = (c["nonce"], NTZ, wb, wbits, start, c["k_end"])
    assert _expected(c, wb=wb, wbits=wbits, k0=start)[0] == h
    t = time.perf_counter_ns()
    assert forced.search(c["nonce"], 32, wb, wbits, start, c["k_end"]).status == EXHAUSTED
    t_launch = time.perf_counter_ns() - t
    assert _kinds(forced) == [2]
    # The search that finds h returns sooner (its launch is trimmed to h's segment), so many posts
    # of that range land behind its end; a second delay per P is drawn from that search's own time.
    t = time.perf_counter_ns()
    r = forced.search(*args)
    t_found = time.perf_counter_ns() - t
    assert r.status == FOUND and r.global_idx == h and _kinds(forced) == [2]
    rnd = random.Random(f"{wbits}/{ji}/{path}")
    base_tb = _thread_bytes(wb, wbits)[0]
    above = [h + 1, ((h >> 8) + 1) << 8, h + rnd.randrange(1, 1 << 20)]
    if base_tb > 0:
        above.append(((h >> 8) + 1) << 8 | (base_tb - 1))
    below = [h, h - rnd.randrange(1, 1 << 16)]
    assert all(p > start << 8 for p in below)
    for post, span in [(p, t) for p in above + below for t in (t_launch, t_found)]:
        delay = rnd.randrange(0, span + 1)
        if path == "node":
            r, t_post, t_dec = _search_with_node_post(forced, board, args, post, delay)
            early, late, either = t_post < t_dec - kMarginNs, t_post > t_dec, post == h
        else:
            r, t_s0, t_b0, t_b1, t_dec = _search_with_thread_bound(forced, args, post, delay)
            t_open = _launches(forced)[1][0].queued_ns
            early, late, either = t_b0 > t_open and t_b1 < t_dec - kMarginNs, t_b1 < t_s0 or t_b0 > t_dec, False
        assert _kinds(forced) == [2]
        got = (r.status, r.global_idx if r.status == FOUND else None)
        print(f"wbits {wbits} P - h = {post - h}: delay {delay / 1e6:.2f} of {span / 1e6:.2f} ms, "
              f"{'early' if early else 'late' if late else 'edge'} -> {got}")
        if post > h or (late and not either):
            assert got == (FOUND, h), (post, h, got)
        elif early and not either:
            assert got == (EXHAUSTED, None), (post, h, got)
        else:
            assert got in ((FOUND, h), (EXHAUSTED, None)), (post, h, got)
        if r.status == FOUND:
            assert r.secret == _secret_of(h)
        r3 = forced.search([1, 2, 3, 4], 3, 0, 0, 0, 1 << 10)
        assert r3.status == FOUND and r3.global_idx == 97
