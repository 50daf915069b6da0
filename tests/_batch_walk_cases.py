"""Case families and the batched walk that pin the generic kernel of the batched search
(csrc/md5_batch.hip) -- shared by tests/test_batch_walk_cases.py (CPU: the families are what they
claim, from hashlib, the C oracle and the round planner alone) and tests/test_gpu_batch_walk.py.
The depth reference and families F and G at the end serve the scan and census kernels as well
(tests/test_listing_walk_cases.py on the CPU, tests/test_gpu_listing_walk.py on the GPU).

Every expected value here comes from hashlib, the oracle or a committed fixture; nothing calls
search_batch or search to learn an answer.  The builders are deterministic (SEED) and cached, so
a process computes each family once.

Notation: edge(a) = 256**a is the first k whose chunk is a + 1 bytes long; R = 256 >> worker_bits
is the number of thread bytes per k; p = nonce_len % 64 is the byte the thread byte goes to; a
candidate needs a second final block when p + 1 + L > 55.
"""
import functools
import hashlib
import json
import os
import random
from dataclasses import dataclass, field, replace
from typing import List, Optional

import distpow
from distpow import DPOW_NO_HIT, EXHAUSTED, FOUND, BatchTask
from distpow._lib import DPOW_BATCH_MAX, DPOW_K_LIMIT

SEED = 20240611
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NO_HIT = (EXHAUSTED, DPOW_NO_HIT, None)


def edge(a):
    return 256 ** a


def secret_of(g):
    """threadByte || the minimal little-endian bytes of k, for the global index g = k * 256 + threadByte."""
    out, k = [g & 0xFF], g >> 8
    while k:
        out.append(k & 0xFF)
        k >>= 8
    return bytes(out)


def tz_of(nonce, g):
    h = hashlib.md5(bytes(nonce) + secret_of(g)).hexdigest()
    return len(h) - len(h.rstrip("0"))


def thread_bytes(wb, wbits):
    """worker.go:302-316, in increasing order."""
    rbits = 8 - wbits % 9
    return [((wb << rbits) | i) & 0xFF for i in range(1 << rbits)]


def window_hits(nonce, ntz, wb, wbits, k0, k1, with_tz=False):
    """Every hit of a window in index order, by hashlib alone."""
    base, zeros, out = hashlib.md5(bytes(nonce)), "0" * ntz, []
    tbs = thread_bytes(wb, wbits)
    for k in range(k0, k1):
        chunk = secret_of(k << 8)[1:]
        for tb in tbs:
            h = base.copy()
            h.update(bytes([tb]) + chunk)
            x = h.hexdigest()
            if x.endswith(zeros):
                out.append([k << 8 | tb, len(x) - len(x.rstrip("0"))] if with_tz else k << 8 | tb)
    return out


def got(res):
    return (res.status, res.global_idx, res.secret)


def found(g):
    return (FOUND, g, secret_of(g))


def walk_batch(search_batch, tasks, ntz):
    """Every hit of every task's window in index order: search_batch over the tasks still live,
    each FOUND task resuming at the k behind its hit with the same k_end, each EXHAUSTED task
    dropping out.  The later thread bytes of a hit's k are hashed with hashlib (at worker_bits 8 a k
    is one candidate, so there the GPU decides every candidate).  -> one hit list per task."""
    hits = [[] for _ in tasks]
    cur = [t.k_begin for t in tasks]
    live = [i for i, t in enumerate(tasks) if t.k_begin < t.k_end]
    assert all(t.num_trailing_zeros == ntz for t in tasks)
    while live:
        batch = [replace(tasks[i], k_begin=cur[i]) for i in live]
        res = []
        for off in range(0, len(batch), DPOW_BATCH_MAX):
            res += search_batch(batch[off:off + DPOW_BATCH_MAX])
        assert len(res) == len(batch)
        nxt = []
        for i, r in zip(live, res):
            t = tasks[i]
            if r.status != FOUND:
                assert got(r) == NO_HIT, (i, t, r)
                continue
            g = r.global_idx
            assert r.secret == secret_of(g) == distpow.secret_from_index(g), (i, t, r)
            assert cur[i] <= g >> 8 < t.k_end, (i, t, r)       # inside what was asked: the walk advances
            hits[i].append(g)
            hits[i] += [(g >> 8) << 8 | tb for tb in thread_bytes(t.worker_byte, t.worker_bits)
                        if tb > (g & 0xFF) and tz_of(t.nonce, (g >> 8) << 8 | tb) >= ntz]
            cur[i] = (g >> 8) + 1
            if cur[i] < t.k_end:
                nxt.append(i)
        live = nxt
    return hits


def oracle_search_batch(oracle):
    """search_batch built on the C oracle alone: drives walk_batch on the CPU."""
    def search_batch(tasks):
        out = []
        for t in tasks:
            r = oracle.mine_window(list(t.nonce), t.num_trailing_zeros, t.worker_byte, t.worker_bits,
                                   t.k_begin, t.k_end)
            hit = r is not None and r[1] < t.bound
            out.append(distpow.SearchResult(FOUND, r[1], bytes(r[0])) if hit else distpow.SearchResult(EXHAUSTED))
        return out
    return search_batch


class Counted:
    """search_batch of a Miner, counting the calls."""

    def __init__(self, miner):
        self.miner, self.calls = miner, 0

    def __call__(self, tasks):
        self.calls += 1
        return self.miner.search_batch(tasks)


def _nonce(rnd, n):
    return bytes(rnd.randrange(256) for _ in range(n))


# ---- family A and the controls of family B: the block count changes inside a wave --------------
@dataclass
class EdgeCase:
    """A window over the chunk-length change at `edge`, with every hit of it by hashlib."""
    task: BatchTask
    a: int               # edge = 256**a (7: the top of the k range)
    edge: int
    p: int
    d: int = 0           # family A: k_begin = max(edge - d, 0)
    hits: List[int] = field(default_factory=list)

    @property
    def wbits(self):
        return self.task.worker_bits


def _wave_cases(rnd, p_of_a):
    """For p = p_of_a(a) and nonce lengths p, p + 64: windows of two 64-index waves whose first
    wave has the edge at its k position d (d = per: the first k of the second wave)."""
    out = []
    for a in range(7):
        for nl in (p_of_a(a), p_of_a(a) + 64):
            for wbits in range(3, 9):
                per = 64 >> (8 - wbits)          # k per 64-lane wave
                for d in range(1, per + 1):
                    kb = max(edge(a) - d, 0)
                    t = BatchTask(_nonce(rnd, nl), 1, rnd.randrange(1 << wbits), wbits, kb, kb + 2 * per)
                    out.append(EdgeCase(t, a, edge(a), nl % 64, d))
    return out


def _fill_hits(cases):
    for c in cases:
        t = c.task
        c.hits = window_hits(t.nonce, t.num_trailing_zeros, t.worker_byte, t.worker_bits, t.k_begin, t.k_end)
    return cases


@functools.lru_cache(maxsize=None)
def family_a():
    """N = 1, p = 54 - a: one block below edge(a), two at it.  1764 tasks of 128 candidates."""
    return _fill_hits(_wave_cases(random.Random(SEED), lambda a: 54 - a))


# ---- family B: every byte position at every chunk-length change, R = 1 --------------------------
TOP = 7   # the eighth "edge": the top of the k range, k_end = DPOW_K_LIMIT


@functools.lru_cache(maxsize=None)
def family_b():
    """N = 1, worker_bits 8 (a k is one candidate): p = 0..63 with nonce lengths p, p + 64, p + 128
    on 64-k windows centred on each edge(a), and on the last 64 k below DPOW_K_LIMIT.  The worker
    byte is random, except that below edge(0) there is one candidate only, k = 0 (the one candidate
    with an empty chunk): at nonce lengths p and p + 128 the worker byte is the lowest whose k = 0
    candidate is a hit by hashlib, so that these windows have a hit on both sides of the edge too."""
    rnd = random.Random(SEED + 1)
    out = []
    for a in range(8):
        for p in range(64):
            for nl in (p, p + 64, p + 128):
                kb = DPOW_K_LIMIT - 64 if a == TOP else max(edge(a) - 32, 0)
                nonce, wb = _nonce(rnd, nl), rnd.randrange(256)
                if a == 0 and nl != p + 64:
                    wb = next((b for b in range(256) if tz_of(nonce, b) >= 1), wb)
                e = DPOW_K_LIMIT if a == TOP else edge(a)
                out.append(EdgeCase(BatchTask(nonce, 1, wb, 8, kb, kb + 64), a, e, p))
    return _fill_hits(out)


@functools.lru_cache(maxsize=None)
def family_b_controls():
    """Family A's shape at worker_bits 3 with the neighbouring p: {"never": p = 53 - a, no candidate
    of the window needs a second block; "always": p = 55 - a, every one does}."""
    rnd = random.Random(SEED + 2)
    return {name: _fill_hits([c for c in _wave_cases(rnd, p_of_a) if c.wbits == 3])
            for name, p_of_a in (("never", lambda a: 53 - a), ("always", lambda a: 55 - a))}


# ---- family C: the deep hits of every layout ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def deep_cases():
    """The cases of layout_deep_hits.json (each lists every N >= 8 hit of its window with its
    trailing-zero count), and one 16-k case round each deep hit of pow_golden.json whose list is
    hashlib's scan of those 16 k."""
    with open(os.path.join(GOLDEN_DIR, "layout_deep_hits.json")) as f:
        cases = [dict(c, source="layout") for c in json.load(f)["cases"]]
    with open(os.path.join(GOLDEN_DIR, "pow_golden.json")) as f:
        deep = json.load(f)["deep_hits"]
    for n, h in enumerate(deep):
        k = h["global_idx"] >> 8
        hits = window_hits(h["nonce"], 8, 0, 0, k - 8, k + 8, with_tz=True)
        assert [g for g, _ in hits] == [h["global_idx"]] and hits[0][1] >= h["ntz"], (h, hits)
        cases.append({"name": f"golden{n}", "nonce": h["nonce"], "k_begin": k - 8, "k_end": k + 8, "nblk": 1,
                      "hits": hits, "source": "golden"})
    return cases


@dataclass
class DeepTask:
    task: BatchTask
    expected: tuple      # got() of the result
    case: str
    nblk: int
    kind: str            # "n8", "n9" or "next" (N = tz + 1 on the hit's own k)
    g: int               # the listed hit the task was built round
    tz: int


def _first_listed(c, ntz, tbs, k0, k1):
    """The lowest listed hit of case c with tz >= ntz in [k0, k1) and the partition: what a search
    returns (the list holds every N >= 8 hit of the case's window)."""
    assert ntz >= 8 and c["k_begin"] <= k0 and k1 <= c["k_end"]
    for g, tz in c["hits"]:
        if tz >= ntz and k0 <= g >> 8 < k1 and (g & 0xFF) in tbs:
            return found(g)
    return NO_HIT


@functools.lru_cache(maxsize=None)
def family_c():
    """Per listed hit (g, tz), at worker_bits 0, 3 and 8 in the hit's own partition: N = 8 and
    N = 9 on [k - 8, k + 8) clipped to the case's window, and N = tz + 1 on [k, k + 1)."""
    out = []
    for c in deep_cases():
        nonce = bytes(c["nonce"])
        for g, tz in c["hits"]:
            k = g >> 8
            k0, k1 = max(k - 8, c["k_begin"]), min(k + 8, c["k_end"])
            for wbits in (0, 3, 8):
                wb = (g & 0xFF) >> (8 - wbits)
                tbs = set(thread_bytes(wb, wbits))
                assert (g & 0xFF) in tbs
                for kind, ntz, w0, w1 in (("n8", 8, k0, k1), ("n9", 9, k0, k1), ("next", tz + 1, k, k + 1)):
                    out.append(DeepTask(BatchTask(nonce, ntz, wb, wbits, w0, w1), _first_listed(c, ntz, tbs, w0, w1),
                                        c["name"], c["nblk"], kind, g, tz))
    return out


# ---- family D: all rows of round 0 on one task, dense hits --------------------------------------
D_NONCE_LENGTHS = [1, 4, 11, 53, 54, 55, 63, 64, 118, 190]
D_SPAN = 4096   # k: 2^20 candidates at worker_bits 0, the whole of round 0 for a lone task


@functools.lru_cache(maxsize=None)
def family_d():
    """{(B, N): 8 batches of B tasks}: 4096-k windows at worker_bits 0, fresh nonces every batch."""
    rnd = random.Random(SEED + 3)
    out = {}
    for b in (1, 2, 3):
        for ntz in (1, 2):
            out[b, ntz] = [[BatchTask(_nonce(rnd, rnd.choice(D_NONCE_LENGTHS)), ntz, 0, 0, kb, kb + D_SPAN)
                            for kb in (rnd.choice([0, edge(2) - 1000, rnd.randrange(1 << 40)]) for _ in range(b))]
                           for _ in range(8)]
    return out


# ---- family E: a hit on each seam ---------------------------------------------------------------
E_BATCH = 64          # tasks per batch: the probe and 63 fillers
E_PROBE = 17          # the probe's place in the batch
E_NTZ = 4
E_WINDOW = 1 << 15    # local indices of the probe's window: two slices of round 0
E_K0 = 70000          # reference hits are taken from k >= E_K0 + the window
SEAMS = ("group-1", "group", "slice-1", "slice", "last")


@dataclass
class SeamCase:
    seam: str
    wbits: int
    batch: List[BatchTask]
    hit: int             # the probe's answer: a reference hit, nothing before it in the window
    offset: int          # its local offset from the probe's i_begin
    slice: int           # round 0's slice and group for this batch (distpow.batch_plan)
    group: int
    expected: Optional[list] = None   # got() per task, by the oracle

    @property
    def probe(self):
        return self.batch[E_PROBE]


def round0_of(batch):
    """(slice, group) of round 0 for the probe of a family-E batch, from the round planner."""
    entries, _ = distpow.batch_plan([(t.k_begin, t.k_end, t.worker_bits) for t in batch])
    first = [e for e in entries if e.launch == 0]
    assert len(first) == len(batch) and first[E_PROBE].task == E_PROBE
    e = first[E_PROBE]
    return e.i_end - e.i_begin, e.group


def oracle_expect(oracle, t):
    r = oracle.mine_window(list(t.nonce), t.num_trailing_zeros, t.worker_byte, t.worker_bits, t.k_begin, t.k_end)
    return NO_HIT if r is None or r[1] >= t.bound else (FOUND, r[1], bytes(r[0]))


def family_e(oracle, wbits):
    """One batch per seam: a probe task (N = 4, E_WINDOW local indices) whose only hit up to its
    answer lies at local offset group - 1, group, slice - 1, slice and on the window's last k
    (at R = 256 the offset is rounded to the k on that side of the seam), among 63 fixed 4-k
    fillers that keep round 0's plan the one that was read."""
    if wbits in _family_e:
        return _family_e[wbits]
    rnd = random.Random(SEED + 4 + wbits)
    rbits = 8 - wbits
    R = 1 << rbits
    nonce, wb = _nonce(rnd, 11), rnd.randrange(1 << wbits)
    fillers = [BatchTask(_nonce(rnd, 4), 2, 0, 0, kb, kb + 4)
               for kb in (rnd.randrange(1 << 20) for _ in range(E_BATCH - 1))]

    def batch_for(kb):
        b = list(fillers)
        b.insert(E_PROBE, BatchTask(nonce, E_NTZ, wb, wbits, kb, kb + E_WINDOW // R))
        return b

    s, grp = round0_of(batch_for(E_K0))
    assert R <= grp < s < E_WINDOW and grp % R == 0
    targets = {"group-1": grp - 1, "group": grp, "slice-1": s - 1, "slice": s, "last": E_WINDOW - 1}
    out, k, tries = {}, E_K0 + E_WINDOW // R, 0
    while len(out) < len(SEAMS):
        tries += 1
        assert tries <= 200, "no reference hit with a hit-free prefix found"
        r = oracle.mine_window(list(nonce), E_NTZ, wb, wbits, k, DPOW_K_LIMIT)   # the next reference hit
        g = r[1]
        k, t = (g >> 8) + 1, g & (R - 1)
        for seam in SEAMS:
            if seam in out:
                continue
            # whole k between the window's begin and the hit: below the seam rounds down, at it up
            m = (targets[seam] - t) // R if seam.endswith("-1") or seam == "last" else -((t - targets[seam]) // R)
            kb = (g >> 8) - m
            probe = BatchTask(nonce, E_NTZ, wb, wbits, kb, kb + E_WINDOW // R)
            if oracle_expect(oracle, probe) != found(g):
                continue     # another hit lies before it: try the next reference hit for this seam
            batch = batch_for(kb)
            assert round0_of(batch) == (s, grp)
            out[seam] = SeamCase(seam, wbits, batch, g, m * R + t, s, grp, [oracle_expect(oracle, b) for b in batch])
            break
    _family_e[wbits] = [out[seam] for seam in SEAMS]
    return _family_e[wbits]


_family_e = {}


# ---- the depth reference: every candidate of a window with its depth ----------------------------
# The scan and the census (Miner.scan, scan_many, census, census_many) answer for a whole window in
# one call, so tests/test_gpu_listing_walk.py compares them with these lists directly, no walk.
D = 33   # depths 0..32 (DPOW_CENSUS_DEPTHS)


@functools.lru_cache(maxsize=None)
def window_depths(nonce, wb, wbits, k0, k1):
    """((global index, depth), ...) of every candidate of a window in the reference's order (k
    outer, thread byte inner), by hashlib alone; a candidate's depth is the number of trailing '0'
    characters of its digest.  Cached per window."""
    base, out = hashlib.md5(nonce), []
    tbs = thread_bytes(wb, wbits)
    for k in range(k0, k1):
        chunk = secret_of(k << 8)[1:]
        for tb in tbs:
            h = base.copy()
            h.update(bytes([tb]) + chunk)
            x = h.hexdigest()
            out.append((k << 8 | tb, len(x) - len(x.rstrip("0"))))
    return tuple(out)


def depths_of(c):
    """window_depths of a case (EdgeCase) or a task."""
    t = getattr(c, "task", c)
    return window_depths(bytes(t.nonce), t.worker_byte, t.worker_bits, t.k_begin, t.k_end)


def scan_hits_of(c, ntz):
    """What Miner.scan returns for the case's window at N = ntz, from the depth reference."""
    return [distpow.ScanHit(g, tz, secret_of(g)) for g, tz in depths_of(c) if tz >= ntz]


def census_of(c):
    """What Miner.census returns for the case's window, from the depth reference."""
    count, first, tz = [0] * D, [None] * D, [0] * D
    for g, t in depths_of(c):
        for d in range(t + 1):
            count[d] += 1
            if first[d] is None:
                first[d], tz[d] = g, t
    return distpow.Census(tuple(count), tuple(first), tuple(tz), max((d for d in range(D) if count[d]), default=0))


# ---- family F: wide partitions (worker_bits 0..2) at every edge and at the top -------------------
F_WBITS = (0, 1, 2)
F_SEED = SEED + 21   # (change the offset, not a threshold, if tests/test_listing_walk_cases.py's conditions fail)


def f_positions(a):
    """The p of family F at edge a: the block-count change itself, then one block for every chunk
    length, the last one-block word, and two blocks for every chunk length.  At the top (chunks of
    7 bytes) p = 54 - 7 = 47 is in the list already; p = 48 is the first that needs two blocks."""
    return (48 if a == TOP else 54 - a, 0, 47, 55, 63)


@functools.lru_cache(maxsize=None)
def family_f():
    """N = 1, worker_bits 0, 1 and 2 (256, 128 and 64 candidates per k): for every a = 0..7 and p of
    f_positions(a), nonce lengths p and p + 64 on [max(edge(a) - 2, 0), edge(a) + 2), and on the
    last three k below DPOW_K_LIMIT at the top.  240 tasks of at most 1024 candidates; at
    worker_bits 0 the top windows end at local index 2^63 - 1."""
    rnd = random.Random(F_SEED)
    out = []
    for a in range(8):
        for wbits in F_WBITS:
            for p in f_positions(a):
                for nl in (p, p + 64):
                    e = DPOW_K_LIMIT if a == TOP else edge(a)
                    kb, ke = (DPOW_K_LIMIT - 3, DPOW_K_LIMIT) if a == TOP else (max(e - 2, 0), e + 2)
                    t = BatchTask(_nonce(rnd, nl), 1, rnd.randrange(1 << wbits), wbits, kb, ke)
                    out.append(EdgeCase(t, a, e, p))
    return _fill_hits(out)


# ---- family G: a partial wave whose clamped lanes need the second block --------------------------
G_WBITS = (4, 5, 6, 7, 8)
G_SEED = SEED + 22


def _partial_wave_cases(rnd, with_edge):
    """p = 54 - a, nonce lengths p and p + 64, worker_bits 4..8: [edge - d, edge + 1) (with_edge) or
    [edge - d, edge) for d = 1..per - 2, per the k of a 64-lane wave; below edge(0) = 1 there is
    k = 0 only, so there d = 1."""
    out = []
    for a in range(7):
        for nl in (54 - a, 54 - a + 64):
            for wbits in G_WBITS:
                per = 64 >> (8 - wbits)
                for d in range(1, 2 if a == 0 else per - 1):
                    t = BatchTask(_nonce(rnd, nl), 1, rnd.randrange(1 << wbits), wbits, edge(a) - d,
                                  edge(a) + (1 if with_edge else 0))
                    out.append(EdgeCase(t, a, edge(a), nl % 64, d))
    return out


@functools.lru_cache(maxsize=None)
def family_g():
    """N = 1: windows of fewer than 64 local indices that end with the first two-block k, edge(a).
    A kernel hashes such a window in one partial wave from the window's begin: its lanes below the
    edge need one block, the lanes of the edge's k two, and so do the inactive lanes, which are
    clamped to the window's last index.  1378 tasks."""
    return _fill_hits(_partial_wave_cases(random.Random(G_SEED), True))


@functools.lru_cache(maxsize=None)
def family_g_controls():
    """Family G's windows without the edge's k: no lane, clamped or not, needs two blocks."""
    return _fill_hits(_partial_wave_cases(random.Random(G_SEED + 1), False))
