"""Case families and the batched walk that pin the generic kernel of the batched search
(csrc/md5_batch.hip) -- shared by tests/test_batch_walk_cases.py (CPU: the families are what they
claim, from hashlib, the C oracle and the round planner alone) and tests/test_gpu_batch_walk.py.
The depth reference and families F and G at the end serve the scan and census kernels as well
(tests/test_listing_walk_cases.py on the CPU, tests/test_gpu_listing_walk.py on the GPU), and the
device scan (tests/test_gpu_scan_dev_walk.py), whose geometry is restated behind them with family H,
the windows that reach every group size of it, and the batched device scan
(tests/test_gpu_scan_many_dev_walk.py) with families M and X, the calls of many tasks that reach every
group size and every prefix round of it (tests/test_scan_many_dev_walk_cases.py on the CPU).

Every expected value here comes from hashlib, the oracle or a committed fixture; nothing calls
search_batch or search to learn an answer (families H, M and X hold no hashes: their windows are too
long for hashlib, and window_depths_cuda takes their depths from the digest kernel).  The builders are
deterministic (SEED) and cached, so a process computes each family once.

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


# ---- the device scan's geometry, restated (csrc/scan_dev.cpp, batch.cpp batch_group) --------------
# dpow_scan_device takes a window up in slices of SCAN_DEV_SLICE local indices from its begin; a slice
# of `total` indices runs in workgroups of clamp(pow2_floor(total / SCAN_DEV_BLOCKS), SCAN_DEV_MIN_GROUP,
# SCAN_DEV_MAX_GROUP) indices, the last one short.  tests/test_listing_walk_cases.py pins the four
# constants to the sources; tests/test_gpu_scan_dev_walk.py pins the rule to the library's behaviour.
SCAN_DEV_BLOCKS = 4096            # csrc/batch.h kBatchBlocks
SCAN_DEV_MIN_GROUP = 256          # csrc/batch.h kBatchMinGroup
SCAN_DEV_MAX_GROUP = 16384        # csrc/batch.h kBatchMaxGroup = csrc/md5_scan_dev.h kScanDevMaxGroup
SCAN_DEV_SLICE = 1 << 28          # csrc/md5_scan_dev.h kScanDevSlice
SCAN_DEV_STEP = 256               # local indices per workgroup step: four waves of 64 lanes
SCAN_DEV_PREFIX_ROUND = 2048      # totals per round of the last workgroup's prefix: 8 per thread


def scan_dev_geometry(total):
    """(group, n_blocks) of a slice of `total` > 0 local indices."""
    q = total // SCAN_DEV_BLOCKS
    group = min(max(1 << (q.bit_length() - 1) if q else 0, SCAN_DEV_MIN_GROUP), SCAN_DEV_MAX_GROUP)
    return group, -(-total // group)


def scan_dev_slices(i_begin, i_end):
    """[(lo, hi, group, n_blocks)] of the slices a call over the local indices [i_begin, i_end) runs."""
    out, lo = [], i_begin
    while lo < i_end:
        hi = min(lo + SCAN_DEV_SLICE, i_end)
        out.append((lo, hi) + scan_dev_geometry(hi - lo))
        lo = hi
    return out


def scan_dev_wave_steps(n):
    """[(steps, active lanes of the last step)] of the four waves of a workgroup whose range holds n
    local indices: wave w's step s starts at offset 64 w + 256 s and runs when that is below n."""
    out = []
    for w in range(4):
        first = 64 * w
        steps = -(-(n - first) // SCAN_DEV_STEP) if first < n else 0
        out.append((steps, min(n - first - SCAN_DEV_STEP * (steps - 1), 64) if steps else 0))
    return out


# ---- family H: every group size of the device scan, ragged across steps ---------------------------
# No hashes: tests/test_gpu_scan_dev_walk.py takes the lists from the digest kernel (window_depths_cuda).
H_SEED = SEED + 31
H_WBITS, H_WB = 3, 5              # R = 32 candidates per k
H_GROUPS = (512, 1024, 2048, 4096, 8192, 16384)


@dataclass(frozen=True)
class ScanWindow:
    """A window of the device scan with the geometry it was built for."""
    name: str
    nonce: bytes
    wb: int
    wbits: int
    k_begin: int
    k_end: int
    group: int           # of its one slice
    n_blocks: int
    s: int               # whole steps of the last group, before its ragged one (0: see the name)

    @property
    def rbits(self):
        return 8 - self.wbits

    @property
    def total(self):
        return (self.k_end - self.k_begin) << self.rbits


def _scan_window(name, rnd, nonce, wb, wbits, total, group, n_blocks, s):
    rbits = 8 - wbits
    assert total % (1 << rbits) == 0
    kb = rnd.randrange(1 << 16, 1 << 20) | 1          # odd: no multiple of group / R
    return ScanWindow(name, nonce, wb, wbits, kb, kb + (total >> rbits), group, n_blocks, s)


@functools.lru_cache(maxsize=None)
def family_h():
    """worker_bits 3 (R = 32), one worker byte, one 4-byte nonce: for each group g of H_GROUPS a window
    of 4096 g + 256 s + 96 local indices (s = 1 for g = 512, else g / 512) -- 4097 workgroups, three
    rounds of the prefix, a last group whose waves 0 and 1 run s + 1 steps, wave 1's last step half
    full, and waves 2 and 3 run s; three windows at group 256 of 2047, 2048 and 2048.375 groups (one
    round of the prefix not full, full, and a second round of one ragged group); and one window at
    worker_bits 0 (R = 256, so no half wave: its last group is three whole steps of the four) with a
    56-byte nonce, two final blocks, at group 1024; and one of 6145 groups of 512, four rounds of the
    prefix, the last group ragged like g512's.  Every k_begin is odd."""
    rnd = random.Random(H_SEED)
    nonce = _nonce(rnd, 4)
    out = []
    for g in H_GROUPS:
        s = 1 if g == 512 else g // 512
        out.append(_scan_window(f"g{g}", rnd, nonce, H_WB, H_WBITS, 4096 * g + 256 * s + 96, g, 4097, s))
    for name, total, n_blocks in (("b2047", 2047 * 256, 2047), ("b2048", 2048 * 256, 2048),
                                  ("b2049r", 2048 * 256 + 96, 2049)):
        out.append(_scan_window(name, rnd, nonce, H_WB, H_WBITS, total, 256, n_blocks, 0))
    out.append(_scan_window("g1024w0n56", rnd, _nonce(rnd, 56), 0, 0, 4096 * 1024 + 768, 1024, 4097, 3))
    # With 4097 workgroups the third round's carry reaches prefix[4096] alone, which no workgroup places
    # from (only a page cut reads it): 6145 groups of 512 put a whole round and a fourth behind it.
    out.append(_scan_window("g512b6145", rnd, nonce, H_WB, H_WBITS, 6144 * 512 + 256 + 96, 512, 6145, 1))
    return tuple(out)


def family_h_window(name):
    return next(w for w in family_h() if w.name == name)


@functools.lru_cache(maxsize=None)
def second_slice_window():
    """2^28 + 2^21 + 352 local indices at worker_bits 3: a whole slice at group 16384, then one of
    4097 groups of 512, the last of 352 indices (group, n_blocks and s are the second slice's)."""
    rnd = random.Random(H_SEED + 1)
    return _scan_window("two-slices", rnd, _nonce(rnd, 4), H_WB, H_WBITS, (1 << 28) + (1 << 21) + 352, 512, 4097, 1)


# ---- families M and X: the batched device scan, many tasks to a launch ------------------------------
# No hashes, like family H: tests/test_gpu_scan_many_dev_walk.py takes the lists from the digest kernel,
# Miner.scan_cuda and Miner.scan_many; tests/test_scan_many_dev_walk_cases.py shows through
# distpow.census_plan, the unit's planner, that the calls are what they name.  A call's launch holds all
# its tasks, and its descriptors are cut from each task's begin in pieces of the launch's group,
# scan_dev_geometry(the launch's total)[0].
M_SEED = SEED + 41   # (change the offset, not a threshold, if the walk's conditions fail: F_SEED's note)
X_SEED = SEED + 42
SCAN_MANY_MAX_BLOCKS = 20480      # csrc/md5_scan_many.h kScanManyMaxBlocks: ten rounds of the prefix
X_TASKS = 4096                    # DPOW_BATCH_MAX
X_LARGE_AT = 2047                 # the large task's place in family X's array


@dataclass(frozen=True)
class ScanCall:
    """One call of the batched device scan: its tasks as ScanWindows in array order (an empty task has
    k_begin == k_end), the group of its one launch and the length of each task's last descriptor."""
    name: str
    group: int
    windows: tuple
    lasts: tuple         # local indices of each task's last descriptor (0: an empty task)

    @property
    def total(self):
        return sum(w.total for w in self.windows)

    @property
    def n_descriptors(self):
        return sum(w.n_blocks for w in self.windows)

    def tasks(self, ntz):
        return [distpow.ScanTask(w.nonce, ntz, w.wb, w.wbits, w.k_begin, w.k_end) for w in self.windows]


def _call_window(name, rnd, nonce_len, wb, wbits, total, group):
    """A task of `total` local indices in a launch of `group`: its ScanWindow (s: the whole steps of its
    last descriptor before a ragged one) and the length of its last descriptor."""
    n_blocks = -(-total // group)
    last = total - (n_blocks - 1) * group if total else 0
    w = _scan_window(name, rnd, _nonce(rnd, nonce_len), wb, wbits, total, group, n_blocks,
                     last // SCAN_DEV_STEP if last % SCAN_DEV_STEP else 0)
    return w, last


def _scan_call(name, group, parts):
    return ScanCall(name, group, tuple(w for w, _ in parts), tuple(last for _, last in parts))


@functools.lru_cache(maxsize=None)
def family_m():
    """For each group g of H_GROUPS one call "m{g}" of five tasks with their own nonces, 4096 g + 256 s +
    673 local indices in all (s as family H: 1 for g = 512, else g / 512), so the launch's group is g:
      t0  worker_bits 3, 4-byte nonce, 1500 g + 256 s + 96 local indices: 1501 descriptors, the last ragged
          across steps like family H's (waves 0 and 1 run s + 1 steps, wave 1's last half full);
      t1  empty;
      t2  worker_bits 3, 55-byte nonce, 96 local indices: one descriptor shorter than a step, waves 2 and
          3 run none;
      t3  worker_bits 0, 56-byte nonce (two final blocks), 2000 g + 256: 2001 descriptors, the last one step;
      t4  worker_bits 8 (R = 1), 63-byte nonce, 596 g + 225: 597 descriptors, the last one step whose
          wave 3 has 33 lanes.
    4100 descriptors: three rounds of the prefix.  And three calls at group 256, "b2047", "b2048" and
    "b2049", of that many descriptors over three tasks -- 1000 descriptors at worker_bits 3 (the last of
    96), 500 whole ones at worker_bits 0 with a 56-byte nonce, and the rest at worker_bits 8 (the last of
    225), so the round boundary behind descriptor 2047 lies inside the third task.  Every k_begin is
    odd, every worker byte non-zero where the partition has one."""
    rnd = random.Random(M_SEED)
    out = []
    for g in H_GROUPS:
        s = 1 if g == 512 else g // 512
        out.append(_scan_call(f"m{g}", g, [
            _call_window(f"m{g}/t0", rnd, 4, rnd.randrange(1, 8), 3, 1500 * g + 256 * s + 96, g),
            _call_window(f"m{g}/t1", rnd, 9, 0, 0, 0, g),
            _call_window(f"m{g}/t2", rnd, 55, rnd.randrange(1, 8), 3, 96, g),
            _call_window(f"m{g}/t3", rnd, 56, 0, 0, 2000 * g + 256, g),
            _call_window(f"m{g}/t4", rnd, 63, rnd.randrange(1, 256), 8, 596 * g + 225, g)]))
    for n in (2047, 2048, 2049):
        out.append(_scan_call(f"b{n}", 256, [
            _call_window(f"b{n}/t0", rnd, 4, rnd.randrange(1, 8), 3, 999 * 256 + 96, 256),
            _call_window(f"b{n}/t1", rnd, 56, 0, 0, 500 * 256, 256),
            _call_window(f"b{n}/t2", rnd, 63, rnd.randrange(1, 256), 8, (n - 1501) * 256 + 225, 256)]))
    return tuple(out)


def family_m_call(name):
    return next(c for c in family_m() if c.name == name)


@functools.lru_cache(maxsize=None)
def family_x():
    """The most descriptors a launch can have: one call of 4096 tasks and 2^28 local indices, group 16384.
    4095 tasks of one k at worker_bits 0 (256 local indices, one short descriptor each) with 4-byte
    nonces of their own and k_begin = j % 300, and at array position 2047 one task of 2^28 - 4095 * 256
    local indices at worker_bits 3: 16320 whole descriptors and one of 256.  20416 descriptors, ten
    rounds of the prefix: small totals in rounds 0 and 9, large ones between, a whole round behind every
    carry."""
    rnd = random.Random(X_SEED)
    base = rnd.randrange(1 << 32)
    large = SCAN_DEV_SLICE - (X_TASKS - 1) * 256
    parts = []
    for j in range(X_TASKS):
        if j == X_LARGE_AT:
            parts.append(_call_window("x/large", rnd, 4, H_WB, H_WBITS, large, SCAN_DEV_MAX_GROUP))
            continue
        nonce = ((base + j) & 0xFFFFFFFF).to_bytes(4, "little")
        parts.append((ScanWindow(f"x/{j}", nonce, 0, 0, j % 300, j % 300 + 1, SCAN_DEV_MAX_GROUP, 1, 0), 256))
    return _scan_call("x", SCAN_DEV_MAX_GROUP, parts)


def window_indices_cuda(wb, wbits, k_begin, n, device, first=0):
    """The global indices (k << 8 | thread byte, k outer) of the local offsets [first, first + n) of a
    window from k_begin, built arithmetically on the device: a torch.int64 tensor."""
    import torch
    rbits = 8 - wbits
    i = torch.arange(first, first + n, dtype=torch.int64, device=device)
    return ((k_begin + (i >> rbits)) << 8) | (wb << rbits) | (i & ((1 << rbits) - 1))


DIGEST_CHUNK = 1 << 22   # entries per digests_cuda call of the reference: a 64 MB digest tensor


def window_depths_cuda(miner, nonce, wb, wbits, k_begin, k_end):
    """The depth of every candidate of a window in index order, by the digest kernel
    (Miner.digests_cuda over window_indices_cuda, DIGEST_CHUNK entries a call): a torch.uint8 tensor on
    the miner's device.  The digest kernel gathers its candidates from a list, one per lane, and
    shares the hash with the device scan's mask kernel but none of its geometry."""
    import torch
    total = (k_end - k_begin) << (8 - wbits)
    dev = torch.device("cuda", miner.device)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    for first in range(0, total, DIGEST_CHUNK):
        n = min(DIGEST_CHUNK, total - first)
        out[first:first + n] = miner.digests_cuda(nonce, window_indices_cuda(wb, wbits, k_begin, n, dev, first))[1]
    return out
