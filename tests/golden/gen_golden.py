#!/usr/bin/env python3
"""Generate tests/golden/pow_golden.json -- golden vectors for the proof-of-work search.

TEST INFRASTRUCTURE.  The reference (philipjesic/Distributed-Proof-Of-Work) is Go,
ships no tests or fixtures, and there is no Go toolchain in this image, so its
outputs cannot be produced by running it.  The vectors here come from

  * an independent pure-Python restatement of the reference's miner loop
    (worker.go:234-244 nextChunk, 246-256 hasNumZeroesSuffix, 301-400 miner),
    using hashlib.md5 (OpenSSL, RFC 1321) and '%x' formatting via bytes.hex();
  * for the two big cases (N=7, N=8: 2.3e8 / 4.1e9 candidates) the C oracle in
    oracle/ (built separately), run over contiguous k sub-windows in parallel
    threads; the first sub-window with a hit is the sequential answer.  Its
    small-case answers are cross-checked against the Python restatement first.

Every case is also checked against SURVEY.md Appendix A where the survey lists it.

  * --deep (added in round 2): N = 9 and 10 first hits (6.9e10 / 1.1e12
    candidates expected), beyond the byte-wise oracle.  They come from
    tests/golden/fast_scan.c, an AVX-512 restatement of the same enumeration,
    which is first cross-checked against every N <= 8 golden above; each new hit
    is then verified with hashlib and its neighbourhood (the 16 k before it) is
    re-searched with the byte-wise C oracle.  Written to the "deep_hits" list,
    the rest of the file is kept as it is.  Cases: BASELINE config 5's "N = 9 on
    fresh nonces seeded random.Random(416)" (4 four-byte nonces; SURVEY.md
    section 8(d) item 5), the config-1/2/5 nonces at N = 9, and [1,2,3,4] at N = 10.

  * --seg-inner: tests/golden/seg_inner_hits.json, all-hits lists for the
    segment-inner kernels (md5_search_si.h search_body_si).  Each case is
    {name, nonce, k_begin, k_end, hits: [[g, tz], ...]}: every candidate
    g = k * 256 + threadByte of the workerBits = 0 window [k_begin, k_end) whose
    hex digest ends in >= 8 '0' characters, with its actual trailing-'0' count,
    sorted by g.  One list serves every partition shape: a partition's hits are
    the entries whose thread byte is in thread_bytes(worker_byte, worker_bits).
    The windows are whole 2^24-k segments (2^32 candidates, ~1 entry each) for
    every W0 = (nonce_len mod 64) / 4 the kernels admit, two midstate nonces
    (64 and 76 bytes), the chunk-length steps at k = 2^40 and 2^48, and the
    last segments below DPOW_K_LIMIT.  They come from fast_scan.c's all-hits
    mode.  Before anything is written
      - all-hits mode is compared with the byte-wise C oracle walked hit by hit
        (mine_window, and per thread byte inside a k) on small windows at
        ntz 4-6, at k = 0, at k >= 2^24, across k = 2^32, 2^40 and 2^48 (chunk
        lengths 4-7) and below DPOW_K_LIMIT, for a 4-, a 12-, a 64- and a
        76-byte nonce;
      - first-hit mode must still reproduce every golden of pow_golden.json it
        can express (workerBits = 0, one final block): first_hits, windows,
        nonce_lengths (which exercises the midstate) and the N = 9 deep_hits
        from k = 0; the N = 10 deep hit (1.7e12 candidates from k = 0, which
        --deep scanned) over the 64 segments that end behind it;
      - every listed hit's digest is recomputed with hashlib.
    The generator enforces (and tests/test_seg_inner_golden.py re-checks): every
    case has >= 4 entries; for each W0 some case has an entry with tz >= 9 behind
    an entry with tz = 8; w1 holds the N = 9 deep golden as its first tz >= 9
    entry.  A case that misses is lengthened in 16-segment steps up to 64
    segments, then its seeded nonce is replaced.

  * --layouts: tests/golden/layout_deep_hits.json, all-hits lists (the same
    [[g, tz], ...] form, ntz 8, workerBits = 0) for every specialised layout
    <NBLK, W0, SH> of md5_search_kernel.h, so that each layout's N >= 8 test
    and its N > 8 full_check are pinned to lists this library had no part in.
    CPU only.  It reads tests/golden/layout_hints.json (tools/layout_hints.py,
    run on the GPU): per case a nonce and one index with >= 9 trailing zeroes
    (8 where the case allows it), found by walking N = 8 hits and checking them
    with hashlib, or by the batch kernel for the tiny k ranges.  A hint is only
    a place to look: it is re-hashed, and the fixture takes the nonce and the
    window's position from it, nothing else.  The window is
    [(s - 1) 2^24 + u, (s + 1) 2^24) with s the hint's 2^24-k segment and u a
    seeded offset below 2^20, clipped to the k of the hint's chunk length (one
    layout per window); the tiny ranges (<1,12,3>, <1,13,0>, <1,13,1>, the
    "_ls" cases below k = 2^16) are scanned whole.  Each case is {name, nonce,
    k_begin, k_end, nblk, w0, sh, deep, hits}; deep says the list has a
    tz >= 9 entry.  <1,13,2> and <1,13,3> have no md5 launch (only k = 0 fits
    one block, or nothing does) and are named under "unreachable".
    fast_scan.c's two-final-block layout (p + 1 + L + 9 > 64) is cross-checked
    before it is used:
      - all-hits and first-hit modes against the byte-wise C oracle walked hit
        by hit, for seeded nonces of 48 ... 63 and 112 ... 127 bytes, on windows
        across k = 256, 65536 and 2^24 (where some of these lengths go from one
        block to two) at ntz 3, 4 and 5;
      - first-hit mode reproduces every two-block golden of pow_golden.json
        (first_hits, nonce_lengths).
    Asserted before the file is written: the hint is in its list; every entry
    re-hashes (hashlib) to its tz; every case but b1w13s1 / ls1 / ls2 has a
    tz >= 9 entry; at least a third of the chunk-length-4 cases have their
    first tz >= 9 entry in the window's second segment (reached with a
    non-zero segment addition); the layouts of the cases and "unreachable"
    are all 72.  The same hints give the same file, byte for byte.

  * --many-plans: tests/golden/many_plans.json, the launch plans of the batched census and the
    batched scan (dpow_census_plan, dpow_scan_plan) and dpow_scan_plan_halve's budgets for a fixed
    list of cases, as the library in the tree returns them: per plan the launch count, the entry
    count and the SHA-256 of the dpow_batch_range rows (tests/_many_plan_cases.py expands a case's
    tasks).  CPU only.  It pins the plans of one commit for the commits after it, so it is run
    before a change to the planner, never after (tests/test_many_plans_golden.py compares).

Usage:  python tests/golden/gen_golden.py [--big] | --deep | --seg-inner | --layouts | --many-plans
"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

RFC1321_SUITE = [  # RFC 1321 Appendix A.5
    ("", "d41d8cd98f00b204e9800998ecf8427e"),
    ("a", "0cc175b9c0f1b6a831c399e269772661"),
    ("abc", "900150983cd24fb0d6963f7d28e17f72"),
    ("message digest", "f96b697d7cb7938d525a2f31aaf161d0"),
    ("abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b"),
    ("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789",
     "d174ab98d277d9f5a5611c2c9f419d9f"),
    ("1234567890" * 8, "57edf4a22be3c955ac49da2e2107b67a"),
]

# SURVEY.md Appendix A (computed by the survey in this container).
SURVEY_APPENDIX_A = {
    ((1, 2, 3, 4), 0): ([0], 0),
    ((1, 2, 3, 4), 1): ([3], 3),
    ((1, 2, 3, 4), 2): ([97], 97),
    ((1, 2, 3, 4), 3): ([97], 97),
    ((1, 2, 3, 4), 4): ([116, 20], 5236),
    ((1, 2, 3, 4), 5): ([149, 103, 2], 157589),
    ((1, 2, 3, 4), 6): ([188, 163, 38], 2532284),
    ((1, 2, 3, 4), 7): ([194, 170, 210, 13], 231910082),
    ((1, 2, 3, 4), 8): ([10, 189, 80, 242], 4065377546),
    ((5, 6, 7, 8), 5): ([84, 244, 3], 259156),
    ((2, 2, 2, 2), 5): ([48, 119], 30512),
    ((2, 2, 2, 2), 7): ([218, 55, 128, 17], 293615578),
    ((2, 2, 2, 2), 8): ([218, 55, 128, 17], 293615578),
}


# ---------------- pure-Python restatement of worker.go ----------------
def next_chunk(chunk):
    """worker.go:234-244 (mutates and returns the list, like the Go slice)."""
    for i in range(len(chunk)):
        if chunk[i] == 0xFF:
            chunk[i] = 0
        else:
            chunk[i] += 1
            return chunk
    chunk.append(1)
    return chunk


def has_num_zeroes_suffix(s, n):
    """worker.go:246-256."""
    found = 0
    for ch in reversed(s):
        if ch == "0":
            found += 1
        else:
            break
    return found >= n


def thread_bytes(worker_byte, worker_bits):
    """worker.go:302-316."""
    rbits = 8 - (worker_bits % 9)
    return [((worker_byte << rbits) | i) & 0xFF for i in range(1 << rbits)]


def chunk_of(k):
    out = []
    while k:
        out.append(k & 0xFF)
        k >>= 8
    return out


def py_mine(nonce, ntz, worker_byte=0, worker_bits=0, k_begin=0, k_end=None):
    """worker.go:301-400 over k in [k_begin, k_end). Returns (secret, global, local) or None."""
    tbs = thread_bytes(worker_byte, worker_bits)
    R = len(tbs)
    chunk = chunk_of(k_begin)
    k = k_begin
    nb = bytes(nonce)
    while k_end is None or k < k_end:
        cb = bytes(chunk)
        for t, tb in enumerate(tbs):
            h = hashlib.md5(nb + bytes([tb]) + cb).hexdigest()  # fmt "%x"
            if has_num_zeroes_suffix(h, ntz):
                return [tb] + list(chunk), k * 256 + tb, k * R + t
        chunk = next_chunk(chunk)
        k += 1
    return None


def md5hex(nonce, secret):
    return hashlib.md5(bytes(nonce) + bytes(secret)).hexdigest()


# ---------------- C oracle driver for the big cases ----------------
def load_oracle():
    path = os.path.join(ROOT, "oracle", "build", "liboracle.so")
    lib = ctypes.CDLL(path)
    lib.oracle_mine_window.restype = ctypes.c_int
    lib.oracle_mine_window.argtypes = [
        ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint8, ctypes.c_uint,
        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t),
        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    return lib


def c_mine(lib, nonce, ntz, wb, wbits, k0, k1):
    sec = ctypes.create_string_buffer(32)
    slen = ctypes.c_size_t()
    g = ctypes.c_uint64()
    loc = ctypes.c_uint64()
    r = lib.oracle_mine_window(bytes(nonce), len(nonce), ntz, wb, wbits, k0, k1, sec,
                               ctypes.byref(slen), ctypes.byref(g), ctypes.byref(loc))
    if r != 1:
        return None
    return list(sec.raw[:slen.value]), g.value, loc.value


def c_mine_parallel(lib, nonce, ntz, k_end, nthreads=8, span=1 << 19):
    """Sequential answer over k in [0, k_end) using contiguous sub-windows in threads."""
    k0 = 0
    while k0 < k_end:
        wins = []
        for j in range(nthreads):
            a = k0 + j * span
            b = min(k_end, a + span)
            if a < b:
                wins.append((a, b))
        res = [None] * len(wins)

        def run(i, a, b):
            res[i] = c_mine(lib, nonce, ntz, 0, 0, a, b)

        ths = [threading.Thread(target=run, args=(i, a, b)) for i, (a, b) in enumerate(wins)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        for r in res:
            if r is not None:
                return r
        k0 = wins[-1][1]
    return None


def config5_fresh_nonces(count=4):
    """BASELINE config 5 / SURVEY.md 8(d) item 5: fresh 4-byte nonces seeded random.Random(416)."""
    rnd = random.Random(416)
    return [[rnd.randrange(256) for _ in range(4)] for _ in range(count)]


def build_fast_scan():
    import subprocess
    out_dir = os.path.join(HERE, "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "fast_scan")
    subprocess.check_call(["gcc", "-O3", "-march=native", "-pthread", "-o", exe, os.path.join(HERE, "fast_scan.c")])
    return exe


def fast_scan(exe, nonce, ntz, k_end=1 << 40, threads=None):
    import subprocess
    threads = threads or os.cpu_count() or 8
    out = subprocess.check_output([exe, bytes(nonce).hex(), str(ntz), "0", str(k_end), str(threads)]).decode().split()
    if out[0] == "none":
        return None
    g = int(out[1])
    k = g >> 8
    return [g & 0xFF] + chunk_of(k), g


def deep(path):
    """N = 9 / 10 first hits via fast_scan, cross-checked first (see module docstring)."""
    import time
    with open(path) as f:
        out = json.load(f)
    exe = build_fast_scan()
    lib = load_oracle()
    for e in out["first_hits"]:  # every N <= 8 golden, incl. the 4.1e9-candidate N = 8 cases
        r = fast_scan(exe, e["nonce"], e["ntz"], k_end=(e["global_idx"] >> 8) + 2)
        assert r is not None and (r[0], r[1]) == (e["secret"], e["global_idx"]), (e, r)
    print("fast_scan agrees with all", len(out["first_hits"]), "first-hit goldens", file=sys.stderr)
    cases = [(n, 9, "config5-fresh-Random(416)") for n in config5_fresh_nonces()]
    cases += [([1, 2, 3, 4], 9, "config1/2 nonce"), ([5, 6, 7, 8], 9, "config5 nonce"),
              ([2, 2, 2, 2], 9, "config5 nonce"), ([1, 2, 3, 4], 10, "config1/2 nonce, N=10")]
    done = {(tuple(e["nonce"]), e["ntz"]) for e in out.get("deep_hits", [])}
    out.setdefault("deep_hits", [])
    for nonce, n, why in cases:
        if (tuple(nonce), n) in done:
            continue
        t = time.time()
        secret, g = fast_scan(exe, nonce, n)
        h = md5hex(nonce, secret)
        assert has_num_zeroes_suffix(h, n), (nonce, n, secret, h)
        k = g >> 8
        # the byte-wise oracle agrees on the neighbourhood: no hit in the 16 k before, this one at k
        near = c_mine(lib, nonce, n, 0, 0, max(0, k - 16), k + 1)
        assert near is not None and near[0] == secret and near[1] == g, (nonce, n, near, g)
        out["deep_hits"].append({"nonce": list(nonce), "ntz": n, "secret": secret, "global_idx": g, "md5": h,
                                 "source": "fast-scan", "case": why})
        print(f"deep hit {nonce} N={n}: {secret} g={g} ({time.time() - t:.0f} s)", file=sys.stderr)
        with open(path, "w") as f:  # checkpoint after every case
            json.dump(out, f, indent=0, separators=(",", ":"))
            f.write("\n")


# ---------------- --seg-inner: all-hits lists for the segment-inner kernels ----------------
SEG = 1 << 24  # k per segment (md5_search_kernel.h: a segment fixes k >> 24)
K_LIMIT = (1 << 55) - 1  # include/dpow.h DPOW_K_LIMIT
SEG_INNER_NTZ = 8
N9_GOLDEN = 48853296051  # deep_hits: [1,2,3,4], N = 9
MAX_SEGS = 64


def secret_from_index(g):
    return [g & 0xFF] + chunk_of(g >> 8)


def tz_of(nonce, g):
    h = md5hex(nonce, secret_from_index(g))
    return len(h) - len(h.rstrip("0"))


def fast_scan_window(exe, nonce, ntz, k0, k1, threads=None):
    """First-hit mode over [k0, k1): global index or None."""
    import subprocess
    threads = threads or os.cpu_count() or 8
    out = subprocess.check_output([exe, bytes(nonce).hex(), str(ntz), str(k0), str(k1), str(threads)]).decode().split()
    return None if out[0] == "none" else int(out[1])


def fast_scan_all(exe, nonce, ntz, k0, k1, threads=None):
    """All-hits mode over [k0, k1): [[g, tz], ...] sorted by g."""
    import subprocess
    threads = threads or os.cpu_count() or 8
    lines = subprocess.check_output(
        [exe, bytes(nonce).hex(), str(ntz), str(k0), str(k1), str(threads), "all"]).decode().splitlines()
    assert lines and lines[-1] == f"end {len(lines) - 1}", lines[-1:]
    hits = []
    for ln in lines[:-1]:
        w = ln.split()
        assert w[0] == "hit" and len(w) == 3, ln
        hits.append([int(w[1]), int(w[2])])
    return hits


def oracle_all_hits(lib, nonce, ntz, k0, k1):
    """The byte-wise oracle walked hit by hit: every hit of the workerBits = 0 window with its
    trailing-zero count.  Inside the k of a hit the later thread bytes are asked one by one
    (workerBits = 8: one thread byte per worker); tz is the largest ntz the oracle still accepts."""
    hits, k = [], k0
    while k < k1:
        r = c_mine(lib, nonce, ntz, 0, 0, k, k1)
        if r is None:
            break
        kh = r[1] >> 8
        for tb in range(r[1] & 0xFF, 256):
            if c_mine(lib, nonce, ntz, tb, 8, kh, kh + 1) is None:
                continue
            tz = ntz
            while tz < 32 and c_mine(lib, nonce, tz + 1, tb, 8, kh, kh + 1) is not None:
                tz += 1
            hits.append([kh * 256 + tb, tz])
        k = kh + 1
    return hits


def seeded_nonce(seed, length):
    rnd = random.Random(seed)
    return [rnd.randrange(256) for _ in range(length)]


def seg_inner_crosscheck(exe, lib, golden):
    """The scanner's new modes against the byte-wise oracle and the existing goldens."""
    nonces = [[1, 2, 3, 4], seeded_nonce(7012, 12), seeded_nonce(7064, 64), seeded_nonce(7076, 76)]
    # (ntz, k_begin, k_end): dense hits; k = 0, k >= 2^24, chunk lengths 4|5, 5|6, 6|7, the top
    wins = [(4, 0, 1 << 13), (5, SEG + 12345, SEG + 12345 + (1 << 15)), (6, 3 * SEG - (1 << 17), 3 * SEG + (1 << 17)),
            (4, (1 << 32) - 4000, (1 << 32) + 4000), (4, (1 << 40) - 4000, (1 << 40) + 4000),
            (5, (1 << 48) - 9000, (1 << 48) + 9000), (4, K_LIMIT - (1 << 13), K_LIMIT)]
    total = 0
    for nonce in nonces:
        for ntz, k0, k1 in wins:
            got = fast_scan_all(exe, nonce, ntz, k0, k1)
            exp = oracle_all_hits(lib, nonce, ntz, k0, k1)
            assert got == exp and (got or ntz > 4), (len(nonce), ntz, k0, k1, got[:4], exp[:4])
            assert all(tz_of(nonce, g) == tz for g, tz in got)
            total += len(got)
    print("all-hits mode agrees with the oracle walk on", len(nonces) * len(wins), "windows,", total, "hits",
          file=sys.stderr)

    def one_block(nonce, k):
        return len(nonce) % 64 + 1 + len(chunk_of(k)) + 9 <= 64

    n = 0
    for e in golden["first_hits"] + golden["nonce_lengths"]:
        k = e["global_idx"] >> 8
        if not one_block(e["nonce"], k + 1):
            continue
        assert fast_scan_window(exe, e["nonce"], e["ntz"], 0, k + 2) == e["global_idx"], e
        n += 1
    for e in golden["windows"]:
        if e["worker_bits"] == 0:
            assert fast_scan_window(exe, e["nonce"], e["ntz"], e["k_begin"], e["k_end"]) == e["global_idx"], e
            n += 1
    for e in golden["deep_hits"]:
        k = e["global_idx"] >> 8
        k0 = 0 if e["ntz"] <= 9 else max(0, (k // SEG + 1 - MAX_SEGS) * SEG)
        assert fast_scan_window(exe, e["nonce"], e["ntz"], k0, k + 2) == e["global_idx"], e
        n += 1
    print("first-hit mode reproduces", n, "existing goldens", file=sys.stderr)


def _n9_after_8(hits):
    """An entry with tz >= 9 behind an entry with tz = 8."""
    seen8 = False
    for _, tz in hits:
        if tz == 8:
            seen8 = True
        elif seen8 and tz >= 9:
            return True
    return False


def seg_inner_cases():
    """name -> (nonce length or the nonce, seed, window(extra) with extra = 0, 16, 32, 48 more segments)."""
    def around(edge):
        return lambda x: (edge - (4 + x // 2) * SEG, edge + (4 + x // 2) * SEG)
    return [
        ("w0", [], None, lambda x: (SEG + 12345, (17 + x) * SEG + 12345)),
        ("w1", [1, 2, 3, 4], None, lambda x: (SEG + 777, 33 * SEG - 4321)),
        ("w2", 8, 8001, lambda x: (2 * SEG + 54321, (18 + x) * SEG + 54321)),
        ("w3", 12, 12001, lambda x: (SEG + 999, (17 + x) * SEG + 999)),
        ("m0", 64, 64001, lambda x: (SEG + 4097, (9 + x) * SEG + 4097)),
        ("m3", 76, 76001, lambda x: (3 * SEG + 31, (11 + x) * SEG + 31)),
        ("l56", [1, 2, 3, 4], None, around(1 << 40)),
        ("l67", [1, 2, 3, 4], None, around(1 << 48)),
        ("top", [1, 2, 3, 4], None, lambda x: (K_LIMIT - (8 + x) * SEG, K_LIMIT)),
    ]


def seg_inner(path):
    import time
    t_all = time.time()
    with open(os.path.join(HERE, "pow_golden.json")) as f:
        golden = json.load(f)
    exe = build_fast_scan()
    lib = load_oracle()
    seg_inner_crosscheck(exe, lib, golden)
    print(f"cross-checks: {time.time() - t_all:.0f} s", file=sys.stderr)

    def scan(name, nonce, win, need):
        """Lengthen in 16-segment steps until `need` holds; None when 64 segments do not do."""
        hits, done_to = [], None
        for extra in range(0, MAX_SEGS, 16):
            k0, k1 = win(extra)
            if (k1 - k0 + SEG - 1) // SEG > MAX_SEGS:
                break
            t = time.time()
            if done_to is None:
                hits = fast_scan_all(exe, nonce, SEG_INNER_NTZ, k0, k1)
            elif (k0, k1) == done_to:
                break  # a fixed window
            else:  # only the new k: below and above what is scanned
                hits = (fast_scan_all(exe, nonce, SEG_INNER_NTZ, k0, done_to[0]) + hits
                        + fast_scan_all(exe, nonce, SEG_INNER_NTZ, done_to[1], k1))
            done_to = (k0, k1)
            print(f"{name}: [{k0}, {k1}) {len(hits)} entries, {sum(tz >= 9 for _, tz in hits)} with tz >= 9 "
                  f"({time.time() - t:.0f} s)", file=sys.stderr)
            if need(hits):
                return {"name": name, "nonce": list(nonce), "k_begin": k0, "k_end": k1, "hits": hits}
        return None

    # the cases that are not their W0's first: >= 4 entries; then the first of each W0 also has to
    # provide the N = 9 entry behind an N = 8 one if no other case of that W0 does
    group = {"w0": ("m0",), "w1": ("l56", "l67", "top"), "w2": (), "w3": ("m3",)}
    spec = {c[0]: c for c in seg_inner_cases()}
    done = {}

    def run(name, need):
        _, nonce, seed, win = spec[name]
        attempt = 0
        while True:
            nv = nonce if seed is None else seeded_nonce(seed + attempt, nonce)
            c = scan(name, nv, win, need)
            if c is not None:
                done[name] = c
                return
            assert seed is not None, f"{name}: a fixed nonce misses its condition at {MAX_SEGS} segments"
            attempt += 1

    for first, others in group.items():
        for name in others:
            run(name, lambda h: len(h) >= 4)
        covered = any(_n9_after_8(done[o]["hits"]) for o in others)
        run(first, lambda h: len(h) >= 4 and (covered or _n9_after_8(h)))

    cases = [done[c[0]] for c in seg_inner_cases()]
    for c in cases:
        gs = [g for g, _ in c["hits"]]
        assert gs == sorted(set(gs)) and all(c["k_begin"] <= g >> 8 < c["k_end"] for g in gs), c["name"]
        for g, tz in c["hits"]:
            assert tz >= SEG_INNER_NTZ and tz_of(c["nonce"], g) == tz, (c["name"], g, tz)
    first9 = next(g for g, tz in done["w1"]["hits"] if tz >= 9)
    assert first9 == N9_GOLDEN and _n9_after_8(done["w1"]["hits"]), first9
    with open(path, "w") as f:
        json.dump({"ntz": SEG_INNER_NTZ, "cases": cases}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    for c in cases:
        print(f"{c['name']}: {len(c['hits'])} entries, {sum(tz >= 9 for _, tz in c['hits'])} with tz >= 9",
              file=sys.stderr)
    print(f"--seg-inner: {time.time() - t_all:.0f} s", file=sys.stderr)


# ---------------- --layouts: all-hits lists for every specialised layout ----------------
LAYOUT_NTZ = 8
# layouts with no md5 launch: one final block only fits the chunk of zero bytes (k = 0, the k = 0 kernel)
LAYOUT_UNREACHABLE = [
    {"nblk": 1, "w0": 13, "sh": 2, "reason": "nonce length 54 mod 64: one block holds only k = 0 (54 + 1 + 0 + 9 = 64)"},
    {"nblk": 1, "w0": 13, "sh": 3, "reason": "nonce length 55 mod 64: no k fits one block (55 + 1 + 0 + 9 = 65)"},
]
LAYOUT_MAY_BE_SHALLOW = ("b1w13s1", "ls1", "ls2")  # tz >= 9 not required (tools/layout_hints.py)


def chunk_range(k):
    """[lo, hi) of the k whose chunk is as long as k's (k >= 1), below DPOW_K_LIMIT."""
    n = len(chunk_of(k))
    return 1 << (8 * (n - 1)), min(1 << (8 * n), K_LIMIT)


def layout_of(nonce_len, k):
    """(nblk, w0, sh) of md5_search_kernel.h's layout for a candidate: final blocks behind the
    midstate, the thread byte's word and byte in them."""
    p = nonce_len % 64
    return (2 if p + 1 + len(chunk_of(k)) + 9 > 64 else 1), p // 4, p % 4


def layouts_crosscheck(exe, lib, golden):
    """The scanner's two-final-block layout against the byte-wise oracle and the existing goldens."""
    total = wins = 0
    for ln in list(range(48, 64)) + list(range(112, 128)):
        nonce = seeded_nonce(8000 + ln, ln)
        for edge in (1 << 8, 1 << 16, 1 << 24):  # chunk lengths 1|2, 2|3, 3|4: one block | two for some of these
            for ntz, half in ((3, 1 << 6), (4, 1 << 9), (5, 1 << 11)):
                k0, k1 = max(0, edge - half), edge + half
                got = fast_scan_all(exe, nonce, ntz, k0, k1)
                exp = oracle_all_hits(lib, nonce, ntz, k0, k1)
                assert got == exp, (ln, ntz, k0, k1, got[:4], exp[:4])
                assert all(tz_of(nonce, g) == tz for g, tz in got)
                first = fast_scan_window(exe, nonce, ntz, k0, k1)
                assert first == (exp[0][0] if exp else None), (ln, ntz, k0, k1, first)
                total += len(got)
                wins += 1
    assert total >= wins  # about 8, 4 and 1 hits per window
    print("two-block all-hits and first-hit modes agree with the oracle walk on", wins, "windows,", total, "hits",
          file=sys.stderr)
    n = 0
    for e in golden["first_hits"] + golden["nonce_lengths"]:
        k = e["global_idx"] >> 8
        if layout_of(len(e["nonce"]), k)[0] == 2:
            assert fast_scan_window(exe, e["nonce"], e["ntz"], 0, k + 2) == e["global_idx"], e
            n += 1
    assert n >= 10, n
    print("first-hit mode reproduces", n, "existing two-block goldens", file=sys.stderr)


def layouts(path):
    """tests/golden/layout_deep_hits.json from tests/golden/layout_hints.json (see the module docstring)."""
    import time
    t_all = time.time()
    with open(os.path.join(HERE, "pow_golden.json")) as f:
        golden = json.load(f)
    with open(os.path.join(HERE, "layout_hints.json")) as f:
        hints = json.load(f)["hints"]
    exe = build_fast_scan()
    lib = load_oracle()
    layouts_crosscheck(exe, lib, golden)
    print(f"cross-checks: {time.time() - t_all:.0f} s", file=sys.stderr)
    cases = []
    for h in hints:
        name, nonce, g = h["name"], h["nonce"], h["global_idx"]
        assert tz_of(nonce, g) >= LAYOUT_NTZ, (name, "the hint does not re-hash")
        k = g >> 8
        lo, hi = chunk_range(k)
        if h["whole_range"]:  # a tiny k range: all of it
            k0, k1 = h["k_lo"], h["k_hi"]
            assert 1 <= k0 < k1 <= 1 << 24, (name, k0, k1)
        else:
            s = k // SEG
            u = random.Random(f"layouts/{name}").randrange(1 << 20)
            k0, k1 = max((s - 1) * SEG + u, lo), min((s + 1) * SEG, hi)
        assert 1 <= k0 <= k < k1 <= K_LIMIT, (name, k0, k, k1)
        lay = layout_of(len(nonce), k0)
        assert lay == layout_of(len(nonce), k1 - 1) == layout_of(len(nonce), k), (name, "one layout per window")
        t = time.time()
        hits = fast_scan_all(exe, nonce, LAYOUT_NTZ, k0, k1)
        gs = [x for x, _ in hits]
        assert g in gs, (name, "the hint is not in the list")
        assert gs == sorted(set(gs)) and all(k0 <= x >> 8 < k1 for x in gs), name
        for x, tz in hits:
            assert tz >= LAYOUT_NTZ and tz_of(nonce, x) == tz, (name, x, tz)
        deep_case = any(tz >= 9 for _, tz in hits)
        assert deep_case or name in LAYOUT_MAY_BE_SHALLOW, (name, "no tz >= 9 entry")
        cases.append({"name": name, "nonce": list(nonce), "k_begin": k0, "k_end": k1, "nblk": lay[0], "w0": lay[1],
                      "sh": lay[2], "deep": deep_case, "hits": hits})
        print(f"{name}: <{lay[0]},{lay[1]},{lay[2]}> [{k0}, {k1}) {len(hits)} entries, "
              f"{sum(tz >= 9 for _, tz in hits)} with tz >= 9 ({time.time() - t:.0f} s)", file=sys.stderr)
    # chunk length 4: the first tz >= 9 entry in the window's second segment (a non-zero segment
    # addition in the launch that reaches it) for at least a third
    l4 = [c for c in cases if c["name"].startswith("len")]
    second = [c["name"] for c in l4
              if (next(x for x, tz in c["hits"] if tz >= 9) >> 8) // SEG > c["k_begin"] // SEG]
    assert len(l4) == 64 and 3 * len(second) >= len(l4), (len(second), len(l4))
    have = {(c["nblk"], c["w0"], c["sh"]) for c in cases} | {(u["nblk"], u["w0"], u["sh"]) for u in LAYOUT_UNREACHABLE}
    assert len(have) == 72, sorted(have)
    with open(path, "w") as f:
        json.dump({"ntz": LAYOUT_NTZ, "unreachable": LAYOUT_UNREACHABLE, "cases": cases}, f, indent=0,
                  separators=(",", ":"))
        f.write("\n")
    print(f"--layouts: {len(cases)} cases, {len(second)} of {len(l4)} chunk-length-4 cases with their first "
          f"tz >= 9 entry in the second segment, {time.time() - t_all:.0f} s", file=sys.stderr)


def _gpu_test_seam_tasks():
    """The task sets whose launch seams tests/test_gpu_scan_many.py (_seam_tasks: the same draws from
    random.Random(5), without the nonces) and tests/test_gpu_census_many.py (test_launch_seams) walk."""
    rnd = random.Random(5)
    scan = [(253, 259, 0, 1), (65536 - 1536, 65536 + 1536, 8, 0), (65533, 65539, 0, 2), (254, 258, 0, 0)]
    while len(scan) < 30:
        wbits = rnd.choice((0, 0, 1, 3, 8))
        k0 = rnd.choice((0, 250, 65530))
        rnd.randrange(0, 130)  # (the nonce's length)
        ntz = rnd.choice((0, 1, 2, 3))
        rnd.randrange(1 << wbits)  # (the worker byte)
        scan.append((k0, k0 + rnd.randrange(1, 14), wbits, ntz))
    census = [[(k0 + 0, k0 + n, 3, 0) for n in sizes]
              for sizes, k0 in (((1000, 5000, 256, 12288, 3), 0), ((100, 3, 2, 200, 1, 130), 65500))]
    return scan, census


def many_plans_cases():
    """(name, tasks spec, [(plan, cap, capacity), ...]) of many_plans.json; _many_plan_cases.expand reads a spec."""
    every_cap, every_capacity = (256, 4096, 1 << 28), (1024, 65536)
    both = [("census", c, 0) for c in (0,) + every_cap] + [("scan", c, y) for c in (0,) + every_cap for y in every_capacity]
    big = [p for p in both if p[1] in (0, 1 << 28)]  # (a small budget would make millions of entries of a long task)
    scan_seams, census_seams = _gpu_test_seam_tasks()
    mixed = {"seed": 11, "n": 96, "worker_bits": [0, 3, 8], "ntz": [0, 1, 6, 7, 9], "k_starts": [0, 250, 65530, 1 << 24],
             "max_k": 300, "empty": 7}
    cases = [
        ("one task", {"list": [[3, 1003, 0, 3]]}, both),
        ("one task of three launches", {"list": [[5, 5 + (3 << 20), 0, 9]]}, big),
        ("4096 tasks of 256 indices", {"repeat": [7, 8, 0, 1], "n": 4096}, both),
        ("4096 tasks of one index", {"repeat": [70000, 70001, 8, 0], "n": 4096}, both),
        ("empty tasks at the front, in the middle and at the end",
         {"list": [[9, 9, 0, 1], [0, 0, 3, 0], [4, 30, 0, 1], [77, 77, 8, 6], [1 << 30, 1 << 30, 0, 9], [250, 270, 3, 0],
                   [12, 12, 0, 7], [5, 5, 8, 0]]}, both),
        ("only empty tasks", {"list": [[9, 9, 0, 1], [0, 0, 3, 0], [1 << 40, 1 << 40, 8, 9]]}, both),
        # 2560, 6656 and 1280 indices under 4096: the second is cut after 1536 and after 5632
        ("a task cut by two seams", {"list": [[0, 10, 0, 2], [10, 36, 0, 2], [0, 5, 0, 2]]},
         [("census", 4096, 0), ("scan", 4096, 65536), ("scan", 4096, 1024)]),
        ("mixed widths and depths", mixed, both),
        ("many mixed tasks", dict(mixed, seed=12, n=4096, max_k=40), both),
        ("long and short tasks, deep and shallow",
         {"list": [[0, 1 << 21, 0, 7], [5, 9, 3, 0], [100, 100 + (1 << 20), 0, 9], [0, 300, 8, 1],
                   [1 << 24, (1 << 24) + (3 << 19), 3, 6], [0, 40, 0, 0], [65530, 65530 + (1 << 12), 0, 1],
                   [1 << 32, (1 << 32) + (1 << 28), 8, 7], [255, 257, 0, 9]]}, big),
        ("test_gpu_scan_many seams", {"list": [list(t) for t in scan_seams]},
         [("scan", c, 0) for c in (0, 512, 768)] + [("census", c, 0) for c in (0, 512, 768)]),
    ]
    for j, tasks in enumerate(census_seams):
        cases.append((f"test_gpu_census_many seams {j}", {"list": [list(t) for t in tasks]},
                      [("census", 4096, 0), ("census", 0, 0), ("scan", 4096, 0)]))
    return cases


MANY_PLANS_HALVE = [(256, 256), (1 << 28, 16384), (257, 1), (512, 512), (513, 300), (1000, 16384), (65536, 4096),
                    (1 << 20, 1 << 16), ((1 << 28) - 256, 16383), (1 << 27, 255), (3 << 26, 9999), (1 << 29, 1 << 20)]


def many_plans(path):
    """tests/golden/many_plans.json: what dpow_census_plan, dpow_scan_plan and dpow_scan_plan_halve of
    the library in the tree return for a fixed list of cases -- per plan the launch count, the entry
    count and the SHA-256 of the returned dpow_batch_range rows.  Recorded before the three batched
    host loops were put on one planner, to pin the plans across that change: it is not run again
    when the planner changes, the committed file is the yardstick."""
    for p in (os.path.join(ROOT, "distributed-proof-of-work_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import distpow
    from _many_plan_cases import census_windows, digest, expand, scan_windows
    out = {"build_id": distpow.build_id(), "cases": [], "halve": []}
    for name, spec, plans in many_plans_cases():
        tasks = expand(spec)
        rows = []
        for plan, cap, capacity in plans:
            if plan == "census":
                blocks, launches = distpow.census_plan(census_windows(tasks), cap)
            else:
                blocks, launches = distpow.scan_plan(scan_windows(tasks), cap, capacity)
            rows.append({"plan": plan, "cap": cap, "capacity": capacity, "launches": launches, "entries": len(blocks),
                         "sha256": digest(blocks)})
            print(f"{name}: {plan} cap {cap} capacity {capacity}: {launches} launches, {len(blocks)} entries",
                  file=sys.stderr)
        out["cases"].append({"name": name, "tasks": spec, "n_tasks": len(tasks), "plans": rows})
    for total, weight in MANY_PLANS_HALVE:
        cap, capacity = distpow.scan_plan_halve(total, weight)
        out["halve"].append({"total": total, "weight": weight, "cap": cap, "capacity": capacity})
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--many-plans", action="store_true",
                    help="write many_plans.json: digests of the batched census's and the batched scan's launch plans")
    ap.add_argument("--layouts", action="store_true",
                    help="write layout_deep_hits.json from layout_hints.json: all-hits lists per layout (fast_scan)")
    ap.add_argument("--big", action="store_true", help="also compute N=7/8 cases via the C oracle")
    ap.add_argument("--deep", action="store_true", help="add N=9/10 hits (fast_scan) to the existing file")
    ap.add_argument("--seg-inner", action="store_true",
                    help="write seg_inner_hits.json: all-hits lists for the segment-inner kernels (fast_scan)")
    args = ap.parse_args()
    if args.many_plans:
        many_plans(os.path.join(HERE, "many_plans.json"))
        return
    if args.layouts:
        layouts(os.path.join(HERE, "layout_deep_hits.json"))
        return
    if args.seg_inner:
        seg_inner(os.path.join(HERE, "seg_inner_hits.json"))
        return
    if args.deep:
        deep(os.path.join(HERE, "pow_golden.json"))
        return

    out = {"rfc1321": [{"msg_hex": m.encode().hex(), "md5": d} for m, d in RFC1321_SUITE],
           "first_hits": [], "partitions": [], "windows": [], "nonce_lengths": []}
    for m, d in RFC1321_SUITE:
        assert hashlib.md5(m.encode()).hexdigest() == d

    # 1) first hits, workerBits = 0 (the deterministic answer)
    small = [((1, 2, 3, 4), n) for n in range(0, 7)] + [((5, 6, 7, 8), 5), ((2, 2, 2, 2), 5),
                                                       ((5, 6, 7, 8), 3), ((9, 9, 9, 9), 4),
                                                       ((0, 0, 0, 0), 4), ((255, 255, 255, 255), 4)]
    for nonce, n in small:
        secret, g, loc = py_mine(nonce, n)
        exp = SURVEY_APPENDIX_A.get((nonce, n))
        if exp is not None:
            assert (secret, g) == (exp[0], exp[1]), (nonce, n, secret, g, exp)
        out["first_hits"].append({"nonce": list(nonce), "ntz": n, "secret": secret, "global_idx": g,
                                  "md5": md5hex(nonce, secret), "source": "python"})
        print("first hit", nonce, n, secret, g, file=sys.stderr)

    # 2) per-partition first hits (worker_byte, worker_bits) -> the multi-GPU min rule
    for wbits in (1, 2, 3):
        for n in (1, 2, 3, 4, 5):
            for wb in range(1 << wbits):
                secret, g, loc = py_mine((1, 2, 3, 4), n, wb, wbits)
                out["partitions"].append({"nonce": [1, 2, 3, 4], "ntz": n, "worker_byte": wb,
                                          "worker_bits": wbits, "secret": secret, "global_idx": g,
                                          "local_idx": loc})
    # quirks: non-power-of-two worker counts (coordinator.go:326 floor(log2 W)), wbits % 9
    for wb, wbits in ((2, 1), (5, 2), (3, 9), (1, 10), (7, 8)):
        secret, g, loc = py_mine((1, 2, 3, 4), 3, wb, wbits)
        out["partitions"].append({"nonce": [1, 2, 3, 4], "ntz": 3, "worker_byte": wb,
                                  "worker_bits": wbits, "secret": secret, "global_idx": g,
                                  "local_idx": loc})

    # 3) windows starting at chunk-length (segment) boundaries
    for k0 in (0, 1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 24) + 12345,
               (1 << 32) - 1, 1 << 32):
        for n in (1, 2, 3):
            for wbits, wb in ((0, 0), (2, 3), (3, 5)):
                r = py_mine((1, 2, 3, 4), n, wb, wbits, k_begin=k0, k_end=k0 + 4096)
                secret, g, loc = r
                out["windows"].append({"nonce": [1, 2, 3, 4], "ntz": n, "worker_byte": wb,
                                       "worker_bits": wbits, "k_begin": k0, "k_end": k0 + 4096,
                                       "secret": secret, "global_idx": g, "local_idx": loc})

    # 4) nonce lengths 0..80 (single block, two final blocks, midstate blocks)
    for ln in list(range(0, 72)) + [100, 119, 120, 127, 128, 200]:
        nonce = [(i * 37 + ln) & 0xFF for i in range(ln)]
        for n in (2, 3):
            secret, g, loc = py_mine(nonce, n)
            out["nonce_lengths"].append({"nonce": nonce, "ntz": n, "secret": secret, "global_idx": g})

    # 5) big cases via the C oracle (cross-checked on small cases first)
    if args.big:
        lib = load_oracle()
        for e in out["first_hits"][:6]:
            r = c_mine_parallel(lib, e["nonce"], e["ntz"], 1 << 20)
            assert r is not None and r[0] == e["secret"] and r[1] == e["global_idx"], (e, r)
        for nonce, n in (((1, 2, 3, 4), 7), ((2, 2, 2, 2), 7), ((2, 2, 2, 2), 8), ((1, 2, 3, 4), 8)):
            secret, g, loc = c_mine_parallel(lib, nonce, n, 1 << 32)
            exp = SURVEY_APPENDIX_A[(nonce, n)]
            assert (secret, g) == (exp[0], exp[1]), (nonce, n, secret, g, exp)
            assert has_num_zeroes_suffix(md5hex(nonce, secret), n)
            out["first_hits"].append({"nonce": list(nonce), "ntz": n, "secret": secret, "global_idx": g,
                                      "md5": md5hex(nonce, secret), "source": "c-oracle"})
            print("big first hit", nonce, n, secret, g, file=sys.stderr)

    with open(os.path.join(HERE, "pow_golden.json"), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
