#!/usr/bin/env python3
"""Hints for tests/golden/layout_deep_hits.json (GPU box only):

    python tools/layout_hints.py [--out tests/golden/layout_hints.json]

For every specialised layout <NBLK, W0, SH> of md5_search_kernel.h this finds one place to look:
a global index g = k * 256 + threadByte whose hex digest ends in >= 9 '0' characters, with the
nonce and the k range it was looked for in.  gen_golden.py --layouts then scans a window round
each hint on the CPU (tests/golden/fast_scan.c) and writes the fixture from the scan alone: a hint
contributes the nonce and the window's position, nothing else.

How an index is found, so that it does not depend on the code the fixture is meant to pin (the
N > 8 branch, full_check / md5_tail<.., 1>):
  - "walk": N = 8 searches (D-equality or the two-block prefilter), each resuming behind the last
    hit; every hit, and the later thread bytes of its k, is hashed with hashlib and the first one
    with >= 9 trailing zeroes is the hint;
  - "many": for layouts whose whole k range is tiny, Miner.mine_many (the batch kernel, which
    shares nothing with the specialised kernels' deep paths) over many nonces, each hit checked
    with hashlib.
No N >= 9 search of the specialised kernels is made.

Cases (nonces from seeded_nonce, a tiny-range nonce's first four bytes replaced by a counter):
  - len00 ... len63: chunk length 4 (walk from k = 2^24), every layout chunk length 4 reaches;
  - b2w12s2 / b2w12s1 / b2w12s0: <2,12,2..0>, nonce lengths 50 / 49 / 48 from k = 2^32 / 2^40 / 2^48;
  - b1w12s3: <1,12,3>, length 51, k in [65536, 2^24); b1w13s0: <1,13,0>, length 52, k in
    [256, 65536); b1w13s1: <1,13,1>, length 53, k in [1, 256) (>= 9 zeroes if one turns up within
    TINY_BUDGET_S, else 8: "deep" false);
  - c5 / c6 / c7: one final block at chunk lengths 5, 6, 7;
  - mid69 / mid115 / mid190: midstate nonces of 64 + 5, 64 + 51 and 128 + 62 bytes;
  - ls1 / ls2: the "_ls" kernels (SH = 0, k in [1, 65536) at N = 8), one and two final blocks,
    >= 8 zeroes.
"""
import argparse
import hashlib
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-proof-of-work_amd"))

SEG = 1 << 24
TINY_BUDGET_S = 60.0


def seeded_nonce(seed, length):
    """gen_golden.seeded_nonce."""
    rnd = random.Random(seed)
    return [rnd.randrange(256) for _ in range(length)]


def secret_of(g):
    out, k = [g & 0xFF], g >> 8
    while k:
        out.append(k & 0xFF)
        k >>= 8
    return bytes(out)


def tz_of(nonce, g):
    h = hashlib.md5(bytes(nonce) + secret_of(g)).hexdigest()
    return len(h) - len(h.rstrip("0"))


def cases():
    """(name, how, nonce length, seed, k_lo, k_hi, wanted zeroes)."""
    out = [(f"len{n:02d}", "walk", n, 9000 + n, 1 << 24, 1 << 32, 9) for n in range(64)]
    out += [("b2w12s2", "walk", 50, 9150, 1 << 32, 1 << 40, 9),
            ("b2w12s1", "walk", 49, 9149, 1 << 40, 1 << 48, 9),
            ("b2w12s0", "walk", 48, 9148, 1 << 48, (1 << 55) - 1, 9),
            ("b1w12s3", "walk-nonces", 51, 9251, 1 << 16, 1 << 24, 9),
            ("b1w13s0", "many", 52, 9252, 1 << 8, 1 << 16, 9),
            ("b1w13s1", "many", 53, 9253, 1, 1 << 8, 9),
            ("c5", "walk", 5, 9305, 1 << 32, 1 << 40, 9),
            ("c6", "walk", 22, 9322, 1 << 40, 1 << 48, 9),
            ("c7", "walk", 35, 9335, 1 << 48, (1 << 55) - 1, 9),
            ("mid69", "walk", 69, 9469, 1 << 24, 1 << 32, 9),
            ("mid115", "walk", 115, 9515, 1 << 24, 1 << 32, 9),
            ("mid190", "walk", 190, 9590, 1 << 24, 1 << 32, 9),
            ("ls1", "many", 8, 9608, 1, 1 << 16, 8),
            ("ls2", "many", 56, 9656, 1, 1 << 16, 8)]
    return out


def walk(m, distpow, nonce, k_lo, k_hi, want):
    """The first index of [k_lo, k_hi) with >= want zeroes among the N = 8 hits, or None."""
    k, n8 = k_lo, 0
    while k < k_hi:
        ke = min(k_hi, k + 256 * SEG)
        r = m.search(nonce, 8, 0, 0, k, ke)
        if r.status != distpow.FOUND:
            assert r.status == distpow.EXHAUSTED, r
            k = ke
            continue
        g = r.global_idx
        n8 += 1
        for t in range(g & 0xFF, 256):
            if tz_of(nonce, (g >> 8) << 8 | t) >= want:
                return (g >> 8) << 8 | t, n8
        k = (g >> 8) + 1
    return None, n8


def variant(base, i):
    """base with its first four bytes replaced by the counter i."""
    return [(i >> (8 * b)) & 0xFF for b in range(4)] + base[4:]


def many(m, distpow, base, k_lo, k_hi, want, budget_s):
    """mine_many over variants of base: (nonce, g, tz) of the first hit with >= want zeroes; when the
    budget runs out, of the first one with 8."""
    from distpow import BatchTask
    ntz = 9 if want >= 9 and (k_hi - k_lo) * 256 >= 1 << 20 else 8  # tiny ranges: take N = 8 hits, keep one as a fallback
    t0, i, fallback, per = time.perf_counter(), 0, None, 4096
    while True:
        nonces = [variant(base, i + j) for j in range(per)]
        i += per
        res = m.mine_many([BatchTask(n, ntz, 0, 0, k_lo) for n in nonces], k_limit=k_hi, window=k_hi - k_lo)
        for n, r in zip(nonces, res):
            if r.status != distpow.FOUND:
                assert r.status == distpow.EXHAUSTED, r
                continue
            tz = tz_of(n, r.global_idx)
            assert tz >= ntz and k_lo <= r.global_idx >> 8 < k_hi, (n, r)
            if tz >= want:
                return n, r.global_idx, tz, i
            if fallback is None and tz >= 8:
                fallback = (n, r.global_idx, tz)
        if time.perf_counter() - t0 > budget_s:
            assert fallback is not None, "no N = 8 hit within the budget"
            return fallback + (i,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "layout_hints.json"))
    ap.add_argument("--only", default="", help="comma-separated case names")
    args = ap.parse_args()
    import distpow
    only = set(filter(None, args.only.split(",")))
    hints = []
    t_all = time.perf_counter()
    with distpow.Miner(0) as m:
        for name, how, length, seed, k_lo, k_hi, want in cases():
            if only and name not in only:
                continue
            t = time.perf_counter()
            note = ""
            if how == "walk":
                nonce = seeded_nonce(seed, length)
                g, n8 = walk(m, distpow, nonce, k_lo, k_hi, want)
                assert g is not None, name
                note = f"{n8} N = 8 hits walked"
            elif how == "walk-nonces":
                base, i, g = seeded_nonce(seed, length), 0, None
                while g is None:
                    nonce = variant(base, i)
                    g, _ = walk(m, distpow, nonce, k_lo, k_hi, want)
                    i += 1
                note = f"{i} nonces walked"
            else:
                nonce, g, tz, i = many(m, distpow, seeded_nonce(seed, length), k_lo, k_hi, want, TINY_BUDGET_S)
                note = f"{i} nonces mined"
            tz = tz_of(nonce, g)
            assert tz >= min(want, 8) and k_lo <= g >> 8 < k_hi
            hints.append({"name": name, "nonce": nonce, "global_idx": g, "tz": tz, "k_lo": k_lo, "k_hi": k_hi,
                          "whole_range": how != "walk"})
            print(f"{name}: g {g} (k segment {(g >> 8) // SEG}) tz {tz}, {note}, {time.perf_counter() - t:.2f} s",
                  flush=True)
            with open(args.out, "w") as f:  # checkpoint after every case
                json.dump({"hints": hints}, f, indent=0, separators=(",", ":"))
                f.write("\n")
    print(f"{len(hints)} hints in {time.perf_counter() - t_all:.0f} s -> {args.out}")


if __name__ == "__main__":
    main()
