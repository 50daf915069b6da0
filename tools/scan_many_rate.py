"""The batched scan's measurements on one GPU, by tools/census_many_rate.py's method.

  kernel_rate  one N = 32 task over 2^28 k of the full partition (2^36 candidates) through
               dpow_scan_batch beside dpow_scan on the same window (candidates over the launches' own
               ticks), alternating in one process
  tasks        fresh 4-byte nonces at N = 3, B in {1, 16, 256, 4096} tasks of 2^12, 2^16 and 2^20
               candidates: one Miner.scan_many call beside Miner.scan looped on the same context,
               alternating; tasks per second of each and their ratio
  dense        N = 0, 64 tasks of 2^12 candidates (2^18 hits, 16 launches): the call's kernel_ms beside
               its wall time, and the same windows through Miner.scan_page in a loop
Medians of REPS repetitions after one warm-up of each shape; a host clock around calls that return
only when the answers are back.  Python's collector is run between the repetitions of B >= 256.

    python3 tools/scan_many_rate.py [--reps 5] [--out profiles/scan_many_rate.json] [--rate-log2k 28]
"""
import argparse
import gc
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-proof-of-work_amd"))

import distpow  # noqa: E402
from distpow import ScanTask  # noqa: E402


def med(xs):
    return statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-rate-only", action="store_true",
                    help="the kernel-rate section alone (an A/B of two builds needs nothing else)")
    ap.add_argument("--rate-log2k", type=int, default=28)
    args = ap.parse_args()
    miner = distpow.Miner(0)
    nonce = [1, 2, 3, 4]
    rnd = random.Random(17)

    def fresh(b):
        return [bytes(rnd.randrange(256) for _ in range(4)) for _ in range(b)]

    # -- the kernel's rate beside scan_kernel's -----------------------------------------------------
    k0, nk = 1 << 24, 1 << args.rate_log2k
    miner.scan(nonce, 32, 0, 0, k0, k0 + (1 << 20))
    miner.scan_many([ScanTask(nonce, 32, 0, 0, k0, k0 + (1 << 20))])
    many_k, many_w, one_k, one_w = [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        (r, hits, k_done), = miner.scan_batch([ScanTask(nonce, 32, 0, 0, k0, k0 + nk)])
        many_w.append(nk * 256 / (time.perf_counter() - t0) / 1e9)
        st = miner.last_scan_many_stats
        assert (r, hits, k_done, st.candidates) == (distpow.EXHAUSTED, [], k0 + nk, nk * 256)
        many_k.append(st.candidates / (st.kernel_ms * 1e-3) / 1e9)
        launches = st.launches
        t0 = time.perf_counter()
        r, hits, k_done = miner.scan_page(nonce, 32, 0, 0, k0, k0 + nk)
        one_w.append(nk * 256 / (time.perf_counter() - t0) / 1e9)
        s1 = miner.last_scan_stats
        assert (r, hits, k_done, s1.candidates, s1.launches) == (distpow.EXHAUSTED, [], k0 + nk, nk * 256, launches)
        one_k.append(s1.candidates / (s1.kernel_ms * 1e-3) / 1e9)
    rate = {"candidates": nk * 256, "launches": launches, "scan_many_kernel_ghs": med(many_k),
            "scan_many_wall_ghs": med(many_w), "scan_kernel_ghs": med(one_k), "scan_wall_ghs": med(one_w),
            "many_over_scan_kernel": med(many_k) / med(one_k), "goal": 0.95,
            "scan_many_kernel_ghs_all": many_k, "scan_kernel_ghs_all": one_k}
    print(json.dumps({"kernel_rate": rate}), file=sys.stderr, flush=True)
    if args.kernel_rate_only:
        only = {"tool": "tools/scan_many_rate.py", "reps": args.reps, "build_id": distpow.build_id(), "kernel_rate": rate}
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(only, indent=1) + "\n")
        print(json.dumps(only))
        miner.close()
        return

    # -- tasks per second: one call beside the loop -------------------------------------------------
    tasks_tab = []
    for log2c in (12, 16, 20):
        nk_t = (1 << log2c) >> 8
        for B in (1, 16, 256, 4096):
            t_many, t_loop, k_ms = [], [], []
            got = loop = None
            for rep in range(args.reps + 1):
                # (The collector: tools/census_many_rate.py says why it runs here and only for large B.)
                got = loop = None
                if B >= 256:
                    gc.collect()
                nonces = fresh(B)
                tasks = [ScanTask(n, 3, 0, 0, 0, nk_t) for n in nonces]
                # Room for every hit, so that scan_many is one call: twice the expected number.  The
                # loop's pages are sized the same way, for one task (Miner.scan's default page is 2^16
                # entries, whose allocation alone would cost a small call more than the call).
                room_1 = max(1024, 2 * ((1 << log2c) >> 12))
                room = max(1024, 2 * B * ((1 << log2c) >> 12))
                t0 = time.perf_counter()
                got = miner.scan_many(tasks, max_hits=room)
                dm = time.perf_counter() - t0
                st = miner.last_scan_many_stats
                t0 = time.perf_counter()
                loop = [miner.scan(n, 3, 0, 0, 0, nk_t, max_hits=room_1) for n in nonces]
                dl = time.perf_counter() - t0
                assert got == loop
                if rep:  # (the first repetition is the warm-up)
                    t_many.append(dm)
                    t_loop.append(dl)
                    k_ms.append(st.kernel_ms)
            row = {"candidates_per_task": 1 << log2c, "B": B, "launches": st.launches,
                   "hits": sum(map(len, got)),
                   "many_call_ms": med(t_many) * 1e3, "many_kernel_ms": med(k_ms), "loop_ms": med(t_loop) * 1e3,
                   "many_tasks_per_s": B / med(t_many), "loop_tasks_per_s": B / med(t_loop),
                   "many_us_per_task": med(t_many) / B * 1e6, "loop_us_per_task": med(t_loop) / B * 1e6,
                   "many_over_loop": med(t_loop) / med(t_many)}
            tasks_tab.append(row)
            print(json.dumps({"tasks": row}), file=sys.stderr, flush=True)

    # -- where a dense call's time goes: N = 0 ------------------------------------------------------
    B, nk_t = 64, (1 << 12) >> 8
    w_many, k_many, w_loop, k_loop, launches_many = [], [], [], [], 0
    for rep in range(args.reps + 1):
        nonces = fresh(B)
        tasks = [ScanTask(n, 0, 0, 0, 0, nk_t) for n in nonces]
        gc.collect()
        t0 = time.perf_counter()
        got = miner.scan_batch(tasks, max_hits=B << 12)
        dm = time.perf_counter() - t0
        sm = miner.last_scan_many_stats
        assert sum(len(h) for _, h, _ in got) == B << 12 and all(r == distpow.EXHAUSTED for r, _, _ in got)
        launches_many = sm.launches
        got = None
        gc.collect()
        t0 = time.perf_counter()
        kl = 0.0
        for n in nonces:
            miner.scan_page(n, 0, 0, 0, 0, nk_t, max_hits=1 << 12)
            kl += miner.last_scan_stats.kernel_ms
        dl = time.perf_counter() - t0
        if rep:
            w_many.append(dm * 1e3)
            k_many.append(sm.kernel_ms)
            w_loop.append(dl * 1e3)
            k_loop.append(kl)
    dense = {"ntz": 0, "B": B, "candidates_per_task": 1 << 12, "hits": B << 12, "launches": launches_many,
             "many_kernel_ms": med(k_many), "many_call_ms": med(w_many),
             "host_and_python_ms": med(w_many) - med(k_many),
             "host_share": (med(w_many) - med(k_many)) / med(w_many),
             "loop_kernel_ms": med(k_loop), "loop_ms": med(w_loop), "many_over_loop": med(w_loop) / med(w_many)}
    print(json.dumps({"dense": dense}), file=sys.stderr, flush=True)

    out = {"tool": "tools/scan_many_rate.py", "reps": args.reps, "build_id": distpow.build_id(), "kernel_rate": rate,
           "tasks": tasks_tab, "dense": dense}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    miner.close()


if __name__ == "__main__":
    main()
