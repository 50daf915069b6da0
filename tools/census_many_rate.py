"""The batched census's measurements on one GPU.

  kernel_rate  one task over 2^28 k of the full partition through dpow_census_batch beside
               dpow_census_window on the same window (candidates over the launches' own ticks),
               alternating in one process
  tasks        fresh 4-byte nonces, B in {1, 16, 256, 4096} tasks of 2^12, 2^16 and 2^20 candidates:
               one Miner.census_many call beside Miner.census looped on the same context,
               alternating; tasks per second of each and their ratio
  where        B = 4096 tasks of 2^12 candidates: the call's kernel_ms and wall time beside the same
               2^24 candidates as one task through the same entry point
Medians of REPS repetitions after one warm-up of each shape; a host clock around calls that return
only when the answers are back.  Python's collector is run between the repetitions of B >= 256.

    python3 tools/census_many_rate.py [--reps 5] [--out profiles/census_many_rate.json] [--rate-log2k 28]
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
from distpow import CensusTask  # noqa: E402


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
    rnd = random.Random(16)

    def fresh(b):
        return [bytes(rnd.randrange(256) for _ in range(4)) for _ in range(b)]

    # -- the kernel's rate beside census_kernel's ---------------------------------------------------
    k0, nk = 1 << 24, 1 << args.rate_log2k
    miner.census(nonce, 0, 0, k0, k0 + (1 << 20))
    miner.census_many([CensusTask(nonce, 0, 0, k0, k0 + (1 << 20))])
    many_k, many_w, one_k, one_w = [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        (r, cm, k_done), = miner.census_batch([CensusTask(nonce, 0, 0, k0, k0 + nk)])
        many_w.append(nk * 256 / (time.perf_counter() - t0) / 1e9)
        st = miner.last_census_many_stats
        assert (r, k_done, st.candidates) == (distpow.EXHAUSTED, k0 + nk, nk * 256)
        many_k.append(st.candidates / (st.kernel_ms * 1e-3) / 1e9)
        launches = st.launches
        t0 = time.perf_counter()
        r, c1, k_done = miner.census_page(nonce, 0, 0, k0, k0 + nk)
        one_w.append(nk * 256 / (time.perf_counter() - t0) / 1e9)
        s1 = miner.last_census_stats
        assert (r, k_done, s1.candidates, s1.launches) == (distpow.EXHAUSTED, k0 + nk, nk * 256, launches)
        one_k.append(s1.candidates / (s1.kernel_ms * 1e-3) / 1e9)
        assert cm == c1
    rate = {"candidates": nk * 256, "launches": launches, "census_many_kernel_ghs": med(many_k),
            "census_many_wall_ghs": med(many_w), "census_kernel_ghs": med(one_k), "census_wall_ghs": med(one_w),
            "many_over_census_kernel": med(many_k) / med(one_k), "goal": 0.95,
            "census_many_kernel_ghs_all": many_k, "census_kernel_ghs_all": one_k}
    print(json.dumps({"kernel_rate": rate}), file=sys.stderr, flush=True)
    if args.kernel_rate_only:
        only = {"tool": "tools/census_many_rate.py", "reps": args.reps, "build_id": distpow.build_id(), "kernel_rate": rate}
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
                # The last repetition's 2 B result objects are dropped and collected first, so that the
                # collector's passes inside the timed calls do not walk them (at B = 4096 they cost a call
                # several times its own time).  Small calls are left alone: a collection right in front
                # of them costs them more, in cold caches, than any garbage does.
                got = loop = None
                if B >= 256:
                    gc.collect()
                nonces = fresh(B)
                tasks = [CensusTask(n, 0, 0, 0, nk_t) for n in nonces]
                t0 = time.perf_counter()
                got = miner.census_many(tasks)
                dm = time.perf_counter() - t0
                st = miner.last_census_many_stats
                t0 = time.perf_counter()
                loop = [miner.census(n, 0, 0, 0, nk_t) for n in nonces]
                dl = time.perf_counter() - t0
                assert got == loop
                if rep:  # (the first repetition is the warm-up)
                    t_many.append(dm)
                    t_loop.append(dl)
                    k_ms.append(st.kernel_ms)
            row = {"candidates_per_task": 1 << log2c, "B": B, "launches": st.launches,
                   "many_call_ms": med(t_many) * 1e3, "many_kernel_ms": med(k_ms), "loop_ms": med(t_loop) * 1e3,
                   "many_tasks_per_s": B / med(t_many), "loop_tasks_per_s": B / med(t_loop),
                   "many_us_per_task": med(t_many) / B * 1e6, "loop_us_per_task": med(t_loop) / B * 1e6,
                   "many_over_loop": med(t_loop) / med(t_many)}
            tasks_tab.append(row)
            print(json.dumps({"tasks": row}), file=sys.stderr, flush=True)

    # -- where a call's time goes: 4096 x 2^12 candidates beside 2^24 candidates as one task --------
    B, nk_t = 4096, (1 << 12) >> 8
    w_many, k_many, w_one, k_one = [], [], [], []
    for rep in range(args.reps + 1):
        tasks = [CensusTask(n, 0, 0, 0, nk_t) for n in fresh(B)]
        gc.collect()
        t0 = time.perf_counter()
        miner.census_batch(tasks)
        dm = time.perf_counter() - t0
        sm = miner.last_census_many_stats
        one = [CensusTask(fresh(1)[0], 0, 0, 0, B * nk_t)]
        t0 = time.perf_counter()
        miner.census_batch(one)
        do = time.perf_counter() - t0
        so = miner.last_census_many_stats
        assert sm.candidates == so.candidates == 1 << 24 and sm.launches == so.launches == 1
        if rep:
            w_many.append(dm * 1e3)
            k_many.append(sm.kernel_ms)
            w_one.append(do * 1e3)
            k_one.append(so.kernel_ms)
    where = {"candidates": 1 << 24, "B": B, "many_kernel_ms": med(k_many), "many_call_ms": med(w_many),
             "one_task_kernel_ms": med(k_one), "one_task_call_ms": med(w_one),
             "kernel_ms_difference": med(k_many) - med(k_one),
             "host_and_python_ms": med(w_many) - med(k_many),
             "tables_copied_bytes": B * 66 * 8}
    print(json.dumps({"where": where}), file=sys.stderr, flush=True)

    out = {"tool": "tools/census_many_rate.py", "reps": args.reps, "build_id": distpow.build_id(), "kernel_rate": rate,
           "tasks": tasks_tab, "where": where}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    miner.close()


if __name__ == "__main__":
    main()
