"""Tasks per second of the batched search against the two existing paths, on one GPU.

For N in {3, 4, 5, 6} and B in {1, 16, 64, 256, 1024} seeded fresh 4-byte nonces:
  (a) one Miner.mine_many call (dpow_search_batch),
  (b) the same tasks looped through Miner.mine on one context,
  (c) the same tasks spread over 8 threads with a context each (the existing concurrent path).
Every shape is warmed first; (a), (b) and (c) alternate in one process, REPS times; a host clock
around calls that return only when the answers are back.  The outputs of (a) are checked
against (b) at every size.  Also the generic kernel's plain rate: one N = 32 task over 2^28 k,
next to the specialised kernel's rate for the same window.

    python3 tools/batch_rate.py [--reps 5] [--out profiles/batch_rate.json] [--quick]
"""
import argparse
import json
import os
import random
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-proof-of-work_amd"))

import distpow  # noqa: E402
from distpow import BatchTask  # noqa: E402

THREADS = 8


def summary(times, n):
    rates = sorted(n / t for t in times)
    return {"median": statistics.median(rates), "min": rates[0], "max": rates[-1],
            "median_ms": statistics.median(times) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-rate-only", action="store_true",
                    help="the kernel-rate section alone (an A/B of two builds needs nothing else)")
    ap.add_argument("--quick", action="store_true", help="N in {3, 5}, B in {1, 64} only")
    ap.add_argument("--rate-log2k", type=int, default=28)
    args = ap.parse_args()
    ns = [3, 5] if args.quick else [3, 4, 5, 6]
    bs = [1, 64] if args.quick else [1, 16, 64, 256, 1024]
    if args.kernel_rate_only:
        ns = []
    miner = distpow.Miner(0)
    pool = [distpow.Miner(0) for _ in range(0 if args.kernel_rate_only else THREADS)]

    def run_a(reqs):
        t0 = time.perf_counter()
        res = miner.mine_many(reqs)
        return time.perf_counter() - t0, [(r.status, r.global_idx, r.secret) for r in res]

    def run_b(reqs):
        t0 = time.perf_counter()
        res = [miner.mine(r.nonce, r.num_trailing_zeros) for r in reqs]
        return time.perf_counter() - t0, [(r.status, r.global_idx, r.secret) for r in res]

    def run_c(reqs):
        out = [None] * len(reqs)

        def work(w):
            for i in range(w, len(reqs), THREADS):
                r = pool[w].mine(reqs[i].nonce, reqs[i].num_trailing_zeros)
                out[i] = (r.status, r.global_idx, r.secret)

        ths = [threading.Thread(target=work, args=(w,)) for w in range(min(THREADS, len(reqs)))]
        t0 = time.perf_counter()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        return time.perf_counter() - t0, out

    table = []
    for n in ns:
        for b in bs:
            rnd = random.Random(1000 * n + b)
            reqs = [BatchTask(bytes(rnd.randrange(256) for _ in range(4)), n) for _ in range(b)]
            for f in (run_a, run_b, run_c):  # warm the shape
                f(reqs)
            times = {"a": [], "b": [], "c": []}
            match = True
            rounds = []
            for _ in range(args.reps):
                ta, ra = run_a(reqs)
                rounds.append(miner.last_batch_stats.rounds)
                tb, rb = run_b(reqs)
                tc, rc = run_c(reqs)
                match = match and ra == rb == rc and all(r[0] == distpow.FOUND for r in ra)
                times["a"].append(ta)
                times["b"].append(tb)
                times["c"].append(tc)
            row = {"ntz": n, "tasks": b, "outputs_match": match, "batch_rounds": rounds[-1],
                   "batch": summary(times["a"], b), "looped": summary(times["b"], b),
                   "threads8": summary(times["c"], b)}
            row["batch_over_looped"] = row["batch"]["median"] / row["looped"]["median"]
            row["batch_over_threads8"] = row["batch"]["median"] / row["threads8"]["median"]
            table.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)

    # the generic kernel's plain rate next to the specialised kernel's, same window
    k0, nk = 1 << 24, 1 << args.rate_log2k
    task = BatchTask([1, 2, 3, 4], 32, 0, 0, k0, k0 + nk)
    miner.search_batch([BatchTask([1, 2, 3, 4], 32, 0, 0, k0, k0 + (1 << 16))])
    miner.search([1, 2, 3, 4], 32, 0, 0, k0, k0 + (1 << 16))
    t0 = time.perf_counter()
    r = miner.search_batch([task])[0]
    t_batch = time.perf_counter() - t0
    st = miner.last_batch_stats
    miner.reset_stats()
    t0 = time.perf_counter()
    r2 = miner.search([1, 2, 3, 4], 32, 0, 0, k0, k0 + nk)
    t_search = time.perf_counter() - t0
    s2 = miner.stats()
    rate = {"candidates": nk * 256, "statuses": [r.status, r2.status],
            "batch_wall_ghs": nk * 256 / t_batch / 1e9, "batch_kernel_ghs": st.candidates / (st.kernel_ms * 1e-3) / 1e9,
            "batch_launches": st.launches,
            "search_wall_ghs": nk * 256 / t_search / 1e9,
            "search_kernel_ghs": s2.candidates / (s2.kernel_ms * 1e-3) / 1e9}
    out = {"tool": "tools/batch_rate.py", "reps": args.reps, "threads": THREADS, "build_id": distpow.build_id(),
           "table": table, "kernel_rate": rate}
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"rows": len(table), "all_match": all(r["outputs_match"] for r in table),
                      "kernel_rate": rate}))
    for m in [miner] + pool:
        m.close()


if __name__ == "__main__":
    main()
