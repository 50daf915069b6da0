"""The task queue's rates and latencies on one GPU (distpow.TaskQueue).

  M1  tasks per second: B in {1, 16, 64, 256, 1024} fresh 4-byte nonces at N = 3, window k < 2^16,
      (a) submitted to a queue one by one and collected, (b) as one Miner.search_batch call;
      answers compared.  And one N = 32 task over 2^32 candidates through each kernel: launches
      of 16384 workgroups that read a descriptor each from pinned memory (queue_kernel) against
      workgroups that compute their range (batch_kernel), kernel time as the launches stamp it.
  M2  fresh N = 2 tasks beside one old task (N = 32, never decided), one submitted every 100 us
      whatever the answers do, so that every launch holds fresh tasks: their submit-to-decided
      time and the old task's hash rate, per value of the planner's spread
      (DPOW_DIAG_QUEUE_SPREAD).
  M3  the known limit: the same with one fresh task at a time, each submitted after the previous
      answer, so that it arrives while an old-task-only launch is in flight.

    python3 tools/queue_rate.py [--reps 5] [--out profiles/queue_rate.json] [--quick]
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
from distpow import BatchTask, TaskQueue  # noqa: E402

WAIT_MS = 20000


def nonces(rnd, n, length=4):
    return [bytes(rnd.randrange(256) for _ in range(length)) for _ in range(n)]


def collect(q, n):
    out = {}
    for _ in range(n):
        r = q.next(WAIT_MS)
        if r is None:
            raise RuntimeError("queue_rate: time-out waiting for a result")
        out[r.ticket] = r
    return out


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(p * len(xs)))]


def m1(miner, reps, bs):
    rnd = random.Random(20251020)
    rows = []
    with TaskQueue(0) as q:
        for b in bs:
            tq, tb = [], []
            for rep in range(reps + 1):   # the first pass warms the shape
                tasks = [BatchTask(n, 3, k_end=1 << 16) for n in nonces(rnd, b)]
                t0 = time.perf_counter()
                tickets = [q.submit(t) for t in tasks]
                got = collect(q, b)
                t1 = time.perf_counter()
                res = miner.search_batch(tasks)
                t2 = time.perf_counter()
                for ticket, r in zip(tickets, res):
                    a = got[ticket].result
                    if (a.status, a.global_idx, a.secret) != (r.status, r.global_idx, r.secret):
                        raise RuntimeError(f"queue_rate: queue and batch differ: {a} {r}")
                if rep:
                    tq.append(t1 - t0)
                    tb.append(t2 - t1)
            rows.append({"n": 3, "b": b, "queue_tasks_per_s": b / statistics.median(tq),
                         "batch_tasks_per_s": b / statistics.median(tb),
                         "queue_ms": statistics.median(tq) * 1e3, "batch_ms": statistics.median(tb) * 1e3})
            print(rows[-1], file=sys.stderr, flush=True)
    return rows


def m1_descriptors(miner, reps):
    """One N = 32 task over 2^32 candidates through each kernel.  Past its first rounds a launch is
    2^28 candidates either way: 16384 workgroups that each read a descriptor from pinned memory
    (queue_kernel), or that compute their range from one map entry (batch_kernel)."""
    task = BatchTask([7, 7, 7, 7], 32, 0, 0, 1 << 24, (1 << 24) + (1 << 24))
    rows = []
    for rep in range(reps + 1):
        with TaskQueue(0) as q:
            r = q.wait(q.submit(task), WAIT_MS)
            if r is None or r.status != distpow.EXHAUSTED:
                raise RuntimeError(f"queue_rate: {r}")
            st = q.stats()[0]
            qrow = {"launches": st.launches, "candidates": st.candidates, "kernel_ms": st.kernel_ms}
        miner.search_batch([task])
        st = miner.last_batch_stats
        brow = {"launches": st.launches, "candidates": st.candidates, "kernel_ms": st.kernel_ms}
        if rep:
            rows.append({"queue": qrow, "batch": brow,
                         "queue_ghs": qrow["candidates"] / qrow["kernel_ms"] * 1e-6,
                         "batch_ghs": brow["candidates"] / brow["kernel_ms"] * 1e-6})
            print(rows[-1], file=sys.stderr, flush=True)
    return rows


def open_loop(spread, period_us, n_fresh):
    """M2: arrivals on a clock of their own."""
    os.environ["DPOW_DIAG_QUEUE_SPREAD"] = str(spread)
    rnd = random.Random(20251023 + spread)
    try:
        with TaskQueue(0) as q:
            old = q.submit(BatchTask([9, 9, 9, 9], 32, 0, 0, 1 << 24, (1 << 24) + (1 << 40)))
            time.sleep(0.02)   # the old task reaches the cap
            fresh = [BatchTask(n, 2, k_end=64) for n in nonces(rnd, n_fresh)]
            s0, t0 = q.stats()[0], time.perf_counter()
            c0, l0 = s0.candidates, s0.launches

            def submitter():
                for i, t in enumerate(fresh):
                    while time.perf_counter() < t0 + i * period_us * 1e-6:
                        pass
                    q.submit(t)

            th = threading.Thread(target=submitter)
            th.start()
            lat, launches = [], []
            for _ in range(n_fresh):
                r = q.next(WAIT_MS)
                if r is None:
                    raise RuntimeError("queue_rate: time-out")
                lat.append(r.queued_ms)
                launches.append(r.launches)
            th.join()
            s1, t1 = q.stats()[0], time.perf_counter()
            q.cancel(old)
            return {"spread": spread, "period_us": period_us, "fresh": n_fresh,
                    "fresh_ms_median": statistics.median(lat), "fresh_ms_p90": pct(lat, 0.9), "fresh_ms_max": max(lat),
                    "fresh_launches_max": max(launches), "launches": s1.launches - l0,
                    "launch_ms_mean": (t1 - t0) * 1e3 / max(s1.launches - l0, 1),
                    "candidates_per_s": (s1.candidates - c0) / (t1 - t0)}
    finally:
        os.environ.pop("DPOW_DIAG_QUEUE_SPREAD", None)


def beside_old(spread, depth, n_fresh):
    os.environ["DPOW_DIAG_QUEUE_SPREAD"] = str(spread)
    rnd = random.Random(20251022 + spread)
    try:
        with TaskQueue(0) as q:
            old = q.submit(BatchTask([9, 9, 9, 9], 32, 0, 0, 1 << 24, (1 << 24) + (1 << 40)))
            time.sleep(0.02)   # the old task reaches the cap
            s0, t0 = q.stats()[0], time.perf_counter()
            c0, l0 = s0.candidates, s0.launches
            lat = []
            fresh = [BatchTask(n, 2, k_end=64) for n in nonces(rnd, n_fresh)]
            it = iter(fresh)
            in_flight = 0
            for _ in range(depth):
                q.submit(next(it))
                in_flight += 1
            while in_flight:
                r = q.next(WAIT_MS)
                if r is None:
                    raise RuntimeError("queue_rate: time-out")
                in_flight -= 1
                lat.append(r.queued_ms)
                if r.launches != 1:
                    raise RuntimeError(f"queue_rate: a fresh task took {r.launches} launches")
                t = next(it, None)
                if t is not None:
                    q.submit(t)
                    in_flight += 1
            s1, t1 = q.stats()[0], time.perf_counter()
            q.cancel(old)
            return {"spread": spread, "depth": depth, "fresh": n_fresh,
                    "fresh_ms_median": statistics.median(lat), "fresh_ms_p90": pct(lat, 0.9), "fresh_ms_max": max(lat),
                    "fresh_tasks_per_s": n_fresh / (t1 - t0),
                    "launches": s1.launches - l0,
                    "candidates_per_s": (s1.candidates - c0) / (t1 - t0)}
    finally:
        os.environ.pop("DPOW_DIAG_QUEUE_SPREAD", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-rate-only", action="store_true",
                    help="M1's descriptor launch alone (an A/B of two builds needs nothing else)")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    bs = [1, 64] if args.quick else [1, 16, 64, 256, 1024]
    spreads = [16] if args.quick else [1, 4, 16, 64, 256]
    n_fresh = 100 if args.quick else 400
    out = {"tool": "tools/queue_rate.py", "build_id": distpow.build_id(), "reps": args.reps}
    with distpow.Miner(0) as miner:
        if not args.kernel_rate_only:
            out["m1_tasks_per_s"] = m1(miner, args.reps, bs)
        out["m1_descriptor_launch"] = m1_descriptors(miner, min(args.reps, 3))
    if args.kernel_rate_only:
        spreads = []
    out["m2_fresh_beside_old"] = []
    out["m3_fresh_after_previous_answer"] = []
    for s in spreads:
        out["m2_fresh_beside_old"].append(open_loop(s, 100, n_fresh))
        print(out["m2_fresh_beside_old"][-1], file=sys.stderr, flush=True)
    for s in spreads:
        out["m3_fresh_after_previous_answer"].append(beside_old(s, 1, n_fresh // 2))
        print(out["m3_fresh_after_previous_answer"][-1], file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
