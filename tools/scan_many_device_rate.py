"""The batched device scan's measurements on one GPU.

  mask_rate   scan_many_mask_kernel's GH/s on one N = 32 task of 2^36 candidates next to
              scan_many_kernel's on the same task (candidates over the launches' own ticks)
  fresh       one call of 256 fresh nonces at N = 3 over 2^12, 2^16 and 2^20 candidates each
              (Miner.scan_many_cuda) beside Miner.scan_many and beside Miner.scan_cuda in a loop
  dense       N = 0, 64 tasks of 2^12 candidates (262144 hits) beside Miner.scan_batch
  host        the call's host time (the call minus its kernel time) against the number of hits (16
              tasks at N = 0) and against the number of tasks (2^12 candidates each at N = 3)
Medians of REPS repetitions after one warm-up of each shape, the sides alternating in one process; a
host clock around calls that return only when the answers are complete.

    python3 tools/scan_many_device_rate.py [--reps 5] [--out profiles/scan_many_device_rate.json] [--rate-log2k 28]
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
    rnd = random.Random(20)

    def fresh(b):
        return [bytes(rnd.randrange(256) for _ in range(4)) for _ in range(b)]

    def device_call(tasks, room, want_depths=True):
        """One dpow_scan_batch_device call: (ms, hits, stats)."""
        t0 = time.perf_counter()
        res, idx, dep, rows = miner.scan_batch_cuda(tasks, room, want_depths)
        dt = (time.perf_counter() - t0) * 1e3
        assert all(r == distpow.EXHAUSTED for r, _ in res)
        return dt, idx.numel(), miner.last_scan_many_device_stats

    # -- the mask kernel's plain rate beside scan_many_kernel's -------------------------------------
    k0, nk = 1 << 24, 1 << args.rate_log2k
    device_call([ScanTask(nonce, 32, 0, 0, k0, k0 + (1 << 20))], 1 << 14)
    miner.scan_many([ScanTask(nonce, 32, 0, 0, k0, k0 + (1 << 20))])
    mask_k, mask_w, many_k, many_w = [], [], [], []
    for _ in range(args.reps):
        dt, n, st = device_call([ScanTask(nonce, 32, 0, 0, k0, k0 + nk)], 1 << 14)
        assert n == 0 and st.candidates == nk * 256
        mask_w.append(nk * 256 / (dt * 1e-3) / 1e9)
        mask_k.append(st.candidates / (st.kernel_ms * 1e-3) / 1e9)
        mask_launches = st.rounds
        t0 = time.perf_counter()
        (r, hits, k_done), = miner.scan_batch([ScanTask(nonce, 32, 0, 0, k0, k0 + nk)])
        many_w.append(nk * 256 / (time.perf_counter() - t0) / 1e9)
        sm = miner.last_scan_many_stats
        assert (r, hits, k_done, sm.candidates) == (distpow.EXHAUSTED, [], k0 + nk, nk * 256)
        many_k.append(sm.candidates / (sm.kernel_ms * 1e-3) / 1e9)
    rate = {"candidates": nk * 256, "mask_kernel_ghs": med(mask_k), "mask_wall_ghs": med(mask_w),
            "mask_launches": mask_launches, "scan_many_kernel_ghs": med(many_k), "scan_many_wall_ghs": med(many_w),
            "scan_many_launches": sm.launches, "mask_over_scan_many_kernel": med(mask_k) / med(many_k),
            "mask_kernel_ghs_all": mask_k, "scan_many_kernel_ghs_all": many_k}
    print(json.dumps({"mask_rate": rate}), file=sys.stderr, flush=True)
    if args.kernel_rate_only:
        only = {"tool": "tools/scan_many_device_rate.py", "reps": args.reps, "build_id": distpow.build_id(),
                "mask_rate": rate}
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(only, indent=1) + "\n")
        print(json.dumps(only))
        miner.close()
        return

    # -- 256 fresh nonces at N = 3: one call beside scan_many and beside scan_cuda in a loop ----------
    fresh_tab = []
    B = 256
    for log2c in (12, 16, 20):
        nk_t = (1 << log2c) >> 8
        room = max(1 << 14, 2 * B * ((1 << log2c) >> 12))
        room_1 = max(1 << 14, 2 * ((1 << log2c) >> 12))
        t_dev, t_many, t_loop, k_dev, k_many = [], [], [], [], []
        for rep in range(args.reps + 1):
            gc.collect()
            nonces = fresh(B)
            tasks = [ScanTask(n, 3, 0, 0, 0, nk_t) for n in nonces]
            t0 = time.perf_counter()
            idx, dep, rows = miner.scan_many_cuda(tasks, room)
            dd = time.perf_counter() - t0
            sd = miner.last_scan_many_device_stats
            t0 = time.perf_counter()
            got = miner.scan_many(tasks, max_hits=room)
            dm = time.perf_counter() - t0
            sm = miner.last_scan_many_stats
            t0 = time.perf_counter()
            loop = [miner.scan_cuda(n, 3, 0, 0, 0, nk_t, room_1) for n in nonces]
            dl = time.perf_counter() - t0
            assert idx.numel() == sum(map(len, got)) == sum(i.numel() for i, _ in loop)
            hits = idx.numel()
            got = loop = None
            if rep:  # (the first repetition is the warm-up)
                t_dev.append(dd * 1e3)
                t_many.append(dm * 1e3)
                t_loop.append(dl * 1e3)
                k_dev.append(sd.kernel_ms)
                k_many.append(sm.kernel_ms)
        row = {"candidates_per_task": 1 << log2c, "B": B, "hits": hits, "device_call_ms": med(t_dev),
               "device_kernel_ms": med(k_dev), "device_launches": sd.launches, "device_mask_launches": sd.rounds,
               "scan_many_ms": med(t_many), "scan_many_kernel_ms": med(k_many), "scan_cuda_loop_ms": med(t_loop),
               "scan_many_over_device": med(t_many) / med(t_dev), "loop_over_device": med(t_loop) / med(t_dev)}
        fresh_tab.append(row)
        print(json.dumps({"fresh": row}), file=sys.stderr, flush=True)

    # -- the dense call: N = 0, 262144 hits ------------------------------------------------------------
    B, nk_t = 64, (1 << 12) >> 8
    w_dev, k_dev, w_many, k_many = [], [], [], []
    for rep in range(args.reps + 1):
        nonces = fresh(B)
        tasks = [ScanTask(n, 0, 0, 0, 0, nk_t) for n in nonces]
        gc.collect()
        dt, n, sd = device_call(tasks, B << 12)
        assert n == B << 12
        t0 = time.perf_counter()
        got = miner.scan_batch(tasks, max_hits=B << 12)
        dm = (time.perf_counter() - t0) * 1e3
        sm = miner.last_scan_many_stats
        assert sum(len(h) for _, h, _ in got) == B << 12
        got = None
        if rep:
            w_dev.append(dt)
            k_dev.append(sd.kernel_ms)
            w_many.append(dm)
            k_many.append(sm.kernel_ms)
    dense = {"ntz": 0, "B": B, "candidates_per_task": 1 << 12, "hits": B << 12, "device_call_ms": med(w_dev),
             "device_kernel_ms": med(k_dev), "device_launches": sd.launches, "device_host_ms": med(w_dev) - med(k_dev),
             "scan_many_call_ms": med(w_many), "scan_many_kernel_ms": med(k_many),
             "scan_many_over_device": med(w_many) / med(w_dev)}
    print(json.dumps({"dense": dense}), file=sys.stderr, flush=True)

    # -- host time against hits and against tasks ---------------------------------------------------
    def host_row(tasks, room, label):
        rows = []
        for rep in range(args.reps + 1):
            gc.collect()
            r = device_call(tasks, room)
            if rep:
                rows.append(r)
        call, kern = med([r[0] for r in rows]), med([r[2].kernel_ms for r in rows])
        out = dict(label, hits=rows[0][1], launches=rows[0][2].launches, call_ms=call, kernel_ms=kern,
                   host_ms=call - kern)
        print(json.dumps({"host": out}), file=sys.stderr, flush=True)
        return out

    by_hits = [host_row([ScanTask(n, 0, 0, 0, 0, (1 << log2n) >> 12) for n in fresh(16)], 1 << log2n,
                        {"tasks": 16, "ntz": 0, "candidates": 1 << log2n}) for log2n in (14, 16, 20, 24)]
    by_tasks = [host_row([ScanTask(n, 3, 0, 0, 0, 16) for n in fresh(b)], 1 << 14,
                         {"tasks": b, "ntz": 3, "candidates": b << 12}) for b in (1, 16, 256, 4096)]

    out = {"tool": "tools/scan_many_device_rate.py", "reps": args.reps, "build_id": distpow.build_id(),
           "mask_rate": rate, "fresh": fresh_tab, "dense": dense, "host_by_hits": by_hits, "host_by_tasks": by_tasks}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    miner.close()


if __name__ == "__main__":
    main()
