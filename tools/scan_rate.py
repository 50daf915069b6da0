"""The scan's measurements on one GPU.

  scan_rate   the scan kernel's GH/s on one N = 32 window of 2^28 k, next to batch_kernel on the same
              window (tools/batch_rate.py's kernel_rate method: candidates over the launches' own
              ticks), alternating in one process
  walk        one fixture window's N >= 8 hits (tests/golden/layout_deep_hits.json, len04) listed by a
              Miner.search loop that resumes behind each hit (tools/layout_hints.py's walk), and the
              same list from one scan
  dense       N = 0 over 2^20 candidates: kernel time and host time (sort + verify) of one dpow_scan call
Medians of REPS repetitions after one warm-up of each shape; a host clock around calls that return
only when the answers are back.

    python3 tools/scan_rate.py [--reps 5] [--out profiles/scan_rate.json] [--rate-log2k 28]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-proof-of-work_amd"))

import distpow  # noqa: E402
from distpow import BatchTask, _lib  # noqa: E402


def med(xs):
    return statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rate-log2k", type=int, default=28)
    args = ap.parse_args()
    miner = distpow.Miner(0)
    nonce = [1, 2, 3, 4]

    # -- the kernel's plain rate beside batch_kernel's --------------------------------------------
    k0, nk = 1 << 24, 1 << args.rate_log2k
    miner.scan(nonce, 32, 0, 0, k0, k0 + (1 << 20))
    miner.search_batch([BatchTask(nonce, 32, 0, 0, k0, k0 + (1 << 20))])
    scan_k, scan_w, batch_k, batch_w, launches = [], [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r, hits, k_done = miner.scan_page(nonce, 32, 0, 0, k0, k0 + nk)
        scan_w.append(nk * 256 / (time.perf_counter() - t0) / 1e9)
        st = miner.last_scan_stats
        assert (r, hits, k_done) == (distpow.EXHAUSTED, [], k0 + nk) and st.candidates == nk * 256
        scan_k.append(st.candidates / (st.kernel_ms * 1e-3) / 1e9)
        launches.append(st.launches)
        t0 = time.perf_counter()
        res = miner.search_batch([BatchTask(nonce, 32, 0, 0, k0, k0 + nk)])[0]
        batch_w.append(nk * 256 / (time.perf_counter() - t0) / 1e9)
        sb = miner.last_batch_stats
        assert res.status == distpow.EXHAUSTED
        batch_k.append(sb.candidates / (sb.kernel_ms * 1e-3) / 1e9)
    rate = {"candidates": nk * 256, "scan_kernel_ghs": med(scan_k), "scan_wall_ghs": med(scan_w),
            "scan_launches": launches[-1], "batch_kernel_ghs": med(batch_k), "batch_wall_ghs": med(batch_w),
            "scan_over_batch_kernel": med(scan_k) / med(batch_k),
            "scan_kernel_ghs_all": scan_k, "batch_kernel_ghs_all": batch_k}
    print(json.dumps({"scan_rate": rate}), file=sys.stderr, flush=True)

    # -- walk against scan ----------------------------------------------------------------------
    with open(os.path.join(ROOT, "tests", "golden", "layout_deep_hits.json")) as f:
        case = next(c for c in json.load(f)["cases"] if c["name"] == "len04")
    want = [g for g, _ in case["hits"]]

    def walk():
        hits, k = [], case["k_begin"]
        while k < case["k_end"]:
            r = miner.search(case["nonce"], 8, 0, 0, k, case["k_end"])
            if r.status != distpow.FOUND:
                break
            hits.append(r.global_idx)
            k = (r.global_idx >> 8) + 1
        return hits

    def scan():
        return [h.global_idx for h in miner.scan(case["nonce"], 8, 0, 0, case["k_begin"], case["k_end"])]

    assert walk() == want and scan() == want   # (no fixture window has two hits in one k)
    t_walk, t_scan = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        walk()
        t_walk.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        scan()
        t_scan.append(time.perf_counter() - t0)
    walk_row = {"case": "len04", "candidates": (case["k_end"] - case["k_begin"]) * 256, "hits": len(want),
                "walk_ms": med(t_walk) * 1e3, "walk_searches": len(want) + 1, "scan_ms": med(t_scan) * 1e3,
                "scan_launches": miner.last_scan_stats.launches}
    print(json.dumps({"walk": walk_row}), file=sys.stderr, flush=True)

    # -- dense cost ---------------------------------------------------------------------------------
    n_cand = 1 << 20
    arr = (_lib.ScanHitC * n_cand)()
    cnt, kd, st = ctypes.c_size_t(), ctypes.c_uint64(), _lib.BatchStats()
    nb = bytes(nonce)
    wall, kern = [], []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        rc = distpow.lib().dpow_scan(miner._ctx, nb, len(nb), 0, 0, 0, 0, n_cand >> 8, arr, n_cand, ctypes.byref(cnt),
                                     ctypes.byref(kd), ctypes.byref(st))
        dt = time.perf_counter() - t0
        assert rc == distpow.EXHAUSTED and cnt.value == n_cand and arr[n_cand - 1].global_idx == n_cand - 1
        if rep:
            wall.append(dt * 1e3)
            kern.append(st.kernel_ms)
    dense = {"candidates": n_cand, "launches": st.launches, "call_ms": med(wall), "kernel_ms": med(kern),
             "host_ms": med(wall) - med(kern), "host_ns_per_hit": (med(wall) - med(kern)) * 1e6 / n_cand}
    print(json.dumps({"dense": dense}), file=sys.stderr, flush=True)

    out = {"tool": "tools/scan_rate.py", "reps": args.reps, "build_id": distpow.build_id(), "scan_rate": rate,
           "walk": walk_row, "dense": dense}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    miner.close()


if __name__ == "__main__":
    main()
