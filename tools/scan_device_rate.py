"""The device scan's measurements on one GPU.

  mask_rate   scan_mask_kernel's GH/s on one N = 32 window of 2^36 candidates next to scan_kernel's on
              the same window (candidates over the launches' own ticks), alternating in one process
  place       the place launch's and the depth launches' time beside the mask launch's, on a sparse
              slice (N = 8, 2^28 candidates) and on a dense one (N = 0, 2^24 candidates)
  dense       N = 0 over 2^16, 2^20 and 2^24 candidates through Miner.scan_cuda beside Miner.scan: the
              call, its kernel time, and the host time (the call minus kernel_ms) per launch
  sparse      the len04 fixture window (tests/golden/layout_deep_hits.json) at N = 8 beside Miner.scan
  n3          N = 3 over 2^30 candidates beside Miner.scan, whose list binds it to 2^26-candidate slices
Medians of REPS repetitions after one warm-up of each shape, both sides alternating in one process;
a host clock around calls that return only when the answers are complete.

    python3 tools/scan_device_rate.py [--reps 5] [--out profiles/scan_device_rate.json] [--rate-log2k 28]
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
from distpow import _lib  # noqa: E402


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

    with open(os.path.join(ROOT, "tests", "golden", "layout_deep_hits.json")) as f:
        case = next(c for c in json.load(f)["cases"] if c["name"] == "len04")

    def device_call(ntz, k0, k1, max_hits, want_depths=True, nonce=nonce):
        """One dpow_scan_device call: (ms, hits, stats, (mask, place, depth) ms)."""
        t0 = time.perf_counter()
        r, idx, dep, k_done = miner.scan_cuda_page(nonce, ntz, 0, 0, k0, k1, max_hits, want_depths)
        dt = (time.perf_counter() - t0) * 1e3
        assert (r, k_done) == (distpow.EXHAUSTED, k1)
        return dt, idx.numel(), miner.last_scan_device_stats, miner.scan_device_times()

    page = (_lib.ScanHitC * (1 << 20))()
    nb = bytes(nonce)

    def host_call(ntz, k0, k1):
        """Miner.scan's calls (dpow_scan, paged over MORE) without its Python objects: (ms, hits, stats)."""
        cnt, kd, st, total = ctypes.c_size_t(), ctypes.c_uint64(k0), _lib.BatchStats(), _lib.BatchStats()
        hits, r = 0, distpow.MORE
        t0 = time.perf_counter()
        while r == distpow.MORE:
            r = _lib.check(distpow.lib().dpow_scan(miner._ctx, nb, len(nb), ntz, 0, 0, kd.value, k1, page, len(page),
                                                   ctypes.byref(cnt), ctypes.byref(kd), ctypes.byref(st)), "dpow_scan")
            hits += cnt.value
            total.launches += st.launches
            total.kernel_ms += st.kernel_ms
        dt = (time.perf_counter() - t0) * 1e3
        assert r == distpow.EXHAUSTED and kd.value == k1
        return dt, hits, total

    # -- the mask kernel's plain rate beside scan_kernel's ------------------------------------------
    k0, nk = 1 << 24, 1 << args.rate_log2k
    device_call(32, k0, k0 + (1 << 20), 1 << 14)
    host_call(32, k0, k0 + (1 << 20))
    mask_k, mask_w, scan_k, scan_w = [], [], [], []
    for _ in range(args.reps):
        dt, n, st, _ = device_call(32, k0, k0 + nk, 1 << 14)
        assert n == 0 and st.candidates == nk * 256 and st.launches == st.rounds
        mask_w.append(nk * 256 / (dt * 1e-3) / 1e9)
        mask_k.append(st.candidates / (st.kernel_ms * 1e-3) / 1e9)
        mask_launches = st.rounds
        t0 = time.perf_counter()
        r, hits, k_done = miner.scan_page(nonce, 32, 0, 0, k0, k0 + nk)
        scan_w.append(nk * 256 / (time.perf_counter() - t0) / 1e9)
        ss = miner.last_scan_stats
        assert (r, hits, k_done) == (distpow.EXHAUSTED, [], k0 + nk) and ss.candidates == nk * 256
        scan_k.append(ss.candidates / (ss.kernel_ms * 1e-3) / 1e9)
    rate = {"candidates": nk * 256, "mask_kernel_ghs": med(mask_k), "mask_wall_ghs": med(mask_w),
            "mask_launches": mask_launches, "scan_kernel_ghs": med(scan_k), "scan_wall_ghs": med(scan_w),
            "scan_launches": ss.launches, "mask_over_scan_kernel": med(mask_k) / med(scan_k),
            "mask_kernel_ghs_all": mask_k, "scan_kernel_ghs_all": scan_k}
    print(json.dumps({"mask_rate": rate}), file=sys.stderr, flush=True)
    if args.kernel_rate_only:
        only = {"tool": "tools/scan_device_rate.py", "reps": args.reps, "build_id": distpow.build_id(), "mask_rate": rate}
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(only, indent=1) + "\n")
        print(json.dumps(only))
        miner.close()
        return

    # -- the place launch beside the mask launch -----------------------------------------------------
    # (the sparse slice: 2^28 candidates of the len04 fixture's window around its one N >= 8 hit)
    k_hit = next(g for g, tz in case["hits"] if tz >= 8) >> 8
    assert case["k_begin"] <= k_hit - (1 << 19) and k_hit + (1 << 19) <= case["k_end"]
    place = []
    for name, ntz, a, b, room, nc in (("sparse", 8, k_hit - (1 << 19), k_hit + (1 << 19), 1 << 14, case["nonce"]),
                                      ("dense", 0, 0, 1 << 16, 1 << 24, nonce)):
        device_call(ntz, a, b, room, nonce=nc)
        rows = [device_call(ntz, a, b, room, nonce=nc) for _ in range(args.reps)]
        assert rows[0][1] == (1 if name == "sparse" else 1 << 24)
        place.append({"slice": name, "ntz": ntz, "candidates": (b - a) * 256, "hits": rows[0][1],
                      "launches": rows[0][2].launches, "mask_ms": med([r[3][0] for r in rows]),
                      "place_ms": med([r[3][1] for r in rows]), "depth_ms": med([r[3][2] for r in rows]),
                      "call_ms": med([r[0] for r in rows])})
    print(json.dumps({"place": place}), file=sys.stderr, flush=True)

    # -- dense calls: host time against the number of hits -----------------------------------------
    dense = []
    for log2n in (16, 20, 24):
        n_cand = 1 << log2n
        k1 = n_cand >> 8
        device_call(0, 0, k1, n_cand)
        with_host = log2n <= 20
        if with_host:
            host_call(0, 0, k1)
        dev, host = [], []
        for _ in range(args.reps):
            dev.append(device_call(0, 0, k1, n_cand))
            assert dev[-1][1] == n_cand
            if with_host:
                host.append(host_call(0, 0, k1))
                assert host[-1][1] == n_cand
        if not with_host:   # one call: seconds of host work
            host.append(host_call(0, 0, k1))
        launches = dev[0][2].launches
        call, kern = med([r[0] for r in dev]), med([r[2].kernel_ms for r in dev])
        dense.append({"candidates": n_cand, "device_call_ms": call, "device_kernel_ms": kern,
                      "device_launches": launches, "device_slices": dev[0][2].rounds,
                      "device_host_ms": call - kern, "device_host_us_per_launch": (call - kern) * 1e3 / launches,
                      "scan_call_ms": med([r[0] for r in host]), "scan_kernel_ms": med([r[2].kernel_ms for r in host]),
                      "scan_launches": host[0][2].launches, "scan_reps": len(host)})
    print(json.dumps({"dense": dense}), file=sys.stderr, flush=True)

    # -- a sparse window ------------------------------------------------------------------------------
    want = [g for g, tz in case["hits"] if tz >= 8]

    def sparse_device():
        t0 = time.perf_counter()
        idx, dep = miner.scan_cuda(case["nonce"], 8, 0, 0, case["k_begin"], case["k_end"], 1 << 14)
        return (time.perf_counter() - t0) * 1e3, idx.tolist(), miner.last_scan_device_stats

    def sparse_host():
        t0 = time.perf_counter()
        hits = miner.scan(case["nonce"], 8, 0, 0, case["k_begin"], case["k_end"])
        return (time.perf_counter() - t0) * 1e3, [h.global_idx for h in hits], miner.last_scan_stats

    assert sparse_device()[1] == want and sparse_host()[1] == want
    sd, sh = [], []
    for _ in range(args.reps):
        sd.append(sparse_device())
        sh.append(sparse_host())
    sparse = {"case": "len04", "candidates": (case["k_end"] - case["k_begin"]) * 256, "hits": len(want),
              "device_ms": med([r[0] for r in sd]), "device_kernel_ms": med([r[2].kernel_ms for r in sd]),
              "device_launches": sd[0][2].launches, "device_slices": sd[0][2].rounds,
              "scan_ms": med([r[0] for r in sh]), "scan_kernel_ms": med([r[2].kernel_ms for r in sh]),
              "scan_launches": sh[0][2].launches}
    print(json.dumps({"sparse": sparse}), file=sys.stderr, flush=True)

    # -- N = 3: 2^28 slices against the list-bound 2^26 ---------------------------------------------
    a, b = k0, k0 + (1 << 22)
    device_call(3, a, b, 1 << 20)
    host_call(3, a, b)
    nd, nh = [], []
    for _ in range(args.reps):
        nd.append(device_call(3, a, b, 1 << 20))
        nh.append(host_call(3, a, b))
        assert nd[-1][1] == nh[-1][1]
    n3 = {"candidates": (b - a) * 256, "hits": nd[0][1], "device_ms": med([r[0] for r in nd]),
          "device_kernel_ms": med([r[2].kernel_ms for r in nd]), "device_launches": nd[0][2].launches,
          "device_slices": nd[0][2].rounds, "scan_ms": med([r[0] for r in nh]),
          "scan_kernel_ms": med([r[2].kernel_ms for r in nh]), "scan_launches": nh[0][2].launches}
    print(json.dumps({"n3": n3}), file=sys.stderr, flush=True)

    out = {"tool": "tools/scan_device_rate.py", "reps": args.reps, "build_id": distpow.build_id(), "mask_rate": rate,
           "place": place, "dense": dense, "sparse": sparse, "n3": n3}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    miner.close()


if __name__ == "__main__":
    main()
