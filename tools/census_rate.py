"""The census's measurements on one GPU.

  census_rate  the census kernel's GH/s on one window of 2^28 k, next to scan_kernel at N = 32 on the
               same window (tools/scan_rate.py's method: candidates over the launches' own ticks),
               alternating in one process
  rare         the same rate with kCensusRare at 2, 3 and 4: libraries built with
               EXTRA=-DDPOW_CENSUS_RARE=<n> and named by --rare n=path (3 is the tree's own when not
               named), each through its own context, alternating in this process
  dense        N = 0's dense window, 2^20 candidates: one census beside one dpow_scan at N = 0
  fixture      the len04 window of tests/golden/layout_deep_hits.json: one census beside one scan at N = 8
Medians of REPS repetitions after one warm-up of each shape; a host clock around calls that return
only when the answers are back.

    python3 tools/census_rate.py [--reps 5] [--out profiles/census_rate.json] [--rate-log2k 28]
                                 [--rare 2=lib2.so --rare 4=lib4.so]
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


class RareLib:
    """One context of another build of the library, bound just far enough to take a census."""

    def __init__(self, path):
        self.L = L = ctypes.CDLL(path)
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        L.dpow_abi_version.restype = ctypes.c_int
        assert L.dpow_abi_version() == _lib.header_abi_version(), path
        L.dpow_open.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.dpow_close.argtypes = [vp]
        L.dpow_census_window.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, u64,
                                         u64, ctypes.POINTER(_lib.CensusC), ctypes.POINTER(u64),
                                         ctypes.POINTER(_lib.BatchStats)]
        self.ctx = vp()
        assert L.dpow_open(0, ctypes.byref(self.ctx)) == 0, path

    def census(self, nonce, k0, k1):
        c, kd, st = _lib.CensusC(), ctypes.c_uint64(), _lib.BatchStats()
        nb = bytes(nonce)
        rc = self.L.dpow_census_window(self.ctx, nb, len(nb), 0, 0, k0, k1, ctypes.byref(c), ctypes.byref(kd),
                                       ctypes.byref(st))
        assert rc == distpow.EXHAUSTED and kd.value == k1, (rc, kd.value)
        return tuple(c.count_ge), st

    def close(self):
        self.L.dpow_close(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-rate-only", action="store_true",
                    help="the kernel-rate section alone (an A/B of two builds needs nothing else)")
    ap.add_argument("--rate-log2k", type=int, default=28)
    ap.add_argument("--rare", action="append", default=[], metavar="N=LIB")
    args = ap.parse_args()
    miner = distpow.Miner(0)
    nonce = [1, 2, 3, 4]

    # -- the kernel's plain rate beside scan_kernel's ----------------------------------------------
    k0, nk = 1 << 24, 1 << args.rate_log2k
    miner.census(nonce, 0, 0, k0, k0 + (1 << 20))
    miner.scan(nonce, 32, 0, 0, k0, k0 + (1 << 20))
    cen_k, cen_w, scan_k, scan_w = [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r, c, k_done = miner.census_page(nonce, 0, 0, k0, k0 + nk)
        cen_w.append(nk * 256 / (time.perf_counter() - t0) / 1e9)
        st = miner.last_census_stats
        assert (r, k_done, c.count_ge[0]) == (distpow.EXHAUSTED, k0 + nk, nk * 256) and st.candidates == nk * 256
        cen_k.append(st.candidates / (st.kernel_ms * 1e-3) / 1e9)
        launches = st.launches
        t0 = time.perf_counter()
        r, hits, k_done = miner.scan_page(nonce, 32, 0, 0, k0, k0 + nk)
        scan_w.append(nk * 256 / (time.perf_counter() - t0) / 1e9)
        ss = miner.last_scan_stats
        assert (r, hits, k_done) == (distpow.EXHAUSTED, [], k0 + nk) and ss.candidates == nk * 256
        scan_k.append(ss.candidates / (ss.kernel_ms * 1e-3) / 1e9)
    rate = {"candidates": nk * 256, "census_kernel_ghs": med(cen_k), "census_wall_ghs": med(cen_w),
            "census_launches": launches, "scan_kernel_ghs": med(scan_k), "scan_wall_ghs": med(scan_w),
            "census_over_scan_kernel": med(cen_k) / med(scan_k), "deepest": c.deepest,
            "count_ge": list(c.count_ge[:c.deepest + 1]),
            "census_kernel_ghs_all": cen_k, "scan_kernel_ghs_all": scan_k}
    print(json.dumps({"census_rate": rate}), file=sys.stderr, flush=True)
    if args.kernel_rate_only:
        only = {"tool": "tools/census_rate.py", "reps": args.reps, "build_id": distpow.build_id(), "census_rate": rate}
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(only, indent=1) + "\n")
        print(json.dumps(only))
        miner.close()
        return

    # -- kCensusRare at 2, 3 and 4 -----------------------------------------------------------------
    rare = {}
    if args.rare:
        paths = dict(a.split("=", 1) for a in args.rare)
        paths.setdefault("3", distpow.LIB_PATH)
        libs = {n: RareLib(p) for n, p in sorted(paths.items())}
        ghs = {n: [] for n in libs}
        for n, lib in libs.items():
            assert lib.census(nonce, k0, k0 + (1 << 20))[0] == miner.census(nonce, 0, 0, k0, k0 + (1 << 20)).count_ge
        for _ in range(args.reps):
            for n, lib in libs.items():
                counts, st = lib.census(nonce, k0, k0 + nk)
                assert counts == c.count_ge, n   # every build counts the same
                ghs[n].append(st.candidates / (st.kernel_ms * 1e-3) / 1e9)
        rare = {"candidates": nk * 256, "kernel_ghs": {n: med(v) for n, v in ghs.items()}, "kernel_ghs_all": ghs}
        for lib in libs.values():
            lib.close()
        print(json.dumps({"rare": rare}), file=sys.stderr, flush=True)

    # -- the dense window: one census beside one scan at N = 0 --------------------------------------
    n_cand = 1 << 20
    arr = (_lib.ScanHitC * n_cand)()
    cnt, kd, st = ctypes.c_size_t(), ctypes.c_uint64(), _lib.BatchStats()
    nb = bytes(nonce)
    cen_ms, cen_kern, scan_ms, scan_kern = [], [], [], []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        r, cd, k_done = miner.census_page(nonce, 0, 0, 0, n_cand >> 8)
        dt = time.perf_counter() - t0
        assert (r, k_done, cd.count_ge[0]) == (distpow.EXHAUSTED, n_cand >> 8, n_cand)
        cl = miner.last_census_stats
        t1 = time.perf_counter()
        rc = distpow.lib().dpow_scan(miner._ctx, nb, len(nb), 0, 0, 0, 0, n_cand >> 8, arr, n_cand, ctypes.byref(cnt),
                                     ctypes.byref(kd), ctypes.byref(st))
        ds = time.perf_counter() - t1
        assert rc == distpow.EXHAUSTED and cnt.value == n_cand
        if rep:
            cen_ms.append(dt * 1e3)
            cen_kern.append(cl.kernel_ms)
            scan_ms.append(ds * 1e3)
            scan_kern.append(st.kernel_ms)
    dense = {"candidates": n_cand, "census_launches": cl.launches, "census_call_ms": med(cen_ms),
             "census_kernel_ms": med(cen_kern), "scan_launches": st.launches, "scan_call_ms": med(scan_ms),
             "scan_kernel_ms": med(scan_kern), "scan_over_census": med(scan_ms) / med(cen_ms),
             "deepest": cd.deepest, "count_ge": list(cd.count_ge[:cd.deepest + 1])}
    print(json.dumps({"dense": dense}), file=sys.stderr, flush=True)

    # -- a fixture window: one census beside one scan at N = 8 --------------------------------------
    with open(os.path.join(ROOT, "tests", "golden", "layout_deep_hits.json")) as f:
        case = next(x for x in json.load(f)["cases"] if x["name"] == "len04")
    args4 = (0, 0, case["k_begin"], case["k_end"])
    cf = miner.census(case["nonce"], *args4)
    hits = miner.scan(case["nonce"], 8, *args4)
    assert cf.count_ge[8] == len(hits) == len(case["hits"]) and cf.first_ge[8] == hits[0].global_idx
    t_cen, t_scan = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        miner.census(case["nonce"], *args4)
        t_cen.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        miner.scan(case["nonce"], 8, *args4)
        t_scan.append(time.perf_counter() - t0)
    fixture = {"case": "len04", "candidates": (case["k_end"] - case["k_begin"]) * 256, "census_ms": med(t_cen) * 1e3,
               "census_launches": miner.last_census_stats.launches, "scan_ms": med(t_scan) * 1e3,
               "scan_launches": miner.last_scan_stats.launches, "deepest": cf.deepest,
               "count_ge": list(cf.count_ge[:cf.deepest + 1])}
    print(json.dumps({"fixture": fixture}), file=sys.stderr, flush=True)

    out = {"tool": "tools/census_rate.py", "reps": args.reps, "build_id": distpow.build_id(), "census_rate": rate,
           "rare": rare, "dense": dense, "fixture": fixture}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    miner.close()


if __name__ == "__main__":
    main()
