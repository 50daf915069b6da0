"""The digests' measurements on one GPU.

  kernel      digest_kernel's rate from dpow_digests_device on 2^24 indices resident on the device,
              sequential and uniformly random below 2^55 (candidates over the stream's own event time
              around the launches), next to scan_kernel at N = 32 on a window of 2^24 candidates
              (candidates over the launches' own ticks), alternating in one process
  host_call   dpow_digests on host lists of n = 2^8 .. 2^24 sequential indices: time per call and
              entries per second, next to what a caller has today for the same list -- distpow.md5
              in a Python loop and dpow_digest_of_index in a C loop (dpow_cli digest-host) -- and the
              n at which the GPU call overtakes each
  staging     the two staging schemes (DPOW_DIAG_DIGEST_STAGING=mapped|copy) at n = 256 and n = 2^22
  chunk       the chunk sizes 2^16, 2^18, 2^20 (DPOW_DIAG_DIGEST_CHUNK) at n = 2^20, 2^22 and 2^24, in a
              library built with EXTRA=-DDPOW_DIGEST_CHUNK_LOG2=20 (--chunk-lib), the staging both ways
  outputs     one host list of 2^24 entries with both outputs, the digests alone and the depths alone
              (25, 24 and 9 bytes per entry through pinned memory): what binds the host call
Medians of REPS repetitions after one warm-up of each shape, the sides of each comparison
alternating; a host clock around calls that return only when the answers are back.

    python3 tools/digest_rate.py [--reps 5] [--out profiles/digest_rate.json] [--chunk-lib lib.so]
    python3 tools/digest_rate.py --only-outputs --out profiles/digest_rate.json   # adds that section to the file
"""
import argparse
import array
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-proof-of-work_amd"))

import distpow  # noqa: E402
from distpow import _lib  # noqa: E402

NONCE = bytes([1, 2, 3, 4])
G0 = 1 << 32


def med(xs):
    return statistics.median(xs)


class HostList:
    """n sequential indices from G0 and the outputs of one dpow_digests call, allocated once."""

    def __init__(self, n):
        self.n = n
        self.idx = array.array("Q", range(G0, G0 + n))
        self.addr = self.idx.buffer_info()[0]
        self.dig = ctypes.create_string_buffer(16 * n)
        self.dep = ctypes.create_string_buffer(n)
        self.done, self.st = ctypes.c_size_t(), _lib.BatchStats()

    def call(self, miner, dig=True, dep=True):
        t0 = time.perf_counter()
        rc = distpow.lib().dpow_digests(miner._ctx, NONCE, len(NONCE), self.addr, self.n, self.dig if dig else None,
                                        self.dep if dep else None, ctypes.byref(self.done), ctypes.byref(self.st))
        dt = time.perf_counter() - t0
        assert rc == distpow.EXHAUSTED and self.done.value == self.n, (rc, _lib.last_error())
        return dt

    def check(self):
        for j in (0, self.n // 2, self.n - 1):
            d, tz = distpow.digest_of_index(NONCE, G0 + j)
            assert self.dig.raw[16 * j:16 * j + 16] == d and self.dep.raw[j] == tz, j


def setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)


def measure_chunks(miner, reps):
    """Chunk sizes and stagings at n = 2^20, 2^22 and 2^24, alternating."""
    rows = []
    for lg in (20, 22, 24):
        hl = HostList(1 << lg)
        sides = [(st, c) for st in ("mapped", "copy") for c in (16, 18, 20)]
        times = {s: [] for s in sides}
        for rep in range(reps + 1):
            for s in sides:
                setenv("DPOW_DIAG_DIGEST_STAGING", s[0])
                setenv("DPOW_DIAG_DIGEST_CHUNK", 1 << s[1])
                dt = hl.call(miner)
                assert hl.st.launches == -(-hl.n >> s[1]), (hl.st.launches, s)
                if rep:
                    times[s].append(dt)
        hl.check()
        for s in sides:
            rows.append({"n": hl.n, "staging": s[0], "chunk_log2": s[1], "call_ms": med(times[s]) * 1e3,
                         "entries_per_s": hl.n / med(times[s])})
    setenv("DPOW_DIAG_DIGEST_STAGING", None)
    setenv("DPOW_DIAG_DIGEST_CHUNK", None)
    return rows


def measure_outputs(miner, reps):
    """One list of 2^24 entries with both outputs, the digests alone and the depths alone, alternating."""
    hl = HostList(1 << 24)
    sides = {"both": (True, True), "digests": (True, False), "depths": (False, True)}
    times, kern = {s: [] for s in sides}, {s: [] for s in sides}
    for rep in range(reps + 1):
        for s, (dig, dep) in sides.items():
            dt = hl.call(miner, dig, dep)
            if rep:
                times[s].append(dt)
                kern[s].append(hl.st.kernel_ms)
    hl.check()
    bytes_per_entry = {"both": 25, "digests": 24, "depths": 9}
    return [{"outputs": s, "n": hl.n, "bytes_per_entry": bytes_per_entry[s], "call_ms": med(times[s]) * 1e3,
             "kernel_ms": med(kern[s]), "ns_per_entry": med(times[s]) * 1e9 / hl.n} for s in sides]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-rate-only", action="store_true",
                    help="the kernel-rate section alone (an A/B of two builds needs nothing else)")
    ap.add_argument("--chunk-lib", default=None, help="a library built with EXTRA=-DDPOW_DIGEST_CHUNK_LOG2=20")
    ap.add_argument("--only-chunk", action="store_true", help="(the child run under --chunk-lib)")
    ap.add_argument("--only-outputs", action="store_true", help="measure the outputs section alone and add it to --out")
    args = ap.parse_args()
    miner = distpow.Miner(0)
    if args.only_outputs:
        rows = measure_outputs(miner, args.reps)
        miner.close()
        with open(args.out) as f:
            out = json.load(f)
        assert out["build_id"] == distpow.build_id(), "the file is another build's"
        out["outputs"] = rows
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(rows))
        return
    if args.only_chunk:
        print(json.dumps(measure_chunks(miner, args.reps)))
        miner.close()
        return

    # -- the kernel's rate beside scan_kernel's ---------------------------------------------------
    import torch
    dev = torch.device("cuda", 0)
    n = 1 << 24
    lists = {"sequential": torch.arange(G0, G0 + n, dtype=torch.int64, device=dev),
             "random": torch.randint(0, 1 << 55, (n,), dtype=torch.int64, device=dev,
                                     generator=torch.Generator(device=dev).manual_seed(1))}
    k0 = 1 << 24
    rate = {name: [] for name in lists}
    rate["scan"] = []
    for rep in range(args.reps + 1):
        for name, idx in lists.items():
            miner.digests_cuda(NONCE, idx)
            st = miner.last_digest_stats
            assert st.candidates == n and st.launches == 1
            if rep:
                rate[name].append(n / (st.kernel_ms * 1e-3) / 1e9)
        r, hits, k_done = miner.scan_page(NONCE, 32, 0, 0, k0, k0 + (n >> 8))
        st = miner.last_scan_stats
        assert (r, hits) == (distpow.EXHAUSTED, []) and st.candidates == n
        if rep:
            rate["scan"].append(n / (st.kernel_ms * 1e-3) / 1e9)
    # the sequential list's outputs against the host, at a few places
    dig, dep = miner.digests_cuda(NONCE, lists["sequential"])
    for j in (0, 12345, n - 1):
        d, tz = distpow.digest_of_index(NONCE, G0 + j)
        assert bytes(dig[j].cpu().tolist()) == d and int(dep[j]) == tz
    kernel = {"entries": n, "digest_sequential_ghs": med(rate["sequential"]), "digest_random_ghs": med(rate["random"]),
              "scan_kernel_ghs": med(rate["scan"]), "launches_per_call": 1,
              "sequential_over_scan": med(rate["sequential"]) / med(rate["scan"]),
              "random_over_scan": med(rate["random"]) / med(rate["scan"]),
              "bytes_per_entry": 25, "digest_sequential_gbs": med(rate["sequential"]) * 25,
              "all": rate}
    print(json.dumps({"kernel": kernel}), file=sys.stderr, flush=True)
    if args.kernel_rate_only:
        only = {"tool": "tools/digest_rate.py", "reps": args.reps, "build_id": distpow.build_id(), "kernel": kernel}
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(only, indent=1) + "\n")
        print(json.dumps(only))
        miner.close()
        return
    del lists, dig, dep
    torch.cuda.empty_cache()

    # -- what a caller has today ------------------------------------------------------------------
    m = 1 << 14
    py = []
    for rep in range(3):
        t0 = time.perf_counter()
        for g in range(G0, G0 + m):
            d = distpow.md5(NONCE + distpow.secret_from_index(g))
            distpow.trailing_zero_nibbles(d)
        py.append((time.perf_counter() - t0) / m * 1e9)
    cli = os.path.join(ROOT, "distributed-proof-of-work_amd", "distpow", "dpow_cli")
    c_loop = json.loads(subprocess.check_output([cli, "digest-host", NONCE.hex(), "18", str(args.reps)], timeout=120))
    today = {"python_loop_ns_per_entry": med(py), "python_loop_entries": m,
             "c_loop_ns_per_entry": c_loop["ns_per_entry"], "c_loop_entries": c_loop["n"]}
    print(json.dumps({"today": today}), file=sys.stderr, flush=True)

    # -- the host call ------------------------------------------------------------------------------
    host_rows = []
    for lg in range(8, 25):
        hl = HostList(1 << lg)
        hl.call(miner)
        ts, ks = [], []
        for _ in range(args.reps):
            ts.append(hl.call(miner))
            ks.append(hl.st.kernel_ms)
        hl.check()
        t = med(ts)
        host_rows.append({"n": hl.n, "call_ms": t * 1e3, "entries_per_s": hl.n / t, "ns_per_entry": t * 1e9 / hl.n,
                          "kernel_ms": med(ks), "launches": hl.st.launches,
                          "python_loop_ms": hl.n * today["python_loop_ns_per_entry"] * 1e-6,
                          "c_loop_ms": hl.n * today["c_loop_ns_per_entry"] * 1e-6})
        print(json.dumps(host_rows[-1]), file=sys.stderr, flush=True)
    cross = {}
    for key in ("python_loop_ms", "c_loop_ms"):
        cross[key.replace("_ms", "_overtaken_at_n")] = next((r["n"] for r in host_rows if r["call_ms"] < r[key]), None)

    # -- staging ------------------------------------------------------------------------------------
    staging_rows = []
    for nn in (256, 1 << 22):
        hl = HostList(nn)
        times = {"mapped": [], "copy": []}
        for rep in range(args.reps + 1):
            for s in times:
                setenv("DPOW_DIAG_DIGEST_STAGING", s)
                dt = hl.call(miner)
                if rep:
                    times[s].append(dt)
        hl.check()
        setenv("DPOW_DIAG_DIGEST_STAGING", None)
        staging_rows.append({"n": nn, "mapped_call_ms": med(times["mapped"]) * 1e3,
                             "copy_call_ms": med(times["copy"]) * 1e3, "launches": hl.st.launches})
        print(json.dumps(staging_rows[-1]), file=sys.stderr, flush=True)
    output_rows = measure_outputs(miner, args.reps)
    miner.close()

    # -- chunk sizes, in the library that allows 2^20 ---------------------------------------------
    chunk_rows = None
    if args.chunk_lib:
        env = dict(os.environ, DPOW_LIB_PATH=os.path.abspath(args.chunk_lib))
        chunk_rows = json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), "--only-chunk",
                                                         "--reps", str(args.reps)], env=env, timeout=600))

    out = {"tool": "tools/digest_rate.py", "reps": args.reps, "build_id": distpow.build_id(), "kernel": kernel,
           "today": today, "host_call": host_rows, "crossover": cross, "staging": staging_rows, "outputs": output_rows, "chunk": chunk_rows}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
