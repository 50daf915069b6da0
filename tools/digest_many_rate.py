"""The measurements of the digests of many nonces on one GPU.

  one_task    one task of 2^24 resident entries: digest_many_kernel's time beside digest_kernel's in the
              same run (the launches' own events), and the calls around them
  mix         256 and 4096 tasks of 2^12, 16 and 1 resident entries each: one Miner.digests_many_cuda call
              beside Miner.digests_cuda in a loop over the segments
  worst       4096 tasks of one entry: time per entry beside the C loop over dpow_digest_of_index
              (dpow_cli digest-host)
  chain       256 fresh nonces at N = 3 over 2^12 candidates each: scan_many_cuda -> digests_many_cuda
              beside scan_cuda -> digests_cuda per task
  host_form   256 tasks of 2^12 entries through Miner.digests_many beside Miner.digests in a loop; 2^24
              entries of one task with both outputs, with depths only and with neither (check only),
              dpow_digests_batch beside dpow_digests as C calls on buffers allocated once
  host_time   the device form's host time (the call minus its kernel time) against entries (16 tasks)
              and against tasks (2^16 entries)
Medians of REPS repetitions after one warm-up of each shape, the sides alternating in one process; a
host clock around calls that return only when the answers are complete.

    python3 tools/digest_many_rate.py [--reps 5] [--out profiles/digest_many_rate.json]
"""
import argparse
import array
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-proof-of-work_amd"))

import distpow  # noqa: E402
from distpow import DigestTask, ScanTask, _lib  # noqa: E402


def med(xs):
    return statistics.median(xs)


class T:
    def __init__(self, nonce, ntz=0):
        self.nonce, self.num_trailing_zeros = nonce, ntz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    miner = distpow.Miner(0)
    dev = torch.device("cuda", miner.device)
    rnd = random.Random(21)
    reps = args.reps

    def fresh(b, n=4):
        return [bytes(rnd.randrange(256) for _ in range(n)) for _ in range(b)]

    def timed(f):
        t0 = time.perf_counter()
        out = f()
        return (time.perf_counter() - t0) * 1e3, out

    def sides(a, b):
        """Medians of the two sides, alternating, after a warm-up of each: ([a's columns], [b's])."""
        a(), b()
        ra, rb = [], []
        for _ in range(reps):
            ra.append(a())
            rb.append(b())
        return [med(c) for c in zip(*ra)], [med(c) for c in zip(*rb)]

    out = {"reps": reps}

    # -- one task of 2^24 resident entries --------------------------------------------------------
    n = 1 << 24
    idx = torch.arange(n, dtype=torch.int64, device=dev) + (1 << 32)
    rows = torch.tensor([0, n], dtype=torch.int64, device=dev)
    nonce = bytes([1, 2, 3, 4])

    def many_one():
        ms, _ = timed(lambda: miner.digests_many_cuda([T(nonce)], idx, rows))
        return ms, miner.last_digest_many_stats.kernel_ms

    def single_one():
        ms, _ = timed(lambda: miner.digests_cuda(nonce, idx))
        return ms, miner.last_digest_stats.kernel_ms

    m, s = sides(many_one, single_one)
    out["one_task"] = {"entries": n, "digest_many_kernel_ms": m[1], "digest_kernel_ms": s[1],
                       "ratio_kernel": s[1] / m[1], "digests_many_cuda_ms": m[0], "digests_cuda_ms": s[0]}
    print("one_task", out["one_task"], flush=True)

    # -- many tasks, resident ------------------------------------------------------------------------
    out["mix"] = []
    for b in (256, 4096):
        for per in (1 << 12, 16, 1):
            total = b * per
            nonces = fresh(b)
            tasks = [T(x) for x in nonces]
            ix = idx[:total]
            rw = torch.arange(b + 1, dtype=torch.int64, device=dev) * per
            segs = [ix[j * per:(j + 1) * per] for j in range(b)]

            def one_call():
                ms, _ = timed(lambda: miner.digests_many_cuda(tasks, ix, rw))
                return ms, miner.last_digest_many_stats.kernel_ms

            def loop():
                def run():
                    for x, sg in zip(nonces, segs):
                        miner.digests_cuda(x, sg)
                return (timed(run)[0],)

            m, s = sides(one_call, loop)
            row = {"tasks": b, "entries_each": per, "digests_many_cuda_ms": m[0], "kernel_ms": m[1],
                   "digests_cuda_loop_ms": s[0], "speedup": s[0] / m[0], "ns_per_entry": m[0] * 1e6 / total}
            out["mix"].append(row)
            print("mix", row, flush=True)

    # -- the worst case beside the host loop ---------------------------------------------------------
    cli = os.path.join(ROOT, "distributed-proof-of-work_amd", "distpow", "dpow_cli")
    host = json.loads(subprocess.check_output([cli, "digest-host", "01020304", "12", str(reps)]).decode())
    worst = [r for r in out["mix"] if r["tasks"] == 4096 and r["entries_each"] == 1][0]
    out["worst"] = {"tasks": 4096, "entries_each": 1, "gpu_ns_per_entry": worst["ns_per_entry"],
                    "gpu_kernel_ns_per_entry": worst["kernel_ms"] * 1e6 / 4096,
                    "host_loop_ns_per_entry": host["ns_per_entry"]}
    print("worst", out["worst"], flush=True)

    # -- the chain behind the batched device scan ---------------------------------------------------------
    b = 256
    nonces = fresh(b)
    stasks = [ScanTask(x, 3, k_end=16) for x in nonces]

    def chain():
        def run():
            i, _, r = miner.scan_many_cuda(stasks, want_depths=False)
            return miner.digests_many_cuda(stasks, i, r)[0].shape[0]
        return (timed(run)[0],)

    def chain_loop():
        def run():
            for t in stasks:
                i, _ = miner.scan_cuda(t.nonce, 3, k_end=16, max_hits=1 << 14, want_depths=False)
                miner.digests_cuda(t.nonce, i)
        return (timed(run)[0],)

    m, s = sides(chain, chain_loop)
    out["chain"] = {"tasks": b, "ntz": 3, "candidates_each": 1 << 12, "scan_many_cuda_digests_many_cuda_ms": m[0],
                    "per_task_loop_ms": s[0], "speedup": s[0] / m[0]}
    print("chain", out["chain"], flush=True)

    # -- the host form ---------------------------------------------------------------------------------
    per = 1 << 12
    lists = [array.array("Q", range((1 << 32) + j * per, (1 << 32) + (j + 1) * per)) for j in range(b)]
    dtasks = [DigestTask(x, l) for x, l in zip(nonces, lists)]

    def host_many():
        ms, _ = timed(lambda: miner.digests_many(dtasks))
        return ms, miner.last_digest_many_stats.kernel_ms

    def host_loop():
        def run():
            for t in dtasks:
                miner.digests(t.nonce, t.indices)
        return (timed(run)[0],)

    m, s = sides(host_many, host_loop)
    out["host_form"] = {"tasks": b, "entries_each": per, "digests_many_ms": m[0], "kernel_ms": m[1],
                        "digests_loop_ms": s[0], "speedup": s[0] / m[0], "one_task_2p24": {}}
    # (The C calls on buffers allocated once, as tools/digest_rate.py measures dpow_digests.)
    big = array.array("Q", range(1 << 32, (1 << 32) + n))
    addr = big.buffer_info()[0]
    c_dig, c_dep = ctypes.create_string_buffer(16 * n), ctypes.create_string_buffer(n)
    c_rows = (ctypes.c_uint64 * 2)(0, n)
    c_task = (_lib.DigestTaskC * 1)()
    c_nonce = ctypes.create_string_buffer(nonce, len(nonce))
    c_task[0].nonce, c_task[0].nonce_len, c_task[0].ntz = ctypes.addressof(c_nonce), len(nonce), 1
    done, st = ctypes.c_size_t(), _lib.BatchStats()
    L = distpow.lib()

    def c_many(wd, wz):
        t0 = time.perf_counter()
        rc = L.dpow_digests_batch(miner._ctx, c_task, 1, c_rows, addr, c_dig if wd else None, c_dep if wz else None,
                                  ctypes.byref(done), ctypes.byref(st))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == distpow.EXHAUSTED and done.value == n, (rc, _lib.last_error())
        return dt, st.kernel_ms

    def c_single(wd, wz):
        t0 = time.perf_counter()
        rc = L.dpow_digests(miner._ctx, nonce, len(nonce), addr, n, c_dig if wd else None, c_dep if wz else None,
                            ctypes.byref(done), ctypes.byref(st))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == distpow.EXHAUSTED and done.value == n, (rc, _lib.last_error())
        return dt, st.kernel_ms

    for name, wd, wz in (("both", True, True), ("depths_only", False, True), ("check_only", False, False)):
        if wd or wz:
            m, s = sides(lambda: c_many(wd, wz), lambda: c_single(wd, wz))
            row = {"dpow_digests_batch_ms": m[0], "kernel_ms": m[1], "dpow_digests_ms": s[0]}
        else:  # (dpow_digests has no such mode)
            c_many(wd, wz)
            r = [c_many(wd, wz) for _ in range(reps)]
            row = {"dpow_digests_batch_ms": med([x[0] for x in r]), "kernel_ms": med([x[1] for x in r])}
        row["shallow"] = c_task[0].n_shallow
        out["host_form"]["one_task_2p24"][name] = row
    del big, c_dig, c_dep
    print("host_form", out["host_form"], flush=True)

    # -- the device form's host time ---------------------------------------------------------------------
    def host_time(b, total):
        per = total // b
        tasks = [T(x) for x in fresh(b)]
        ix = idx[:b * per]
        rw = torch.arange(b + 1, dtype=torch.int64, device=dev) * per
        miner.digests_many_cuda(tasks, ix, rw)
        ts, ks = [], []
        for _ in range(reps):
            ts.append(timed(lambda: miner.digests_many_cuda(tasks, ix, rw))[0])
            ks.append(miner.last_digest_many_stats.kernel_ms)
        return {"tasks": b, "entries": b * per, "call_ms": med(ts), "kernel_ms": med(ks), "host_ms": med(ts) - med(ks)}

    out["host_time"] = {"by_entries": [host_time(16, 1 << lg) for lg in (12, 16, 20, 24)],
                        "by_tasks": [host_time(b, 1 << 16) for b in (1, 16, 256, 4096)]}
    print("host_time", out["host_time"], flush=True)

    miner.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
