#!/usr/bin/env python3
"""A/B of the generic kernels' rates between two built trees on one GPU.

Runs the kernel-rate section of tools/batch_rate.py, queue_rate.py, census_rate.py,
census_many_rate.py, scan_many_rate.py, digest_rate.py and scan_device_rate.py
(--kernel-rate-only) alternately from PARENT and from NEW, PARENT first, ROUNDS times, one process
per tool run, and records every round.  A figure passes when NEW's median of rounds is not below
PARENT's lowest round.  Both trees are built beforehand; a parent that predates the
--kernel-rate-only switch gets this tree's tools/ copied over its own (the tools only call the
library).  The first tool run that fails or runs out of time ends the whole run.

    python3 tools/generic_ab.py PARENT [--new .] [--rounds 3] [--reps 3] [--out profiles/generic_shared_ab.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med_of(rows, key):
    return statistics.median(r[key] for r in rows)


# tool -> {figure: how to read it from the tool's --kernel-rate-only output}
FIGURES = {
    "batch_rate.py": {"batch_kernel": lambda d: d["kernel_rate"]["batch_kernel_ghs"]},
    "queue_rate.py": {"queue_kernel": lambda d: med_of(d["m1_descriptor_launch"], "queue_ghs")},
    "census_rate.py": {"census_kernel": lambda d: d["census_rate"]["census_kernel_ghs"]},
    "census_many_rate.py": {"census_many_kernel": lambda d: d["kernel_rate"]["census_many_kernel_ghs"]},
    "scan_many_rate.py": {"scan_many_kernel": lambda d: d["kernel_rate"]["scan_many_kernel_ghs"],
                          "scan_kernel": lambda d: d["kernel_rate"]["scan_kernel_ghs"]},
    "digest_rate.py": {"digest_sequential": lambda d: d["kernel"]["digest_sequential_ghs"],
                       "digest_random": lambda d: d["kernel"]["digest_random_ghs"]},
    "scan_device_rate.py": {"scan_mask_kernel": lambda d: d["mask_rate"]["mask_kernel_ghs"]},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("--new", default=ROOT)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tool-timeout", type=float, default=150.0, help="seconds, per tool run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    trees = {"parent": os.path.abspath(args.parent), "new": os.path.abspath(args.new)}
    rounds = {side: {f: [] for figs in FIGURES.values() for f in figs} for side in trees}
    build = {}
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(args.rounds):
            for side, tree in trees.items():
                for tool, figs in FIGURES.items():
                    out = os.path.join(tmp, "rate.json")
                    subprocess.run([sys.executable, os.path.join(tree, "tools", tool), "--kernel-rate-only", "--reps",
                                    str(args.reps), "--out", out], check=True, timeout=args.tool_timeout,
                                   stdout=subprocess.DEVNULL)
                    with open(out) as f:
                        d = json.load(f)
                    build[side] = d["build_id"]
                    for name, read in figs.items():
                        rounds[side][name].append(read(d))
                print(json.dumps({"round": rnd + 1, "side": side, **{f: v[-1] for f, v in rounds[side].items()}}),
                      file=sys.stderr, flush=True)
    table = {}
    for name in rounds["parent"]:
        p, n = rounds["parent"][name], rounds["new"][name]
        table[name] = {"parent_rounds": p, "new_rounds": n, "parent_min": min(p), "parent_max": max(p),
                       "parent_median": statistics.median(p), "new_median": statistics.median(n),
                       "parent_spread_pct": 100 * (max(p) - min(p)) / statistics.median(p),
                       "new_over_parent_pct": 100 * (statistics.median(n) / statistics.median(p) - 1),
                       "pass": statistics.median(n) >= min(p)}
    result = {"tool": "tools/generic_ab.py", "unit": "GH/s", "rounds": args.rounds, "reps": args.reps,
              "parent_build_id": build["parent"], "new_build_id": build["new"], "figures": table,
              "all_pass": all(r["pass"] for r in table.values())}
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
