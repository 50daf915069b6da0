#!/usr/bin/env python3
"""A/B of the batched host loops' time per call between a parent's library and this tree's, on one
GPU ("What the batched host loops share").

Runs tools/census_many_rate.py, scan_many_rate.py and scan_many_device_rate.py (or those named
with --tools) three times, one process per tool run: with the parent's libdpow.so (DPOW_LIB_PATH;
the tools only call the library, and its ABI is this binding's), with this tree's, and with the
parent's again.  Every figure is a call's host time in milliseconds: the tool's median wall time of
the call minus its median kernel time, the kernel time being what the launches' own ticks and the
stream's events give (dpow_batch_stats.kernel_ms), so the GPU's part of the call is not compared.
The margin of a figure is the distance between the two parent runs; a figure regresses when this
tree's run is slower than both parent runs by more than that.  The first tool run that fails or
runs out of time ends the whole run.  The output file holds a list of sessions; --append adds this
run to the sessions the file already has (a session with more repetitions of one tool, say).

    python3 tools/many_host_ab.py PARENT_LIBDPOW_SO [--reps 5] [--tools a.py,b.py] [--append]
                                  [--out profiles/many_host_ab.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shape(r):
    return f"{r['B']} x 2^{r['candidates_per_task'].bit_length() - 1}"


# tool -> how to read its figures {name: host ms} from its output
FIGURES = {
    "census_many_rate.py": lambda d: {
        **{f"census_many {_shape(r)}": r["many_call_ms"] - r["many_kernel_ms"] for r in d["tasks"]},
        "census_batch 4096 x 2^12 (where)": d["where"]["host_and_python_ms"]},
    "scan_many_rate.py": lambda d: {
        **{f"scan_many {_shape(r)}": r["many_call_ms"] - r["many_kernel_ms"] for r in d["tasks"]},
        "scan_batch dense 64 x 2^12": d["dense"]["host_and_python_ms"]},
    "scan_many_device_rate.py": lambda d: {
        **{f"scan_many_cuda {_shape(r)}": r["device_call_ms"] - r["device_kernel_ms"] for r in d["fresh"]},
        "scan_many_cuda dense 64 x 2^12": d["dense"]["device_host_ms"],
        **{f"scan_many_cuda 16 tasks, N = 0, 2^{r['candidates'].bit_length() - 1} hits": r["host_ms"]
           for r in d["host_by_hits"]},
        **{f"scan_many_cuda {r['tasks']} tasks, N = 3, 2^12 each": r["host_ms"] for r in d["host_by_tasks"]}},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rate-log2k", type=int, default=24, help="the tools' kernel-rate window (not compared here)")
    ap.add_argument("--tool-timeout", type=float, default=300.0, help="seconds, per tool run")
    ap.add_argument("--tools", default=",".join(FIGURES), help="comma-separated, of " + ", ".join(FIGURES))
    ap.add_argument("--append", action="store_true", help="keep the sessions --out already holds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tools = args.tools.split(",")
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for side in ("parent", "new", "parent"):
            env = dict(os.environ)
            env.pop("DPOW_LIB_PATH", None)
            if side == "parent":
                env["DPOW_LIB_PATH"] = os.path.abspath(args.parent_lib)
            figures, build = {}, None
            for tool in tools:
                read = FIGURES[tool]
                out = os.path.join(tmp, "rate.json")
                subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--reps", str(args.reps),
                                "--rate-log2k", str(args.rate_log2k), "--out", out], check=True, env=env,
                               timeout=args.tool_timeout, stdout=subprocess.DEVNULL)
                with open(out) as f:
                    d = json.load(f)
                build = d["build_id"]
                figures.update(read(d))
            runs.append({"side": side, "build_id": build, "ms": figures})
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    table = {}
    for name in runs[0]["ms"]:
        p1, n, p2 = (r["ms"][name] for r in runs)
        margin = abs(p1 - p2)
        table[name] = {"parent_1": p1, "new": n, "parent_2": p2, "parent_spread_ms": margin,
                       "parent_spread_pct": 100 * margin / min(p1, p2),
                       "new_over_slower_parent_pct": 100 * (n / max(p1, p2) - 1),
                       "inside_spread": min(p1, p2) - margin <= n <= max(p1, p2) + margin,
                       "regression": n > max(p1, p2) + margin}
    session = {"tools": tools, "reps": args.reps, "runs": runs, "figures": table,
               "regressions": [k for k, v in table.items() if v["regression"]]}
    result = {"tool": "tools/many_host_ab.py", "unit": "ms of host time per call (wall minus kernel)", "sessions": []}
    if args.append and args.out and os.path.exists(args.out):
        with open(args.out) as f:
            result["sessions"] = json.load(f)["sessions"]
    result["sessions"].append(session)
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
