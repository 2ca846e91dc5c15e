"""Per-kernel A/B of two rocprofv3 --kernel-trace --stats runs (tools/ab_kstats.sh): for every kernel among the
top N of the base run, the average per launch in both, the change, and whether the change exceeds twice the
standard error of the base's own average (StdDev / sqrt(calls) of the base trace).
usage: python tools/kstats_ab.py base/run_kernel_stats.csv new/run_kernel_stats.csv [N] [calls per step divisor]"""
import csv
import math
import sys


def load(path):
    return {r["Name"]: r for r in csv.DictReader(open(path))}


def main():
    base, new = load(sys.argv[1]), load(sys.argv[2])
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 12
    steps = float(sys.argv[4]) if len(sys.argv) > 4 else 0.0
    total = 0.0
    print(f"{'kernel':72s} {'calls':>6} {'base us':>8} {'new us':>8} {'delta':>7} {'2 SE':>6}  verdict")
    for name, b in sorted(base.items(), key=lambda kv: -float(kv[1]["TotalDurationNs"]))[:n]:
        w = new.get(name)
        if w is None:
            print(f"{name[:72]:72s} {b['Calls']:>6} {float(b['AverageNs']) / 1e3:8.2f}   (not in the new run)")
            continue
        calls = int(b["Calls"])
        ab, an = float(b["AverageNs"]) / 1e3, float(w["AverageNs"]) / 1e3
        se2 = 2.0 * float(b["StdDev"]) / 1e3 / math.sqrt(calls)
        d = an - ab
        verdict = "same" if abs(d) <= se2 else ("faster" if d < 0 else "SLOWER")
        per_step = f"  {d * calls / steps:+7.2f} us/step" if steps else ""
        if steps:
            total += d * calls / steps
        print(f"{name[:72]:72s} {calls:>6} {ab:8.2f} {an:8.2f} {d:+7.2f} {se2:6.2f}  {verdict}{per_step}")
    if steps:
        print(f"sum over the listed kernels: {total:+.2f} us per step")


if __name__ == "__main__":
    main()
