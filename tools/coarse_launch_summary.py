#!/usr/bin/env python3
"""Per-launch times of the fp32 network kernel from `rocprofv3 --kernel-trace` output, split into coarse and fine launches.

    python tools/coarse_launch_summary.py OUT.csv ARM=DIR [ARM=DIR ...]

Each DIR is searched for a *kernel_trace.csv.  A 512 x 512 frame is eight passes, each with one coarse (2.1 M points) and one
fine (6.3 M points) `mlp_f32_kernel` launch; the launches are split at the geometric mean of the shortest and the longest.
OUT.csv gets one row per arm and class: launches, mean / min / max / standard deviation in ms, and the per-pass means of the
coarse launches (launch i of a frame is pass i: the model of tools/gate_balance_model.py is per pass)."""
import csv
import glob
import os
import statistics
import sys


def launches(d):
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert paths, f"no kernel_trace.csv under {d}"
    out = []
    for row in csv.DictReader(open(paths[0])):
        if "mlp_f32_kernel" in row["Kernel_Name"]:
            out.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6))
    return [ms for _, ms in sorted(out)]


def main(out, *arms):
    rows = []
    for spec in arms:
        arm, d = spec.split("=", 1)
        ms = launches(d)
        cut = (min(ms) * max(ms)) ** 0.5
        for cls, sel in (("coarse", [m for m in ms if m < cut]), ("fine", [m for m in ms if m >= cut])):
            per_pass = ""
            if cls == "coarse" and len(sel) % 8 == 0:
                per_pass = " ".join(f"{statistics.mean(sel[i::8]):.4f}" for i in range(8))
            rows.append(dict(arm=arm, launches_of=cls, n=len(sel), mean_ms=f"{statistics.mean(sel):.4f}", min_ms=f"{min(sel):.4f}",
                             max_ms=f"{max(sel):.4f}", stdev_ms=f"{statistics.pstdev(sel):.4f}", coarse_mean_ms_by_pass=per_pass))
    with open(out, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    print(open(out).read())


if __name__ == "__main__":
    main(*sys.argv[1:])
