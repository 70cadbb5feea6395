"""Measurement aid: condense the counter-collection CSV of a `rocprofv3 --pmc ...` pass (one row per dispatch and counter)
into one row per (kernel, grid size, counter): the number of dispatches and the min / mean / max of the counter, summed
over the device as rocprofv3 reports it. The form of the pmc_*.csv files under profiles/.

    python tools/pmc_summary.py <dir or counter_collection.csv> [out.csv]
"""
import csv
import glob
import os
import re
import sys


def main():
    src = sys.argv[1]
    files = [src] if os.path.isfile(src) else sorted(glob.glob(os.path.join(src, "**", "*counter_collection.csv"), recursive=True))
    assert files, f"no counter_collection.csv under {src}"
    stats = {}
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"].replace("void ", "").replace("qnnp::(anonymous namespace)::", "")
                name = re.sub(r"\(.*$", "", name)         # the argument list
                key = (name, int(row["Grid_Size"]), row["Counter_Name"])
                stats.setdefault(key, []).append(float(row["Counter_Value"]))
    out = open(sys.argv[2], "w", newline="") if len(sys.argv) > 2 else sys.stdout
    w = csv.writer(out)
    w.writerow(["kernel", "grid_size", "counter", "dispatches", "min", "mean", "max"])
    for (name, grid, counter), v in sorted(stats.items()):
        w.writerow([name, grid, counter, len(v), int(min(v)), int(sum(v) / len(v)), int(max(v))])


if __name__ == "__main__":
    main()
