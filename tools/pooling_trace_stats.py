"""Per-row kernel times of the pooling bench lists from a rocprofv3 kernel trace of tools/bench_pooling.py:

    rocprofv3 --kernel-trace --stats -d OUT -o pooling -- python tools/bench_pooling.py --iters 5
    python tools/pooling_trace_stats.py OUT/pooling_results.db bench_pooling.json profiles/pooling/kernel_trace_stats.csv

The tool runs one row after another, so the trace's consecutive runs of one (kernel, grid) are the rows, in order.
Bytes per row (input read once + output written once) come from the tool's JSON record."""
import csv
import json
import re
import sqlite3
import statistics
import sys


def main(db_path, bench_json, out_csv):
    c = sqlite3.connect(db_path)
    disp = c.execute("select name, grid_x, grid_y, workgroup_x, vgpr_count, duration from kernels "
                     "where name like '%pool_kernel%' order by start").fetchall()
    groups = []
    for d in disp:
        key = (d[0], d[1], d[2])
        if groups and groups[-1][0] == key:
            groups[-1][1].append(d)
        else:
            groups.append((key, [d]))
    bench = json.load(open(bench_json))["rows"]
    assert len(groups) == len(bench), (len(groups), len(bench))
    out = csv.writer(open(out_csv, "w", newline=""))
    out.writerow(["bench_row", "kernel", "grid_x_threads", "grid_y", "workgroup", "vgpr", "dispatches", "median_us",
                  "min_us", "max_us", "bytes", "GBps_at_median"])
    for (key, ds), b in zip(groups, bench):
        durs = [d[5] / 1e3 for d in ds]
        med = statistics.median(durs)
        name = re.search(r"q8_\w+_kernel<\d+>", key[0]).group(0)
        gbps = b["bytes"] / (med * 1e-6) / 1e9
        out.writerow([b["row"], name, key[1], key[2], ds[0][3], ds[0][4], len(ds), round(med, 2), round(min(durs), 2),
                      round(max(durs), 2), b["bytes"], round(gbps, 1)])
        print(f"{b['row']:44s} {name:22s} n={len(ds):3d} median {med:7.1f} us {gbps:8.1f} GB/s")


if __name__ == "__main__":
    main(*sys.argv[1:4])
