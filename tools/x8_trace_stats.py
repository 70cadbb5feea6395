"""Per-row kernel times of tools/bench_x8.py from a rocprofv3 kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -o x8 -- python tools/bench_x8.py --iters 5 --json bench_x8.json
    python tools/x8_trace_stats.py OUT/x8_results.db bench_x8.json profiles/x8/kernel_trace_stats.csv

The tool runs one row after another. Per row the product's kernel runs twice in a row of its own dispatches, each time
followed by torch's kernels: once for the check against the numpy model, then the timed hipGraph replays. So the
trace's runs of consecutive product dispatches come in pairs per row, and the second run of each pair is the timing.
Bytes per row (input read once + output written once) come from the tool's JSON record."""
import csv
import json
import re
import sqlite3
import statistics
import sys

_OURS = re.compile(r"(x8_shuffle_\w+_kernel|u8_clamp_\w+_kernel)")


def main(db_path, bench_json, out_csv):
    c = sqlite3.connect(db_path)
    disp = c.execute("select name, grid_x, grid_y, workgroup_x, vgpr_count, duration from kernels order by start").fetchall()
    runs, inside = [], False
    for d in disp:
        m = _OURS.search(d[0])
        if m:
            if not inside:
                runs.append([])
            runs[-1].append((m.group(1),) + tuple(d[1:]))
        inside = m is not None
    bench = json.load(open(bench_json))["rows"]
    assert len(runs) == 2 * len(bench), (len(runs), len(bench))
    out = csv.writer(open(out_csv, "w", newline=""))
    out.writerow(["bench_row", "kernel", "grid_x_threads", "grid_y", "workgroup", "vgpr", "dispatches", "median_us",
                  "min_us", "max_us", "bytes", "GBps_at_median"])
    for k, b in enumerate(bench):
        ds = runs[2 * k + 1]
        durs = [d[5] / 1e3 for d in ds]
        med = statistics.median(durs)
        gbps = b["bytes"] / (med * 1e-6) / 1e9
        out.writerow([b["row"], ds[0][0], ds[0][1], ds[0][2], ds[0][3], ds[0][4], len(ds), round(med, 2),
                      round(min(durs), 2), round(max(durs), 2), b["bytes"], round(gbps, 1)])
        print(f"{b['row']:52s} {ds[0][0]:26s} n={len(ds):3d} median {med:7.1f} us {gbps:8.1f} GB/s")


if __name__ == "__main__":
    main(*sys.argv[1:4])
