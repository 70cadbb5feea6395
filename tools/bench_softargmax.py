"""Measurement aid: the softargmax operator (hip/q8softargmax.hip) on the MI355X against the byte lookup-table operator
on the same tensor.

Rows: classifier heads of 10, 100, 1000, 1001 and 21841 classes at batch 128 and 4096, and segmentation heads of 21 and
150 classes over 513 x 513 pixels at batch 8. The yardstick is the project's own byte lookup-table operator (sigmoid,
hip/x8lut.hip) on the same tensor in the same process: it moves the same bytes once in and once out, with one LDS lookup a
byte and no reduction. Each row times, interleaved and --rounds times over, both operators with
qnnp_gfx950_time_operator_rotating (a hipGraph of launches replayed, median of five replays) over the same (input, output)
buffer pairs -- enough of them that a buffer is reused only after >= 512 MiB of other traffic, past the 256 MiB Infinity
Cache, but at most MAX_BUFFER_SETS (as bench.py's ConvLayer caps them): the heads at batch 128 are a few KB to a few MB, a
rotation past the cache would take hundreds of thousands of buffers and as many launches in one captured graph, and
those rows are launch-bound whatever the cache holds (their `buffer_sets` column says 64). The median round is reported.
The input is random bytes, never a constant fill: a constant row of 1024 channels sums to 0 modulo 2^32, and every
lookup of a constant input hits one LDS bank. The first rows of the first run of each shape are checked against the
model of tests/_softargmax.py.

    python tools/bench_softargmax.py [--iters 20] [--rows seg] [--json out.json] [--text out.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLASSIFIER_CLASSES = (10, 100, 1000, 1001, 21841)
SHAPES = ([(f"head_c{c}/b{b}", b, c) for b in (128, 4096) for c in CLASSIFIER_CLASSES] +
          [(f"seg_c{c}_513x513/b8", 8 * 513 * 513, c) for c in (21, 150)])
MAX_BUFFER_SETS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--text", default=None)
    ap.add_argument("--rows", default="", help="only the rows whose name contains this text")
    args = ap.parse_args()

    import numpy as np
    import torch
    import qnnpack_amd
    import _softargmax as sam

    assert torch.cuda.is_available(), "bench_softargmax needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = qnnpack_amd.load()
    lib.initialize()
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    lib.set_async(False)
    gen = torch.Generator(device="cuda").manual_seed(11)

    rows, lines = [], []
    for name, n, c in [s for s in SHAPES if args.rows in s[0]]:
        nbytes = n * c
        nsets = min(MAX_BUFFER_SETS, max(1, -(-(512 << 20) // (2 * nbytes))))
        iters = max(args.iters, nsets)
        ins = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(nsets)]
        outs = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        softargmax = lib.create_softargmax_nc_q8(c, sam.DEFAULT_SCALE, 0, 1.0 / 256.0)
        lut = lib.create_sigmoid_nc_q8(c, 121, 0.05, 0, 1.0 / 256.0, 0, 255)
        try:
            lib.setup_softargmax_nc_q8(softargmax, n, ins[0], c, outs[0], c)
            lib.run_operator(softargmax)
            torch.cuda.synchronize()
            head = min(n, 256)
            case = sam.Case(name, head, c)
            want = sam.model(case, ins[0][:head * c].cpu().numpy())[0]
            assert np.array_equal(outs[0][:head * c].cpu().numpy(), want), f"{name}: differs from the model"
            kernel = lib.operator_kernel(softargmax)
            lib.setup_sigmoid_nc_q8(lut, n, ins[0], c, outs[0], c)
            lib.run_operator(lut)
            lut_kernel = lib.operator_kernel(lut)
            t = {"softargmax": [], "lut": []}
            for _ in range(args.rounds):
                t["softargmax"].append(lib.time_operator_rotating(softargmax, ins, outs, args.warmup, iters))
                t["lut"].append(lib.time_operator_rotating(lut, ins, outs, args.warmup, iters))
        finally:
            lib.delete_operator(softargmax)
            lib.delete_operator(lut)
        del ins, outs
        torch.cuda.empty_cache()
        us = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        tbps = {k: 2 * nbytes / (v * 1e-6) / 1e12 for k, v in us.items()}
        row = {"row": name, "kernel": kernel, "lut_kernel": lut_kernel, "rows": n, "C": c, "bytes": 2 * nbytes,
               "buffer_sets": nsets, "launches": iters,
               "softargmax_us": round(us["softargmax"], 2), "lut_us": round(us["lut"], 2),
               "softargmax_TBps": round(tbps["softargmax"], 3), "lut_TBps": round(tbps["lut"], 3),
               "softargmax_over_lut": round(us["softargmax"] / us["lut"], 3),
               "rounds_softargmax_us": [round(v * 1e3, 2) for v in t["softargmax"]],
               "rounds_lut_us": [round(v * 1e3, 2) for v in t["lut"]]}
        rows.append(row)
        line = (f"{name:24s} {kernel:30s} {row['bytes'] / 1e6:8.2f} MB | softargmax {us['softargmax']:8.1f} us "
                f"{tbps['softargmax']:6.3f} TB/s | lut {us['lut']:8.1f} us {tbps['lut']:6.3f} TB/s | softargmax/lut "
                f"{row['softargmax_over_lut']:.3f}")
        lines.append(line)
        print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"iters": args.iters, "rounds": args.rounds, "rows": rows}, f, indent=1)
    if args.text:
        with open(args.text, "w") as f:
            f.write(f"# tools/bench_softargmax.py --iters {args.iters} --rounds {args.rounds}\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
