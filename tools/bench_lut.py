"""Measurement aid: the sigmoid operator (byte lookup table, hip/x8lut.hip) at batch 128 on the MI355X, against the clamp
operator and a torch copy on the same buffers.

Rows: the 13 clamp shapes of tests/_x8.py (CLAMP_BENCH) at --batch. The yardstick is the CLAMP operator on the same
shape in the same process: same traffic (every byte read once and written once), same piece structure, no table. Each
row times, interleaved and --rounds times over, the sigmoid operator, the clamp operator (both with
qnnp_gfx950_time_operator_rotating: a hipGraph of launches replayed, median of five replays) and `y.copy_(x)` (a captured
graph of as many launches, median of five replays), all over the same (input, output) buffer pairs -- enough of them
that a buffer is reused only after >= 512 MiB of other traffic, past the 256 MiB Infinity Cache. The median round is
reported. --input chooses the bytes: `uniform` (every lookup a random table entry: the most LDS bank conflicts a table
read can meet) or `clustered` (a normal distribution around the zero point, as activations are: neighbouring lanes often
read the same dword, which broadcasts). The first run of each row is checked against torch indexing the operator's own
table (read back through the identity input).

    python tools/bench_lut.py [--batch 128] [--iters 20] [--input uniform] [--json out.json] [--text out.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_copy(ins, outs, iters, samples=5):
    """median over `samples` replays of a captured graph of `iters` copies rotating over the buffer sets, per copy (the
    method of tools/bench_x8.py time_torch)"""
    import torch
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for i in range(3):
            outs[i % len(outs)].copy_(ins[i % len(ins)])
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(iters):
            outs[i % len(outs)].copy_(ins[i % len(ins)])
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(samples):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        graph.replay()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / iters)
    del graph
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--input", choices=["uniform", "clustered"], default="uniform")
    ap.add_argument("--json", default=None)
    ap.add_argument("--text", default=None)
    ap.add_argument("--rows", default="", help="only the rows whose name contains this text")
    args = ap.parse_args()

    import torch
    import qnnpack_amd
    import _x8 as x8

    assert torch.cuda.is_available(), "bench_lut needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = qnnpack_amd.load()
    lib.initialize()
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    lib.set_async(False)
    gen = torch.Generator(device="cuda").manual_seed(7)

    identity = torch.arange(256, dtype=torch.uint8, device="cuda")
    table = torch.empty(256, dtype=torch.uint8, device="cuda")
    probe = lib.create_sigmoid_nc_q8(256, 121, 0.05, 0, 1.0 / 256.0, 0, 255)
    lib.setup_sigmoid_nc_q8(probe, 1, identity, 256, table, 256)
    lib.run_operator(probe)
    lib.delete_operator(probe)
    torch.cuda.synchronize()

    rows, lines = [], []
    for c, h in [s for s in x8.CLAMP_BENCH if args.rows in f"c{s[0]}_{s[1]}x{s[1]}"]:
        n = args.batch * h * h
        name = f"c{c}_{h}x{h}/b{args.batch}"
        nbytes = n * c
        nsets = max(1, -(-(512 << 20) // (2 * nbytes)))
        iters = max(args.iters, nsets)
        if args.input == "uniform":
            ins = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(nsets)]
        else:
            ins = [torch.normal(121.0, 20.0, (nbytes,), device="cuda", generator=gen).clamp_(0, 255).to(torch.uint8)
                   for _ in range(nsets)]
        outs = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        sigmoid = lib.create_sigmoid_nc_q8(c, 121, 0.05, 0, 1.0 / 256.0, 0, 255)
        clamp = lib.create_clamp_nc_u8(c, 0, 127)
        try:
            lib.setup_sigmoid_nc_q8(sigmoid, n, ins[0], c, outs[0], c)
            lib.run_operator(sigmoid)
            torch.cuda.synchronize()
            assert torch.equal(outs[0], table[ins[0].long()]), f"{name}: differs from the table applied by torch"
            lut_kernel = lib.operator_kernel(sigmoid)
            lib.setup_clamp_nc_u8(clamp, n, ins[0], c, outs[0], c)
            lib.run_operator(clamp)
            clamp_kernel = lib.operator_kernel(clamp)
            t = {"lut": [], "clamp": [], "copy": []}
            for _ in range(args.rounds):
                t["lut"].append(lib.time_operator_rotating(sigmoid, ins, outs, args.warmup, iters))
                t["clamp"].append(lib.time_operator_rotating(clamp, ins, outs, args.warmup, iters))
                t["copy"].append(time_copy(ins, outs, iters))
        finally:
            lib.delete_operator(sigmoid)
            lib.delete_operator(clamp)
        del ins, outs
        torch.cuda.empty_cache()
        us = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        gbps = {k: 2 * nbytes / (v * 1e-6) / 1e9 for k, v in us.items()}
        row = {"row": name, "input": args.input, "kernel": lut_kernel, "clamp_kernel": clamp_kernel, "pixels": n, "C": c,
               "bytes": 2 * nbytes, "buffer_sets": nsets, "launches": iters,
               "lut_us": round(us["lut"], 2), "clamp_us": round(us["clamp"], 2), "copy_us": round(us["copy"], 2),
               "lut_GBps": round(gbps["lut"], 1), "clamp_GBps": round(gbps["clamp"], 1), "copy_GBps": round(gbps["copy"], 1),
               "lut_over_clamp": round(us["lut"] / us["clamp"], 3), "lut_over_copy": round(us["lut"] / us["copy"], 3),
               "rounds_lut_us": [round(v * 1e3, 2) for v in t["lut"]], "rounds_clamp_us": [round(v * 1e3, 2) for v in t["clamp"]]}
        rows.append(row)
        line = (f"{name:22s} {lut_kernel:16s} {row['bytes'] / 1e6:8.1f} MB | lut {us['lut']:8.1f} us {gbps['lut']:7.1f} GB/s"
                f" | clamp {us['clamp']:8.1f} us {gbps['clamp']:7.1f} GB/s | copy {us['copy']:8.1f} us {gbps['copy']:7.1f} GB/s"
                f" | lut/clamp {row['lut_over_clamp']:.3f}  lut/copy {row['lut_over_copy']:.3f}")
        lines.append(line)
        print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"batch": args.batch, "iters": args.iters, "rounds": args.rounds, "input": args.input, "rows": rows},
                      f, indent=1)
    if args.text:
        with open(args.text, "w") as f:
            f.write(f"# tools/bench_lut.py --batch {args.batch} --iters {args.iters} --rounds {args.rounds} --input {args.input}\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
