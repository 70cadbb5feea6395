"""Measurement aid: channel shuffle and clamp at batch 128 on the MI355X, against torch's equivalents on the same buffers.

Rows: every channel shuffle of the ShuffleNet units in the reference's convolution bench lists and a set of clamp shapes
(tests/_x8.py bench_cases). Each row is timed with qnnp_gfx950_time_operator_rotating (a hipGraph of launches replayed,
median of five replays) over enough (input, output) buffer pairs that a buffer is reused only after >= 512 MiB of other
traffic, past the 256 MiB Infinity Cache. The graph holds max(--iters, buffer pairs) launches, one per pair at least, so
each replay walks every pair and even the small rows are read from HBM. In the same process, interleaved row by row,
the torch equivalent runs on the same buffers and is timed the same way (a captured graph of as many launches, median
of five replays): `out.view(-1, gc, G).copy_(x.view(-1, G, gc).transpose(1, 2))` -- the copy that
`x.view(-1, G, gc).transpose(1, 2).contiguous()` makes -- and `torch.clamp(x, qmin, qmax, out=y)`. Bytes counted: the
input read once plus the output written once. The first run of each row is checked byte for byte against the numpy
model and against torch's result.

    python tools/bench_x8.py [--batch 128] [--iters 20] [--json out.json]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def torch_op(case, x, y):
    import torch
    if case.kind == "shuffle":
        y.view(-1, case.group_channels, case.groups).copy_(x.view(-1, case.groups, case.group_channels).transpose(1, 2))
    else:
        torch.clamp(x, case.qmin, case.qmax, out=y)


def time_torch(case, ins, outs, iters, samples=5):
    """median over `samples` replays of a captured graph of `iters` launches rotating over the buffer sets, per launch"""
    import torch
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for i in range(3):
            torch_op(case, ins[i % len(ins)], outs[i % len(outs)])
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(iters):
            torch_op(case, ins[i % len(ins)], outs[i % len(outs)])
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
    ap.add_argument("--json", default=None)
    ap.add_argument("--rows", default="", help="only the rows whose name contains this text")
    args = ap.parse_args()

    import torch
    import qnnpack_amd
    import _x8 as x8

    assert torch.cuda.is_available(), "bench_x8 needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = qnnpack_amd.load()
    lib.initialize()
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    lib.set_async(False)
    gen = torch.Generator(device="cuda").manual_seed(7)

    rows = []
    for case in [c for c in x8.bench_cases(args.batch) if args.rows in c.name]:
        n, c = case.batch, case.channels
        nbytes = n * c
        nsets = max(1, -(-(512 << 20) // (2 * nbytes)))
        iters = max(args.iters, nsets)
        ins = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(nsets)]
        outs = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        st, op = x8.create(lib, case)
        assert st == 0, (case.name, st)
        try:
            assert x8.setup_status(lib, case, op, n, ins[0], outs[0]) == 0
            lib.run_operator(op)
            torch.cuda.synchronize()
            head = dataclasses.replace(case, batch=64)
            want = x8.expected_one(head, ins[0][:64 * c].cpu().numpy(), 64)
            assert np.array_equal(outs[0][:want.size].cpu().numpy(), want), f"{case.name}: differs from the numpy model"
            ref_out = torch.empty_like(outs[0])
            torch_op(case, ins[0], ref_out)
            assert torch.equal(ref_out, outs[0]), f"{case.name}: differs from torch"
            del ref_out
            kname = lib.operator_kernel(op)
            ms = lib.time_operator_rotating(op, ins, outs, args.warmup, iters)
        finally:
            lib.delete_operator(op)
        torch_ms = time_torch(case, ins, outs, iters)
        del ins, outs
        torch.cuda.empty_cache()
        us, tus = ms * 1e3, torch_ms * 1e3
        shape = dict(G=case.groups, gc=case.group_channels) if case.kind == "shuffle" else dict(qmin=case.qmin, qmax=case.qmax)
        row = {"row": case.name, "kernel": kname, "pixels": n, "C": c, **shape, "bytes": 2 * nbytes,
               "buffer_sets": nsets, "launches": iters, "us": round(us, 2), "GBps": round(2 * nbytes / (us * 1e-6) / 1e9, 1),
               "torch_us": round(tus, 2), "torch_GBps": round(2 * nbytes / (tus * 1e-6) / 1e9, 1),
               "vs_torch": round(tus / us, 3)}
        rows.append(row)
        print(f"{case.name:52s} {kname:18s} {row['bytes'] / 1e6:8.1f} MB {us:8.1f} us {row['GBps']:7.1f} GB/s"
              f" | torch {tus:8.1f} us {row['torch_GBps']:7.1f} GB/s  x{row['vs_torch']:.2f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"batch": args.batch, "iters": args.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
