"""Measurement aid: the reference's pooling bench lists (bench/max-pooling.cc:93-138, bench/average-pooling.cc:94-145, restated
in tests/_pooling.py) at batch 128 on the MI355X.

Each row is timed with qnnp_gfx950_time_operator_rotating (a hipGraph of `iters` launches replayed, median of five
replays) over enough (input, output) buffer pairs that a buffer is reused only after >= 512 MiB of other traffic, past
the 256 MiB Infinity Cache. Bytes counted: the input read once plus the output written once (window overlap re-reads
are cache traffic, not counted). The first run of each row is checked byte for byte against the numpy model.

    python tools/bench_pooling.py [--batch 128] [--iters 20] [--json out.json]
"""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch
    import qnnpack_amd
    import _pooling as pl

    assert torch.cuda.is_available(), "bench_pooling needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = qnnpack_amd.load()
    lib.initialize()
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    lib.set_async(False)
    gen = torch.Generator(device="cuda").manual_seed(7)

    rows = []
    for case in pl.bench_cases(args.batch):
        n, h, w, c = case.batch, case.input_height, case.input_width, case.channels
        oh, ow = case.output_size(h, w)
        in_bytes, out_bytes = n * h * w * c, n * oh * ow * c
        nsets = max(1, -(-(512 << 20) // (in_bytes + out_bytes)))
        ins = [torch.randint(0, 256, (in_bytes,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(nsets)]
        outs = [torch.empty(out_bytes, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        st, op = pl.create(lib, case)
        assert st == 0, (case.name, st)
        try:
            assert pl.setup_status(lib, case, op, n, h, w, ins[0], outs[0]) == 0
            lib.run_operator(op)
            torch.cuda.synchronize()
            # the first two images against the numpy model (the whole batch would need gigabytes of host gathers)
            head = dataclasses.replace(case, batch=2)
            want = pl.expected(head, ins[0][:2 * h * w * c].cpu().numpy())[0]
            assert np.array_equal(outs[0][:want.size].cpu().numpy(), want), f"{case.name}: output differs from the numpy model"
            kname = lib.operator_kernel(op)
            ms = lib.time_operator_rotating(op, ins, outs, args.warmup, args.iters)
        finally:
            lib.delete_operator(op)
        del ins, outs
        torch.cuda.empty_cache()
        us = ms * 1e3
        row = {"row": case.name, "kernel": kname, "N": n, "H": h, "W": w, "K": case.pooling_height,
               "P": case.pad_top, "S": case.stride_height, "C": c, "bytes": in_bytes + out_bytes, "buffer_sets": nsets,
               "us": round(us, 2), "GBps": round((in_bytes + out_bytes) / (us * 1e-6) / 1e9, 1)}
        rows.append(row)
        print(f"{case.name:44s} {kname:16s} {row['bytes'] / 1e6:9.1f} MB {us:9.1f} us {row['GBps']:8.1f} GB/s", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"batch": args.batch, "iters": args.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
