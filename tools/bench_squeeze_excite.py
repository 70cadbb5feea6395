"""Measurement aid: a squeeze-and-excite block on the MI355X as the chain of its five stand-alone operators (global average
pooling, two fully connected layers, hardsigmoid, broadcast multiply: five dependent launches) against the fused operator
(qnnp_gfx950_create_squeeze_excite) in its two flavours -- "se_kernel" 1, the pooling inside the gate kernel (two
launches), and 2, the pooling operator's own launch in front of the gate kernel (three) -- all in one process.

Each of the three is recorded once into a hipGraph of its own and timed with qnnp_gfx950_graph_time (replays bracketed by
events, median of five batches). The three graphs are timed in turn, --rounds times over, and the median round is
reported with the spread between rounds, (max - min) / median. Every graph works on buffers of its own, in place on x as
a network would (the multiply writes x * s over x). Before the timing, the fused operator's output is compared once with
the chain's on equal inputs.

The working set of one graph is the tensor x and a few KB: batch 128 of 28 x 28 x 120 is 12 MB, so x stays in the 256 MiB
last-level cache between replays, for the chain and for the fused operator alike. The figures compare launch structure
and the squeeze path, not HBM bandwidth.

    python tools/bench_squeeze_excite.py [--batches 128,1] [--shapes 784x72x24,...] [--iters 20] [--rounds 5] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (pixels, C, S): MobileNetV3-large's squeeze-and-excite blocks, then a large image
SHAPES = [(28 * 28, 72, 24), (28 * 28, 120, 32), (14 * 14, 480, 120), (14 * 14, 672, 168), (7 * 7, 672, 168), (7 * 7, 960, 240),
          (112 * 112, 32, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,1")
    ap.add_argument("--shapes", default=None, help="PIXELSxCxS,... instead of the built-in list")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import qnnpack_amd
    import _multiply as mul

    assert torch.cuda.is_available(), "bench_squeeze_excite needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = qnnpack_amd.load()
    lib.initialize()
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    lib.set_async(False)
    gen = torch.Generator(device="cuda").manual_seed(17)
    rng = np.random.default_rng(17)
    q = mul.Quant(121, 0.05, 0, 1.0 / 256, 133, 0.04)

    shapes = SHAPES if args.shapes is None else [tuple(int(v) for v in item.split("x")) for item in args.shapes.split(",")]
    rows_out = []
    for batch in [int(b) for b in args.batches.split(",")]:
        for pixels, c, s in shapes:
            k1, b1 = rng.integers(0, 256, size=(s, c), dtype=np.uint8), rng.integers(-2000, 2001, size=s, dtype=np.int32)
            k2, b2 = rng.integers(0, 256, size=(c, s), dtype=np.uint8), rng.integers(-2000, 2001, size=c, dtype=np.int32)
            # requantization scales that spread the rows over their range without saturating them: a sum of K products
            # of a centred activation (about 87 rms after the pooling, 45 after the ReLU) and a centred weight (74 rms)
            scale1, scale2 = 64.0 / (6500.0 * c ** 0.5), 64.0 / (3300.0 * s ** 0.5)
            ops = [lib.create_global_average_pooling_nwc_q8(c, 121, 0.05, 119, 0.004, 0, 255, 0),
                   lib.create_fully_connected_nc_q8(c, s, 119, 1.0, 127, scale1, k1, b1, 60, 1.0, 60, 255, 0),
                   lib.create_fully_connected_nc_q8(s, c, 60, 1.0, 127, scale2, k2, b2, 128, 1.0, 0, 255, 0),
                   lib.create_hardsigmoid_nc_q8(c, 128, 0.011, 0, 1.0 / 256, 0, 255),
                   lib.create_multiply_nc_q8(c, *q.args())]
            fused = {1: lib.create_squeeze_excite(*ops), 2: lib.create_squeeze_excite(*ops)}
            graphs = {}
            try:
                gap, fc1, fc2, gate, multiply = ops
                nbytes = batch * pixels * c
                x0 = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=gen)
                x = {k: x0.clone() for k in ("chain", 1, 2)}
                d_p, d_h, d_e, d_s = (torch.empty(n, dtype=torch.uint8, device="cuda") for n in (batch * c, batch * s, batch * c, batch * c))
                lib.setup_global_average_pooling_nwc_q8(gap, batch, pixels, x["chain"], c, d_p, c)
                lib.setup_fully_connected_nc_q8(fc1, batch, d_p, c, d_h, s)
                lib.setup_fully_connected_nc_q8(fc2, batch, d_h, s, d_e, c)
                lib.setup_lut_nc_x8(gate, batch, d_e, c, d_s, c)
                lib.setup_multiply_nc_q8(multiply, batch, pixels, x["chain"], c, d_s, c, x["chain"], c)
                for flavour in (1, 2):
                    lib.set_option("se_kernel", flavour)
                    try:
                        lib.setup_squeeze_excite(fused[flavour], batch, pixels, x[flavour], c, x[flavour], c)
                    finally:
                        lib.set_option("se_kernel", 0)
                runs = {"chain": ops, 1: [fused[1]], 2: [fused[2]]}
                # once, on equal inputs: the fused operator writes the chain's bytes, and the gate is not saturated
                for key, sequence in runs.items():
                    for op in sequence:
                        lib.run_operator(op)
                torch.cuda.synchronize()
                gate_rows = d_s.cpu().numpy()
                assert np.unique(gate_rows).size >= 8, np.unique(gate_rows)
                for flavour in (1, 2):
                    assert torch.equal(x[flavour], x["chain"]), f"se_kernel {flavour} differs from the chain"
                kernels = {flavour: lib.operator_kernel(fused[flavour]) for flavour in (1, 2)}
                for key, sequence in runs.items():
                    lib.graph_begin()
                    try:
                        for op in sequence:
                            lib.run_operator(op)
                    finally:
                        graphs[key] = lib.graph_end()
                t = {key: [] for key in runs}
                for _ in range(args.rounds):
                    for key in runs:
                        t[key].append(lib.graph_time(graphs[key], args.warmup, args.iters))
                us = {key: statistics.median(v) * 1e3 for key, v in t.items()}
                spread = {key: (max(v) - min(v)) / statistics.median(v) for key, v in t.items()}
                row = {"batch": batch, "pixels": pixels, "channels": c, "squeeze": s, "x_bytes": nbytes, "image_bytes": pixels * c,
                       "chain_us": round(us["chain"], 2), "pool_inside_us": round(us[1], 2), "pool_in_front_us": round(us[2], 2),
                       "chain_over_pool_inside": round(us["chain"] / us[1], 3), "chain_over_pool_in_front": round(us["chain"] / us[2], 3),
                       "spread_chain": round(spread["chain"], 3), "spread_pool_inside": round(spread[1], 3),
                       "spread_pool_in_front": round(spread[2], 3), "kernels": [kernels[1], kernels[2]],
                       "rounds": args.rounds, "replays_per_sample": args.iters}
                rows_out.append(row)
                print(json.dumps(row), flush=True)
            finally:
                for graph in graphs.values():
                    lib.graph_destroy(graph)
                for op in fused.values():
                    lib.delete_operator(op)
                for op in reversed(ops):
                    lib.delete_operator(op)
    info = lib.device_info()
    result = {"device": info, "rows": rows_out}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
