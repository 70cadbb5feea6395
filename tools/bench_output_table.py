"""Measurement aid: the hardswish behind the activated layers of MobileNetV3-large on the MI355X, three ways, all in one
process: the convolution alone, the chain the library offered so far (convolution, then the table operator in place on its
output: two dependent launches and one more pass over the tensor), and the convolution with the table attached
(qnnp_gfx950_attach_output_table: the lookup in the kernel's epilogue where the kernel carries it, else the same table
launch behind it).

Each of the three is recorded once into a hipGraph of its own and timed with qnnp_gfx950_graph_time (replays bracketed by
events). The three graphs are timed in turn, --rounds times over, and the median round is reported with the spread between
rounds, (max - min) / median. Every graph works on an output buffer of its own. Before the timing the attached operator's
output is compared once with the chain's.

The bar (profiles/output_table/README.md): the chain is the code the library had, so it is the yardstick; on a layer whose
kernel carries the table, the attached operator must not be slower than the chain by more than the spread the chain itself
shows over the rounds ("within_chain_spread").

The layers: the 3 -> 16 stem, the expand and depthwise layers of the hardswish blocks (from the block that produces the 80
channel tensors on), 160 -> 960 and the 960 -> 1280 classifier layer, at 224 x 224 input. Weights are uniform bytes around
kernel zero point 128, so the depthwise layers are in the range of the int8 dot-product walks, as trained networks'
depthwise weights around their zero point are.

    python tools/bench_output_table.py [--batches 1,128] [--iters 20] [--rounds 5] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, kind, input pixels per side, channels in, channels out, window, stride)
LAYERS = [
    ("stem_3x3s2_3_16", "conv", 224, 3, 16, 3, 2),
    ("b7_expand_40_240", "pw", 28, 40, 240, 1, 1),
    ("b7_dw3x3s2_240", "dw", 28, 240, 240, 3, 2),
    ("b8_expand_80_200", "pw", 14, 80, 200, 1, 1),
    ("b8_dw3x3_200", "dw", 14, 200, 200, 3, 1),
    ("b9_expand_80_184", "pw", 14, 80, 184, 1, 1),
    ("b9_dw3x3_184", "dw", 14, 184, 184, 3, 1),
    ("b11_expand_80_480", "pw", 14, 80, 480, 1, 1),
    ("b11_dw3x3_480", "dw", 14, 480, 480, 3, 1),
    ("b12_expand_112_672", "pw", 14, 112, 672, 1, 1),
    ("b12_dw3x3_672", "dw", 14, 672, 672, 3, 1),
    ("b13_dw5x5s2_672", "dw", 14, 672, 672, 5, 2),
    ("b14_expand_160_960", "pw", 7, 160, 960, 1, 1),
    ("b14_dw5x5_960", "dw", 7, 960, 960, 5, 1),
    ("classifier_960_1280", "fc", 1, 960, 1280, 1, 1),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,128")
    ap.add_argument("--layers", default=None, help="comma-separated layer names instead of all")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import qnnpack_amd

    assert torch.cuda.is_available(), "bench_output_table needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = qnnpack_amd.load()
    lib.initialize()
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    lib.set_async(False)
    gen = torch.Generator(device="cuda").manual_seed(23)
    rng = np.random.default_rng(23)
    izp, kzp, ozp = 121, 128, 110

    layers = LAYERS if args.layers is None else [l for l in LAYERS if l[0] in args.layers.split(",")]
    rows_out = []
    for batch in [int(b) for b in args.batches.split(",")]:
        for name, kind, hw, cin, cout, k, stride in layers:
            pad = k // 2
            ohw = (hw + 2 * pad - k) // stride + 1
            groups, gic, goc = (cin, 1, 1) if kind == "dw" else (1, cin, cout)
            reduction = k * k * gic
            kernel = rng.integers(0, 256, size=(groups, goc, k, k, gic), dtype=np.uint8)
            bias = rng.integers(-2000, 2001, size=cout, dtype=np.int32)
            # a sum of K products of a centred activation and a centred weight (74 rms each) spread over some 40 output steps
            scale = 40.0 / (74.0 * 74.0 * reduction ** 0.5)
            made = []

            def create():
                if kind == "fc":
                    op = lib.create_fully_connected_nc_q8(cin, cout, izp, 1.0, kzp, scale, kernel.reshape(cout, cin), bias, ozp, 1.0, 0, 255, 0)
                else:
                    op = lib.create_convolution2d_nhwc_q8(pad, pad, pad, pad, k, k, stride, stride, 1, 1, groups, gic, goc, izp, 1.0,
                                                          kzp, scale, kernel, bias, ozp, 1.0, 0, 255, 0)
                made.append(op)
                return op

            graphs = {}
            try:
                rows = batch * ohw * ohw
                x = torch.randint(0, 256, (batch * hw * hw * cin,), dtype=torch.uint8, device="cuda", generator=gen)
                out = {key: torch.zeros(rows * cout, dtype=torch.uint8, device="cuda") for key in ("alone", "chain", "attached")}
                ops = {key: create() for key in out}
                table = lib.create_hardswish_nc_q8(cout, ozp, 0.05, 20, 0.04, 0, 255, 0)
                made.append(table)
                for key, op in ops.items():
                    if kind == "fc":
                        lib.setup_fully_connected_nc_q8(op, batch, x, cin, out[key], cout)
                    else:
                        lib.setup_convolution2d_nhwc_q8(op, batch, hw, hw, x, cin, out[key], cout)
                lib.setup_lut_nc_x8(table, rows, out["chain"], cout, out["chain"], cout)
                lib.attach_output_table(ops["attached"], table)
                runs = {"alone": [ops["alone"]], "chain": [ops["chain"], table], "attached": [ops["attached"]]}
                # once: the attached operator writes the chain's bytes, the table moved them, the outputs are spread
                for sequence in runs.values():
                    for op in sequence:
                        lib.run_operator(op)
                torch.cuda.synchronize()
                assert torch.equal(out["attached"], out["chain"]), f"{name}: attached differs from the chain"
                assert not torch.equal(out["alone"], out["chain"]), name
                assert torch.unique(out["alone"]).numel() >= 64, name
                kernel_name, folded = lib.operator_kernel(ops["attached"]), lib.operator_table_folded(ops["attached"])
                assert kernel_name == lib.operator_kernel(ops["alone"]), (kernel_name, lib.operator_kernel(ops["alone"]))
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
                row = {"layer": name, "batch": batch, "rows": rows, "k": reduction, "channels": cout, "output_bytes": rows * cout,
                       "kernel": kernel_name, "folded": folded,
                       "alone_us": round(us["alone"], 2), "chain_us": round(us["chain"], 2), "attached_us": round(us["attached"], 2),
                       "chain_over_attached": round(us["chain"] / us["attached"], 3),
                       "table_share_of_chain": round((us["chain"] - us["alone"]) / us["chain"], 3),
                       "spread_alone": round(spread["alone"], 3), "spread_chain": round(spread["chain"], 3),
                       "spread_attached": round(spread["attached"], 3),
                       "within_chain_spread": bool(us["attached"] <= us["chain"] * (1.0 + spread["chain"])),
                       "rounds": args.rounds, "replays_per_sample": args.iters}
                rows_out.append(row)
                print(json.dumps(row), flush=True)
            finally:
                for graph in graphs.values():
                    lib.graph_destroy(graph)
                for op in reversed(made):
                    lib.delete_operator(op)
    result = {"device": lib.device_info(), "rows": rows_out}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
