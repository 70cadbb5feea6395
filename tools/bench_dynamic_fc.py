"""Measurement aid: the dynamically quantized fully connected operator (qnnp_gfx950_create_fully_connected_nc_f32_qd8:
two launches) on the MI355X against the closest thing the library offered before it: quantize at a fixed, pre-computed
scale -> per-channel fully connected -> dequantize, three operators and a uint8 tensor on either side of the GEMM.

`qc4w` is the same operator with 4-bit weights (qnnp_gfx950_create_fully_connected_nc_f32_qd8_qc4w: the same weights
rounded down into [-8, 7], half the bytes), timed in turn with the int8 one; `qc4w_over_dynamic` is its time over the
int8 operator's of the same run.

`--qb4w` times something else: the 4-bit operator with block-wise scales
(qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w) at block sizes 64, 128 and 256 against the `qc4w` operator on the
same weights and tensors -- the four operators in turn, --rounds times over, medians and spreads as below;
`qb4w<B>_over_qc4w` is a time ratio within the run, `image_over_qc4w` the device image (weights and block table) over the
qc4w weight image.

`--qb4w-zp` times the block-wise operator with per-block zero points
(qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_zp) against the `qb4w` operator at the same block size, on the same
nibble bytes (read as unsigned by the one, as signed by the other), scales and tensors, in the same process -- the six
operators in turn, --rounds times over; `qb4w_zp<B>_over_qb4w<B>` is a time ratio within the run.

`--qb4w-b32` times the operator with blocks of 32 (qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_b32) against the
`qb4w_zp` operator at block size 64 on the same nibble bytes and tensors (every second scale and zero point), in the same
process -- the two operators in turn, --rounds times over; `qb4w_b32_over_qb4w_zp64` is a time ratio within the run and
`bytes_moved_ratio` the ratio of the bytes one run of either moves (device image, float rows in and out, quantized rows
written and read).

`--mxfp4w` times the MXFP4 operator (qnnp_gfx950_create_fully_connected_nc_f32_qd8_mxfp4w) against the `qb4w_b32` operator
in its signed form on the same nibble bytes (read as E2M1 codes by the one, as signed nibbles by the other), power-of-two
scales and tensors, in the same process -- the two operators in turn, --rounds times over; `mxfp4w_over_qb4w_b32` is a time
ratio within the run and `bytes_moved_ratio` as above.

`--grouped` times the GROUPED MXFP4 operator (qnnp_gfx950_create_grouped_fully_connected_nc_f32_qd8_mxfp4w: three launches,
the routing read on the device) against what a caller could do before it: one `_mxfp4w` operator per group, each set up on its
own PRE-GATHERED rows, run back to back. The read-back of the routing, the gather and the scatter that this needs are NOT
timed, and its launches are replayed from a graph without host gaps: both favour the per-group chain. Shapes are
GROUPSxBATCHxAxKxN; every token takes A distinct groups, uniformly at random. Either side is one run_operator pass recorded
into a hipGraph and timed with qnnp_gfx950_graph_time (median of five samples of --iters replays), the two in turn, --rounds
times over. `--crossover` adds, for the first shape's groups, K and N, both product kernels FORCED (the test header's
"qd8_grouped_kernel") at R = 8, 16 and 32 times the group count: the probe of the rule R <= 16 * groups.

Every operator is timed with qnnp_gfx950_time_operator_rotating over --sets pairs of input and output tensors (the
launches of one sample recorded into a hipGraph, median of five samples), the five operators in turn, --rounds times
over; the median round is reported with the spread between rounds, (max - min) / median. The chain's figure is the sum
of its three operators' medians: kernel time without the gaps between launches, as for the new operator. The tensors
rotate; the weights of one operator cannot, so at small batches they are served by the 256 MiB last-level cache and
`weights_gb_s` (weight bytes / time) is a cache figure wherever the image fits there, not an HBM figure.

`--gated` times the GATED setups (qnnp_gfx950_setup_[grouped_]fully_connected_nc_f32_qd8_gated, alpha = 1, limit = inf,
up_shift = 0) against what a caller does without them: a torch element-wise pass that writes silu(gate) * up as floats (sigmoid,
multiply, multiply: three launches into preallocated buffers) followed by the plain setup of a handle with the same weights.
Either side is recorded into a hipGraph and timed with qnnp_gfx950_graph_time, the sides in turn, --rounds times over; the torch
pass and the plain operator are also timed on their own, and the two row launches by themselves (`rows_alone_gb_s`: bytes read and
written over time). Shapes are FORMxGROUPSxROWSxKxN.

`--moe` times the two ends of a mixture-of-experts layer (include/qnnpack_gfx950_moe.h), each against what a caller does without
it, into preallocated buffers: the top-k router against torch.topk + softmax + the int64 -> int32 copy (three launches), and the
weighted combine against a torch multiply by the weights and a sum over the A axis (two launches and a T x A x N temporary;
every id counts, torch cannot skip rows). Each side is recorded into a hipGraph and timed as `--gated` is; `combine_gb_s` is
the bytes the combine reads and writes over its time. Shapes are ExAxNxT.

`--rmsnorm` times the RMSNORM setups (qnnp_gfx950_setup_[grouped_]fully_connected_nc_f32_qd8_rmsnorm, epsilon = 1e-5, a residual
and a residual_out of its own) against what a caller does without them: the torch chain add, square, mean, add epsilon, rsqrt and
two multiplies (seven launches into preallocated tensors, h written as floats) followed by the plain setup of a handle with the
same weights. Each side is recorded into a hipGraph and timed as `--gated` is; the torch chain and the plain operator are also
timed on their own. Shapes are FORMxGROUPSxROWSxKxN, FORM int8 or grouped.

    python tools/bench_dynamic_fc.py [--qb4w | --qb4w-zp | --qb4w-b32 | --mxfp4w | --grouped [--crossover] | --gated | --rmsnorm | --moe] [--shapes 1x4096x4096,...] [--sets 4] [--iters 20] [--rounds 5] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (batch, K, N): a dynamic linear at batch 1, 16 and 4096, the ViT-B MLP's first layer, and a layer whose int8 weight image
# (256 MiB) is about the size of the last-level cache
SHAPES = [(1, 4096, 4096), (16, 4096, 4096), (4096, 4096, 4096), (197, 768, 3072), (1, 16384, 16384), (16, 16384, 16384)]


BLOCKS = (64, 128, 256)


def qb4w_rows(lib, args, shapes, rng, gen, np, torch):
    """one record per shape: qc4w and qb4w at every block size, whole operators, alternating"""
    rows_out, inf = [], float("inf")
    for k, n in dict.fromkeys((k, n) for _, k, n in shapes):        # operators are made once per weight shape
        nibbles = rng.integers(0, 16, size=(n, k), dtype=np.uint8)
        packed = nibbles[:, 0::2] | (nibbles[:, 1::2] << 4)
        del nibbles
        bias = rng.standard_normal(n).astype(np.float32)
        ops = {"qc4w": lib.create_fully_connected_nc_f32_qd8_qc4w(k, n, packed, rng.uniform(0.005, 0.02, size=n).astype(np.float32),
                                                                  bias, -inf, inf)}
        for block in BLOCKS:
            scales = rng.uniform(0.005, 0.02, size=(n, k // block)).astype(np.float32)
            ops[f"qb4w{block}"] = lib.create_fully_connected_nc_f32_qd8_qb4w(k, n, block, packed, scales, bias, -inf, inf)
        try:
            for batch in [b for b, kk, nn in shapes if (kk, nn) == (k, n)]:
                x = [torch.randn(batch * k, dtype=torch.float32, device="cuda", generator=gen) for _ in range(args.sets)]
                y = [torch.empty(batch * n, dtype=torch.float32, device="cuda") for _ in range(args.sets)]
                for op in ops.values():
                    lib.setup_fully_connected_nc_f32_qd8(op, batch, x[0], k, y[0], n)
                    lib.run_operator(op)
                t = {key: [] for key in ops}
                for _ in range(args.rounds):
                    for key, op in ops.items():
                        t[key].append(lib.time_operator_rotating(op, x, y, args.warmup, args.iters))
                us = {key: statistics.median(v) * 1e3 for key, v in t.items()}
                row = {"batch": batch, "k": k, "n": n,
                       "us": {key: round(v, 2) for key, v in us.items()},
                       "spread": {key: round((max(v) - min(v)) / statistics.median(v), 3) for key, v in t.items()},
                       "kernels": {key: lib.operator_kernel(op) for key, op in ops.items()},
                       "image_mib": {"qc4w": round(n * k / 2 ** 21, 1),
                                     **{f"qb4w{b}": round((n * k / 2 + 8 * n * (k // b)) / 2 ** 20, 1) for b in BLOCKS}},
                       "sets": args.sets, "rounds": args.rounds, "launches_per_sample": args.iters}
                for b in BLOCKS:
                    row[f"qb4w{b}_over_qc4w"] = round(us[f"qb4w{b}"] / us["qc4w"], 3)
                    row.setdefault("image_over_qc4w", {})[f"qb4w{b}"] = round(1 + 16 / b, 4)
                rows_out.append(row)
                print(json.dumps(row), flush=True)
        finally:
            for op in ops.values():
                lib.delete_operator(op)
    return rows_out


def qb4w_zp_rows(lib, args, shapes, rng, gen, np, torch):
    """one record per shape: qb4w and qb4w_zp at every block size on the same nibble bytes, whole operators, alternating"""
    rows_out, inf = [], float("inf")
    for k, n in dict.fromkeys((k, n) for _, k, n in shapes):        # operators are made once per weight shape
        nibbles = rng.integers(0, 16, size=(n, k), dtype=np.uint8)
        packed = nibbles[:, 0::2] | (nibbles[:, 1::2] << 4)
        del nibbles
        bias = rng.standard_normal(n).astype(np.float32)
        ops = {}
        for block in BLOCKS:
            scales = rng.uniform(0.005, 0.02, size=(n, k // block)).astype(np.float32)
            zps = rng.integers(0, 16, size=(n, k // block), dtype=np.uint8)
            ops[f"qb4w{block}"] = lib.create_fully_connected_nc_f32_qd8_qb4w(k, n, block, packed, scales, bias, -inf, inf)
            ops[f"qb4w_zp{block}"] = lib.create_fully_connected_nc_f32_qd8_qb4w_zp(k, n, block, packed, scales, zps, bias, -inf, inf)
        try:
            for batch in [b for b, kk, nn in shapes if (kk, nn) == (k, n)]:
                x = [torch.randn(batch * k, dtype=torch.float32, device="cuda", generator=gen) for _ in range(args.sets)]
                y = [torch.empty(batch * n, dtype=torch.float32, device="cuda") for _ in range(args.sets)]
                for op in ops.values():
                    lib.setup_fully_connected_nc_f32_qd8(op, batch, x[0], k, y[0], n)
                    lib.run_operator(op)
                t = {key: [] for key in ops}
                for _ in range(args.rounds):
                    for key, op in ops.items():
                        t[key].append(lib.time_operator_rotating(op, x, y, args.warmup, args.iters))
                us = {key: statistics.median(v) * 1e3 for key, v in t.items()}
                row = {"batch": batch, "k": k, "n": n,
                       "us": {key: round(v, 2) for key, v in us.items()},
                       "spread": {key: round((max(v) - min(v)) / statistics.median(v), 3) for key, v in t.items()},
                       "kernels": {key: lib.operator_kernel(op) for key, op in ops.items()},
                       "image_mib": {f"qb4w_zp{b}": round((n * k / 2 + 8 * n * (k // b) + 2 * n * ((k + 127) // 128)) / 2 ** 20, 1)
                                     for b in BLOCKS},
                       "sets": args.sets, "rounds": args.rounds, "launches_per_sample": args.iters}
                for b in BLOCKS:
                    row[f"qb4w_zp{b}_over_qb4w{b}"] = round(us[f"qb4w_zp{b}"] / us[f"qb4w{b}"], 3)
                rows_out.append(row)
                print(json.dumps(row), flush=True)
        finally:
            for op in ops.values():
                lib.delete_operator(op)
    return rows_out


def qb4w_b32_rows(lib, args, shapes, rng, gen, np, torch):
    """one record per shape: qb4w_zp at B = 64 and qb4w_b32 on the same nibble bytes, whole operators, alternating"""
    rows_out, inf = [], float("inf")
    for k, n in dict.fromkeys((k, n) for _, k, n in shapes):        # operators are made once per weight shape
        nibbles = rng.integers(0, 16, size=(n, k), dtype=np.uint8)
        packed = nibbles[:, 0::2] | (nibbles[:, 1::2] << 4)
        del nibbles
        bias = rng.standard_normal(n).astype(np.float32)
        scales = rng.uniform(0.005, 0.02, size=(n, k // 32)).astype(np.float32)
        zps = rng.integers(0, 16, size=(n, k // 32), dtype=np.uint8)
        ops = {"qb4w_zp64": lib.create_fully_connected_nc_f32_qd8_qb4w_zp(k, n, 64, packed, scales[:, 0::2], zps[:, 0::2], bias, -inf, inf),
               "qb4w_b32": lib.create_fully_connected_nc_f32_qd8_qb4w_b32(k, n, packed, scales, zps, bias, -inf, inf)}
        # device bytes per weight: nibbles + tables (B = 64: 8 per block and 2 per 128 positions; B = 32: 6 per block)
        image = {"qb4w_zp64": 0.5 + 8 / 64 + 2 / 128, "qb4w_b32": 0.5 + 6 / 32}
        try:
            for batch in [b for b, kk, nn in shapes if (kk, nn) == (k, n)]:
                x = [torch.randn(batch * k, dtype=torch.float32, device="cuda", generator=gen) for _ in range(args.sets)]
                y = [torch.empty(batch * n, dtype=torch.float32, device="cuda") for _ in range(args.sets)]
                for op in ops.values():
                    lib.setup_fully_connected_nc_f32_qd8(op, batch, x[0], k, y[0], n)
                    lib.run_operator(op)
                t = {key: [] for key in ops}
                for _ in range(args.rounds):
                    for key, op in ops.items():
                        t[key].append(lib.time_operator_rotating(op, x, y, args.warmup, args.iters))
                us = {key: statistics.median(v) * 1e3 for key, v in t.items()}
                # bytes one run moves: the image once, the float rows in, the quantized rows out and in again, the float rows out
                moved = {key: n * k * image[key] + batch * (4 * k + 2 * k + 4 * n) for key in ops}
                row = {"batch": batch, "k": k, "n": n,
                       "us": {key: round(v, 2) for key, v in us.items()},
                       "spread": {key: round((max(v) - min(v)) / statistics.median(v), 3) for key, v in t.items()},
                       "kernels": {key: lib.operator_kernel(op) for key, op in ops.items()},
                       "image_mib": {key: round(n * k * image[key] / 2 ** 20, 1) for key in ops},
                       "qb4w_b32_over_qb4w_zp64": round(us["qb4w_b32"] / us["qb4w_zp64"], 3),
                       "bytes_moved_ratio": round(moved["qb4w_b32"] / moved["qb4w_zp64"], 3),
                       "sets": args.sets, "rounds": args.rounds, "launches_per_sample": args.iters}
                rows_out.append(row)
                print(json.dumps(row), flush=True)
        finally:
            for op in ops.values():
                lib.delete_operator(op)
    return rows_out


def mxfp4w_rows(lib, args, shapes, rng, gen, np, torch):
    """one record per shape: qb4w_b32 (signed form) and mxfp4w on the same nibble bytes, whole operators, alternating"""
    rows_out, inf = [], float("inf")
    for k, n in dict.fromkeys((k, n) for _, k, n in shapes):        # operators are made once per weight shape
        nibbles = rng.integers(0, 16, size=(n, k), dtype=np.uint8)
        packed = nibbles[:, 0::2] | (nibbles[:, 1::2] << 4)
        del nibbles
        bias = rng.standard_normal(n).astype(np.float32)
        exponents = rng.integers(118, 123, size=(n, k // 32), dtype=np.uint8)          # 2^-9 .. 2^-5: the range of the float scales
        scales = np.ldexp(np.float32(1), exponents.astype(np.int32) - 127).astype(np.float32)
        ops = {"qb4w_b32": lib.create_fully_connected_nc_f32_qd8_qb4w_b32(k, n, packed, scales, None, bias, -inf, inf),
               "mxfp4w": lib.create_fully_connected_nc_f32_qd8_mxfp4w(k, n, packed, exponents, bias, -inf, inf)}
        # device bytes per weight: nibbles + tables (6 bytes per block of 32; 4 bytes per block of 32)
        image = {"qb4w_b32": 0.5 + 6 / 32, "mxfp4w": 0.5 + 4 / 32}
        try:
            for batch in [b for b, kk, nn in shapes if (kk, nn) == (k, n)]:
                x = [torch.randn(batch * k, dtype=torch.float32, device="cuda", generator=gen) for _ in range(args.sets)]
                y = [torch.empty(batch * n, dtype=torch.float32, device="cuda") for _ in range(args.sets)]
                for op in ops.values():
                    lib.setup_fully_connected_nc_f32_qd8(op, batch, x[0], k, y[0], n)
                    lib.run_operator(op)
                t = {key: [] for key in ops}
                for _ in range(args.rounds):
                    for key, op in ops.items():
                        t[key].append(lib.time_operator_rotating(op, x, y, args.warmup, args.iters))
                us = {key: statistics.median(v) * 1e3 for key, v in t.items()}
                # bytes one run moves: the image once, the float rows in, the quantized rows out and in again, the float rows out
                moved = {key: n * k * image[key] + batch * (4 * k + 2 * k + 4 * n) for key in ops}
                row = {"batch": batch, "k": k, "n": n,
                       "us": {key: round(v, 2) for key, v in us.items()},
                       "spread": {key: round((max(v) - min(v)) / statistics.median(v), 3) for key, v in t.items()},
                       "kernels": {key: lib.operator_kernel(op) for key, op in ops.items()},
                       "image_mib": {key: round(n * k * image[key] / 2 ** 20, 1) for key in ops},
                       "mxfp4w_over_qb4w_b32": round(us["mxfp4w"] / us["qb4w_b32"], 3),
                       "bytes_moved_ratio": round(moved["mxfp4w"] / moved["qb4w_b32"], 3),
                       "sets": args.sets, "rounds": args.rounds, "launches_per_sample": args.iters}
                rows_out.append(row)
                print(json.dumps(row), flush=True)
        finally:
            for op in ops.values():
                lib.delete_operator(op)
    return rows_out


# (groups, batch, A, K, N): a small and a large mixture-of-experts layer at decode batches, and two at prefill sizes
GROUPED_SHAPES = [(32, 16, 4, 2880, 2880), (128, 64, 4, 2880, 2880), (32, 4096, 4, 2880, 5760), (8, 4096, 2, 4096, 14336)]


def graph_us(lib, ops, args):
    """one pass over `ops` recorded into a graph; microseconds per replay"""
    lib.graph_begin()
    try:
        for op in ops:
            lib.run_operator(op)
    finally:
        graph = lib.graph_end()
    try:
        return lib.graph_time(graph, args.warmup, args.iters) * 1e3
    finally:
        lib.graph_destroy(graph)


def grouped_rows(lib, args, shapes, rng, gen, np, torch):
    """one record per shape: the grouped operator and the per-group chain on the same weights and routing, alternating; with
    --crossover also the two forced kernels at R = 8, 16 and 32 times the group count"""
    rows_out, inf = [], float("inf")
    probes = [(shapes[0][0], shapes[0][0] * m // 4, 4, shapes[0][3], shapes[0][4], forced)
              for m in (8, 16, 32) for forced in (1, 2)] if args.crossover else []
    weights = {}
    for groups, batch, a, k, n, forced in [s + (0,) for s in shapes] + probes:
        if (groups, k, n) not in weights:
            weights.clear()                     # one set of weights at a time on the host
            weights[groups, k, n] = (rng.integers(0, 256, size=(groups, n, k // 2), dtype=np.uint8),
                                     rng.integers(118, 123, size=(groups, n, k // 32), dtype=np.uint8),
                                     rng.standard_normal((groups, n)).astype(np.float32))
        packed, exponents, bias = weights[groups, k, n]
        rows = batch * a
        ids = np.argsort(rng.random((batch, groups)), axis=1)[:, :a].astype(np.int32).reshape(-1)     # A distinct groups per token
        d_ids = torch.from_numpy(ids).cuda()
        x = torch.randn(batch * k, dtype=torch.float32, device="cuda", generator=gen)
        y = torch.empty(rows * n, dtype=torch.float32, device="cuda")
        lib.set_option("qd8_grouped_kernel", forced)
        ops = {"grouped": [lib.create_grouped_fully_connected_nc_f32_qd8_mxfp4w(groups, k, n, packed, exponents, bias, -inf, inf)]}
        keep = []
        try:
            lib.setup_grouped_fully_connected_nc_f32_qd8(ops["grouped"][0], batch, a, x, k, d_ids, y, n)
            lib.set_option("qd8_grouped_kernel", 0)
            counts = np.bincount(ids, minlength=groups)
            if not forced:
                ops["per_group"] = []
                for g in np.flatnonzero(counts):
                    op = lib.create_fully_connected_nc_f32_qd8_mxfp4w(k, n, packed[g], exponents[g], bias[g], -inf, inf)
                    ops["per_group"].append(op)
                    keep.append((torch.randn(int(counts[g]) * k, dtype=torch.float32, device="cuda", generator=gen),
                                 torch.empty(int(counts[g]) * n, dtype=torch.float32, device="cuda")))
                    lib.setup_fully_connected_nc_f32_qd8(op, int(counts[g]), keep[-1][0], k, keep[-1][1], n)
            for side in ops.values():
                for op in side:
                    lib.run_operator(op)
            t = {key: [] for key in ops}
            for _ in range(args.rounds):
                for key, side in ops.items():
                    t[key].append(graph_us(lib, side, args))
            us = {key: statistics.median(v) for key, v in t.items()}
            row = {"groups": groups, "batch": batch, "assignments": a, "rows": rows, "k": k, "n": n, "forced": forced,
                   "us": {key: round(v, 2) for key, v in us.items()},
                   "spread": {key: round((max(v) - min(v)) / statistics.median(v), 3) for key, v in t.items()},
                   "kernel": lib.operator_kernel(ops["grouped"][0]),
                   "live_groups": int(np.count_nonzero(counts)), "largest_group": int(counts.max()),
                   "image_mib": round(groups * n * k * (0.5 + 4 / 32) / 2 ** 20, 1),
                   "rounds": args.rounds, "replays_per_sample": args.iters}
            if not forced:
                row["per_group_kernels"] = sorted({lib.operator_kernel(op) for op in ops["per_group"]})
                row["per_group_over_grouped"] = round(us["per_group"] / us["grouped"], 3)
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        finally:
            lib.set_option("qd8_grouped_kernel", 0)
            for side in ops.values():
                for op in side:
                    lib.delete_operator(op)
    return rows_out


# the gated setups: (form, groups, rows, K, N) -- the expert layer of profiles/dynamic_fc_grouped at decode and prefill sizes
# (A = 1), and a dense down projection (K = 14336 -> N = 4096) with _qb4w_b32 weights at batch 1, 16 and 512
GATED_SHAPES = [("grouped", 32, 64, 2880, 2880), ("grouped", 32, 16384, 2880, 2880),
                ("qb4w_b32", 0, 1, 14336, 4096), ("qb4w_b32", 0, 16, 14336, 4096), ("qb4w_b32", 0, 512, 14336, 4096)]


def rows_alone_us(lib, args, torch, x, rows, k, gated):
    """the row launch by itself (qnnp_hip_qd8_[gated_]rows_run, the library's internal launch entry), recorded into a graph"""
    import ctypes
    head = [("input", ctypes.c_void_p), ("quantized", ctypes.c_void_p), ("row_table", ctypes.c_void_p), ("rows", ctypes.c_uint32),
            ("k", ctypes.c_uint32), ("k_pad", ctypes.c_uint32), ("input_stride", ctypes.c_uint64)]
    tail = [("alpha", ctypes.c_float), ("limit", ctypes.c_float), ("up_shift", ctypes.c_float)] if gated else []
    launch_args = type("RowsArgs", (ctypes.Structure,), {"_fields_": head + tail})
    k_pad = (k + 63) // 64 * 64
    quantized = torch.empty(rows * k_pad, dtype=torch.int8, device="cuda")
    table = torch.empty(rows * 2, dtype=torch.float32, device="cuda")
    values = (x.data_ptr(), quantized.data_ptr(), table.data_ptr(), rows, k, k_pad, (2 if gated else 1) * k)
    a = launch_args(*values, *((1.0, float("inf"), 0.0) if gated else ()))
    run = getattr(lib.lib, "qnnp_hip_qd8_gated_rows_run" if gated else "qnnp_hip_qd8_rows_run")
    run.argtypes, run.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    name = ctypes.c_char_p()
    assert run(ctypes.byref(a), ctypes.byref(name)) == 0
    torch.cuda.synchronize()
    lib.graph_begin()
    try:
        assert run(ctypes.byref(a), None) == 0
    finally:
        graph = lib.graph_end()
    try:
        return lib.graph_time(graph, args.warmup, args.iters) * 1e3, name.value.decode()
    finally:
        lib.graph_destroy(graph)


def gated_rows(lib, args, shapes, rng, gen, np, torch):
    """one record per shape: the gated setup against what a caller does without it -- a torch element-wise pass that writes
    h = silu(gate) * up as floats, then the plain setup of a handle with the same weights -- each recorded into a graph, the two
    in turn; and the two row launches by themselves"""
    rows_out, inf = [], float("inf")
    weights = {}
    for form, groups, rows, k, n in shapes:
        if (form, groups, k, n) not in weights:
            weights.clear()
            g = max(groups, 1)
            weights[form, groups, k, n] = (rng.integers(0, 256, size=(g, n, k // 2), dtype=np.uint8),
                                          rng.integers(118, 123, size=(g, n, k // 32), dtype=np.uint8),
                                          rng.standard_normal((g, n)).astype(np.float32))
        packed, exponents, bias = weights[form, groups, k, n]
        x = torch.randn(rows * 2 * k, dtype=torch.float32, device="cuda", generator=gen)
        h = torch.empty(rows * k, dtype=torch.float32, device="cuda")
        t = torch.empty(rows, k, dtype=torch.float32, device="cuda")
        y = torch.empty(rows * n, dtype=torch.float32, device="cuda")
        gate, up = x.view(rows, 2 * k)[:, 0::2], x.view(rows, 2 * k)[:, 1::2]
        ops = []
        try:
            for _ in range(2):          # the same weights twice: one handle is set up gated, the other plain
                if form == "grouped":
                    ops.append(lib.create_grouped_fully_connected_nc_f32_qd8_mxfp4w(groups, k, n, packed, exponents, bias, -inf, inf))
                else:
                    scales = np.ldexp(np.float32(1), exponents[0].astype(np.int32) - 127).astype(np.float32)
                    ops.append(lib.create_fully_connected_nc_f32_qd8_qb4w_b32(k, n, packed[0], scales, None, bias[0], -inf, inf))
            if form == "grouped":
                d_ids = torch.from_numpy(rng.integers(0, groups, rows).astype(np.int32)).cuda()
                lib.setup_grouped_fully_connected_nc_f32_qd8_gated(ops[0], rows, 1, x, 2 * k, 1.0, inf, 0.0, d_ids, y, n)
                lib.setup_grouped_fully_connected_nc_f32_qd8(ops[1], rows, 1, h, k, d_ids, y, n)
            else:
                lib.setup_fully_connected_nc_f32_qd8_gated(ops[0], rows, x, 2 * k, 1.0, inf, 0.0, y, n)
                lib.setup_fully_connected_nc_f32_qd8(ops[1], rows, h, k, y, n)

            def torch_pass():           # three launches into preallocated buffers: nothing is allocated under a capture
                torch.sigmoid(gate, out=t)
                t.mul_(gate)
                torch.mul(t, up, out=h.view(rows, k))

            def graph_of(*steps):
                lib.graph_begin()
                try:
                    for step in steps:
                        step()
                except BaseException:
                    lib.graph_destroy(lib.graph_end())
                    raise
                return lib.graph_end()
            sides = {"gated": (lambda: lib.run_operator(ops[0]),), "torch_then_plain": (torch_pass, lambda: lib.run_operator(ops[1])),
                     "torch_pass": (torch_pass,), "plain": (lambda: lib.run_operator(ops[1]),)}
            results = {}
            for key, steps in sides.items():    # every kernel has run once before anything is captured
                for step in steps:
                    step()
                torch.cuda.synchronize()
                results[key] = y.clone()
            # torch's sigmoid is not the definition's to the last bit, so a few elements may land in the neighbouring int8 code
            differ = float((results["gated"] - results["torch_then_plain"]).abs().max() / results["gated"].abs().max())
            graphs = {key: graph_of(*steps) for key, steps in sides.items()}
            h.zero_()
            lib.graph_launch(graphs["torch_pass"])
            lib.graph_synchronize(graphs["torch_pass"])
            assert float(h.abs().sum()) > 0, "the torch pass was not recorded into the graph"
            times = {key: [] for key in sides}
            alone = {"gated": [], "plain": []}
            try:
                for _ in range(args.rounds):
                    for key, graph in graphs.items():
                        times[key].append(lib.graph_time(graph, args.warmup, args.iters) * 1e3)
                    for key in alone:
                        alone[key].append(rows_alone_us(lib, args, torch, x if key == "gated" else h, rows, k, key == "gated"))
            finally:
                for graph in graphs.values():
                    lib.graph_destroy(graph)
            us = {key: statistics.median(v) for key, v in times.items()}
            rows_us = {key: statistics.median(u for u, _ in v) for key, v in alone.items()}
            k_pad = (k + 63) // 64 * 64
            moved = {"gated": rows * (8 * k + k_pad + 8), "plain": rows * (4 * k + k_pad + 8)}
            row = {"form": form, "groups": groups, "rows": rows, "k": k, "n": n,
                   "us": {key: round(v, 2) for key, v in us.items()},
                   "spread": {key: round((max(v) - min(v)) / statistics.median(v), 3) for key, v in times.items()},
                   "chain_over_gated": round(us["torch_then_plain"] / us["gated"], 3),
                   "largest_output_difference_over_largest_output": differ,
                   "rows_alone_us": {key: round(v, 2) for key, v in rows_us.items()},
                   "rows_alone_gb_s": {key: round(moved[key] / rows_us[key] * 1e-3, 1) for key in rows_us},
                   "rows_kernels": {key: v[0][1] for key, v in alone.items()},
                   "kernel": lib.operator_kernel(ops[0]), "rounds": args.rounds, "replays_per_sample": args.iters}
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        finally:
            for op in ops:
                lib.delete_operator(op)
    return rows_out


# the rmsnorm setups: (form, groups, rows, K, N) -- 2880-wide rows at one token, a small batch and a prefill into a dense int8
# layer and into the 32-expert grouped layer (A = 1), and one 8192-wide dense shape
RMSNORM_SHAPES = [("int8", 0, 1, 2880, 2880), ("int8", 0, 64, 2880, 2880), ("int8", 0, 16384, 2880, 2880),
                  ("grouped", 32, 1, 2880, 2880), ("grouped", 32, 64, 2880, 2880), ("grouped", 32, 16384, 2880, 2880),
                  ("int8", 0, 512, 8192, 8192)]


def rmsnorm_rows(lib, args, shapes, rng, gen, np, torch):
    """one record per shape: the rmsnorm setup against what a caller does without it -- the torch residual add + RMSNorm chain
    (seven launches into preallocated tensors, the sum kept as the new residual stream) and the plain setup of a handle with
    the same weights -- each recorded into a graph, the sides in turn. The rmsnorm side writes residual_out to a tensor of its
    own, not in place, so that every replay reads the same residual."""
    rows_out, inf, eps = [], float("inf"), 1e-5
    for form, groups, rows, k, n in shapes:
        g = max(groups, 1)
        x, residual = (torch.randn(rows, k, dtype=torch.float32, device="cuda", generator=gen) for _ in range(2))
        gamma = torch.rand(k, dtype=torch.float32, device="cuda", generator=gen) + 0.5
        s, t, h, s_out = (torch.empty(rows, k, dtype=torch.float32, device="cuda") for _ in range(4))
        m = torch.empty(rows, 1, dtype=torch.float32, device="cuda")
        y = torch.empty(rows * n, dtype=torch.float32, device="cuda")
        ops = []
        try:
            if form == "grouped":
                weights = (groups, k, n, rng.integers(0, 256, size=(g, n, k // 2), dtype=np.uint8),
                           rng.integers(118, 123, size=(g, n, k // 32), dtype=np.uint8), None, -inf, inf)
                create = lib.create_grouped_fully_connected_nc_f32_qd8_mxfp4w
            else:
                weights = (k, n, rng.integers(-128, 128, size=(n, k), dtype=np.int8),
                           rng.uniform(0.005, 0.02, size=n).astype(np.float32), None, -inf, inf)
                create = lib.create_fully_connected_nc_f32_qd8
            for _ in range(2):          # the same weights twice: one handle is set up on normalized rows, the other plain
                ops.append(create(*weights))
            if form == "grouped":
                d_ids = torch.from_numpy(rng.integers(0, groups, rows).astype(np.int32)).cuda()
                lib.setup_grouped_fully_connected_nc_f32_qd8_rmsnorm(ops[0], rows, 1, x, k, gamma, eps, residual, s_out, k, d_ids, y, n)
                lib.setup_grouped_fully_connected_nc_f32_qd8(ops[1], rows, 1, h, k, d_ids, y, n)
            else:
                lib.setup_fully_connected_nc_f32_qd8_rmsnorm(ops[0], rows, x, k, gamma, eps, residual, s_out, k, y, n)
                lib.setup_fully_connected_nc_f32_qd8(ops[1], rows, h, k, y, n)

            def torch_chain():          # seven launches into preallocated tensors: nothing is allocated under a capture
                torch.add(x, residual, out=s)
                torch.mul(s, s, out=t)
                torch.mean(t, dim=1, keepdim=True, out=m)
                m.add_(eps)
                m.rsqrt_()
                torch.mul(s, m, out=t)
                torch.mul(t, gamma, out=h)

            sides = {"rmsnorm": (lambda: lib.run_operator(ops[0]),), "torch_then_plain": (torch_chain, lambda: lib.run_operator(ops[1])),
                     "torch_chain": (torch_chain,), "plain": (lambda: lib.run_operator(ops[1]),)}
            results = {}
            for key, steps in sides.items():    # every kernel has run once before anything is captured
                for step in steps:
                    step()
                torch.cuda.synchronize()
                results[key] = y.clone()
            # torch's mean and rsqrt are not the definition's to the last bit, so a few elements may land in the neighbouring int8 code
            differ = float((results["rmsnorm"] - results["torch_then_plain"]).abs().max() / results["rmsnorm"].abs().max())
            assert bool((s_out == s).all()), "residual_out is the torch sum, bit for bit"
            graphs = {}
            for key, steps in sides.items():
                lib.graph_begin()
                try:
                    for step in steps:
                        step()
                finally:
                    graphs[key] = lib.graph_end()
            h.zero_()
            lib.graph_launch(graphs["torch_chain"])
            lib.graph_synchronize(graphs["torch_chain"])
            assert float(h.abs().sum()) > 0, "the torch chain was not recorded into the graph"
            times = {key: [] for key in sides}
            try:
                for _ in range(args.rounds):
                    for key, graph in graphs.items():
                        times[key].append(lib.graph_time(graph, args.warmup, args.iters) * 1e3)
            finally:
                for graph in graphs.values():
                    lib.graph_destroy(graph)
            us = {key: statistics.median(v) for key, v in times.items()}
            k_pad = (k + 63) // 64 * 64
            row = {"form": form, "groups": groups, "rows": rows, "k": k, "n": n,
                   "us": {key: round(v, 2) for key, v in us.items()},
                   "spread": {key: round((max(v) - min(v)) / statistics.median(v), 3) for key, v in times.items()},
                   "chain_over_rmsnorm": round(us["torch_then_plain"] / us["rmsnorm"], 3),
                   "largest_output_difference_over_largest_output": differ,
                   # what the row launch of either side moves: input, residual and residual_out and the quantized row and its entry,
                   # plus gamma once -- against h alone; and what the torch chain moves in front of the plain side: ten passes over
                   # a [rows][K] float tensor (add 3, square 2, mean 1, the two multiplies 2 each)
                   "row_launch_bytes": {"rmsnorm": rows * (12 * k + k_pad + 8) + 4 * k, "plain": rows * (4 * k + k_pad + 8)},
                   "torch_chain_bytes": rows * 10 * 4 * k,
                   "rows_kernels": {"rmsnorm": lib.dynamic_rows_kernel(ops[0]), "plain": lib.dynamic_rows_kernel(ops[1])},
                   "kernel": lib.operator_kernel(ops[0]), "rounds": args.rounds, "replays_per_sample": args.iters}
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        finally:
            for op in ops:
                lib.delete_operator(op)
    return rows_out


# (experts, A, N, tokens): gpt-oss's routing and hidden size at one token, a small batch and a prefill
MOE_SHAPES = [(32, 4, 2880, 1), (32, 4, 2880, 64), (32, 4, 2880, 16384)]


def moe_rows(lib, args, shapes, rng, gen, np, torch):
    """one record per shape: router and combine against their torch chains, each side recorded into a graph, the sides in turn"""
    rows_out = []
    for e, a, n, tokens in shapes:
        logits = torch.randn(tokens, e, dtype=torch.float32, device="cuda", generator=gen)
        rows = torch.randn(tokens * a, n, dtype=torch.float32, device="cuda", generator=gen)
        ids, w = torch.empty(tokens, a, dtype=torch.int32, device="cuda"), torch.empty(tokens, a, dtype=torch.float32, device="cuda")
        t_values, t_index = torch.empty_like(w), torch.empty(tokens, a, dtype=torch.int64, device="cuda")
        t_ids, t_w = torch.empty_like(ids), torch.empty_like(w)
        y, t_y, t_product = torch.empty(tokens, n, dtype=torch.float32, device="cuda"), torch.empty(tokens, n, dtype=torch.float32, device="cuda"), torch.empty_like(rows)
        ops = {"router": lib.create_topk_router_nc_f32(e, a), "combine": lib.create_weighted_combine_nc_f32(n, a, e)}
        try:
            lib.setup_topk_router_nc_f32(ops["router"], tokens, logits, e, ids, w)
            lib.setup_weighted_combine_nc_f32(ops["combine"], tokens, rows, n, w, ids, y, n)

            def torch_router():
                torch.topk(logits, a, dim=1, out=(t_values, t_index))
                torch.softmax(t_values, dim=1, out=t_w)
                t_ids.copy_(t_index)

            def torch_combine():
                torch.mul(rows.view(tokens, a, n), w.view(tokens, a, 1), out=t_product.view(tokens, a, n))
                torch.sum(t_product.view(tokens, a, n), dim=1, out=t_y)

            sides = {"router": lambda: lib.run_operator(ops["router"]), "torch_router": torch_router,
                     "combine": lambda: lib.run_operator(ops["combine"]), "torch_combine": torch_combine}
            for step in sides.values():         # every kernel has run once before anything is captured
                step()
            torch.cuda.synchronize()
            agree = {"ids_equal": float((ids == t_ids).float().mean()), "weights": float((w - t_w).abs().max()),
                     "combine": float((y - t_y).abs().max() / t_y.abs().max())}
            graphs = {}
            for key, step in sides.items():
                lib.graph_begin()
                try:
                    step()
                finally:
                    graphs[key] = lib.graph_end()
            times = {key: [] for key in sides}
            try:
                for _ in range(args.rounds):
                    for key, graph in graphs.items():
                        times[key].append(lib.graph_time(graph, args.warmup, args.iters) * 1e3)
            finally:
                for graph in graphs.values():
                    lib.graph_destroy(graph)
            us = {key: statistics.median(v) for key, v in times.items()}
            moved = tokens * (a * n * 4 + n * 4 + a * 8)
            row = {"experts": e, "assignments": a, "n": n, "tokens": tokens, "us": {key: round(v, 2) for key, v in us.items()},
                   "spread": {key: round((max(v) - min(v)) / statistics.median(v), 3) for key, v in times.items()},
                   "torch_over_router": round(us["torch_router"] / us["router"], 3),
                   "torch_over_combine": round(us["torch_combine"] / us["combine"], 3),
                   "combine_gb_s": round(moved / us["combine"] * 1e-3, 1), "agreement": agree,
                   "kernels": {key: lib.operator_kernel(op) for key, op in ops.items()}, "rounds": args.rounds,
                   "replays_per_sample": args.iters}
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        finally:
            for op in ops.values():
                lib.delete_operator(op)
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qb4w", action="store_true", help="time the block-wise 4-bit operator against the qc4w one instead")
    ap.add_argument("--qb4w-zp", action="store_true",
                    help="time the block-wise 4-bit operator with zero points against the one without instead")
    ap.add_argument("--qb4w-b32", action="store_true",
                    help="time the 4-bit operator with blocks of 32 against the zero-point one at block size 64 instead")
    ap.add_argument("--mxfp4w", action="store_true",
                    help="time the MXFP4 operator against the signed 4-bit operator with blocks of 32 instead")
    ap.add_argument("--grouped", action="store_true",
                    help="time the grouped MXFP4 operator against one MXFP4 operator per group instead (shapes: GROUPSxBATCHxAxKxN)")
    ap.add_argument("--crossover", action="store_true", help="with --grouped: both product kernels forced around R = 16 * groups")
    ap.add_argument("--gated", action="store_true",
                    help="time the gated setups against a torch element-wise pass and the plain setup instead (shapes: FORMxGROUPSxROWSxKxN, "
                         "FORM grouped or qb4w_b32)")
    ap.add_argument("--rmsnorm", action="store_true",
                    help="time the rmsnorm setups against the torch residual add + RMSNorm chain and the plain setup instead (shapes: "
                         "FORMxGROUPSxROWSxKxN, FORM int8 or grouped)")
    ap.add_argument("--moe", action="store_true",
                    help="time the top-k router and the weighted combine against their torch chains instead (shapes: ExAxNxT)")
    ap.add_argument("--shapes", default=None, help="BATCHxKxN,... instead of the built-in list")
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import qnnpack_amd

    assert torch.cuda.is_available(), "bench_dynamic_fc needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = qnnpack_amd.load()
    lib.initialize()
    if args.gated or args.rmsnorm or args.moe:      # torch's launches are recorded with the library's: both on one stream that can be captured, not the null stream
        torch.cuda.set_stream(torch.cuda.Stream())
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    lib.set_async(False)
    rng = np.random.default_rng(23)
    gen = torch.Generator(device="cuda").manual_seed(23)

    shapes = (GROUPED_SHAPES if args.grouped else GATED_SHAPES if args.gated else RMSNORM_SHAPES if args.rmsnorm else MOE_SHAPES if args.moe else SHAPES) if args.shapes is None else [
        tuple(v if v.isalpha() or "_" in v else int(v) for v in item.split("x")) for item in args.shapes.split(",")]
    rows_out = qb4w_rows(lib, args, shapes, rng, gen, np, torch) if args.qb4w else []
    if args.qb4w_zp:
        rows_out += qb4w_zp_rows(lib, args, shapes, rng, gen, np, torch)
    if args.qb4w_b32:
        rows_out += qb4w_b32_rows(lib, args, shapes, rng, gen, np, torch)
    if args.mxfp4w:
        rows_out += mxfp4w_rows(lib, args, shapes, rng, gen, np, torch)
    if args.grouped:
        rows_out += grouped_rows(lib, args, shapes, rng, gen, np, torch)
    if args.gated:
        rows_out += gated_rows(lib, args, shapes, rng, gen, np, torch)
    if args.rmsnorm:
        rows_out += rmsnorm_rows(lib, args, shapes, rng, gen, np, torch)
    if args.moe:
        rows_out += moe_rows(lib, args, shapes, rng, gen, np, torch)
    for batch, k, n in ([] if args.qb4w or args.qb4w_zp or args.qb4w_b32 or args.mxfp4w or args.grouped or args.gated or args.rmsnorm or args.moe else shapes):
        kernel = rng.integers(-128, 128, size=(n, k), dtype=np.int8)
        scales = rng.uniform(0.005, 0.02, size=n).astype(np.float32)
        bias = rng.standard_normal(n).astype(np.float32)
        in_scale, out_scale = 0.05, 4.0
        nibbles = (kernel >> 4).view(np.uint8) & 15             # [-8, 7]; weight k of a row in bits 4 (k % 2) .. of byte k / 2
        nibbles = np.pad(nibbles, ((0, 0), (0, k % 2)))
        ops = {"dynamic": lib.create_fully_connected_nc_f32_qd8(k, n, kernel, scales, bias, float("-inf"), float("inf")),
               "qc4w": lib.create_fully_connected_nc_f32_qd8_qc4w(k, n, nibbles[:, 0::2] | (nibbles[:, 1::2] << 4), scales, bias,
                                                                  float("-inf"), float("inf")),
               "quantize": lib.create_quantize_nc_f32_q8(k, 128, in_scale, 0, 255),
               "fc": lib.create_fully_connected_nc_q8_per_channel(k, n, 128, in_scale, 128, scales, (kernel.astype(np.int16) + 128).astype(np.uint8),
                                                                  np.zeros(n, np.int32), 128, out_scale, 0, 255),
               "dequantize": lib.create_dequantize_nc_q8_f32(n, 128, out_scale)}
        try:
            x = [torch.randn(batch * k, dtype=torch.float32, device="cuda", generator=gen) for _ in range(args.sets)]
            y = [torch.empty(batch * n, dtype=torch.float32, device="cuda") for _ in range(args.sets)]
            xq = [torch.empty(batch * k, dtype=torch.uint8, device="cuda") for _ in range(args.sets)]
            yq = [torch.empty(batch * n, dtype=torch.uint8, device="cuda") for _ in range(args.sets)]
            lib.setup_fully_connected_nc_f32_qd8(ops["dynamic"], batch, x[0], k, y[0], n)
            lib.setup_fully_connected_nc_f32_qd8(ops["qc4w"], batch, x[0], k, y[0], n)
            lib.setup_quantize_nc_f32_q8(ops["quantize"], batch, x[0], k, xq[0], k)
            lib.setup_fully_connected_nc_q8(ops["fc"], batch, xq[0], k, yq[0], n)
            lib.setup_dequantize_nc_q8_f32(ops["dequantize"], batch, yq[0], n, y[0], n)
            tensors = {"dynamic": (x, y), "qc4w": (x, y), "quantize": (x, xq), "fc": (xq, yq), "dequantize": (yq, y)}
            for op in ops.values():
                lib.run_operator(op)
            kernels = {"rows": lib.dynamic_rows_kernel(ops["dynamic"]), "dynamic": lib.operator_kernel(ops["dynamic"]),
                       "qc4w": lib.operator_kernel(ops["qc4w"]), "fc": lib.operator_kernel(ops["fc"])}
            t = {key: [] for key in ops}
            for _ in range(args.rounds):
                for key, op in ops.items():
                    t[key].append(lib.time_operator_rotating(op, *tensors[key], args.warmup, args.iters))
            us = {key: statistics.median(v) * 1e3 for key, v in t.items()}
            spread = {key: round((max(v) - min(v)) / statistics.median(v), 3) for key, v in t.items()}
            chain = us["quantize"] + us["fc"] + us["dequantize"]
            row = {"batch": batch, "k": k, "n": n, "dynamic_us": round(us["dynamic"], 2), "qc4w_us": round(us["qc4w"], 2),
                   "qc4w_over_dynamic": round(us["qc4w"] / us["dynamic"], 3), "chain_us": round(chain, 2),
                   "quantize_us": round(us["quantize"], 2), "fc_us": round(us["fc"], 2), "dequantize_us": round(us["dequantize"], 2),
                   "chain_over_dynamic": round(chain / us["dynamic"], 3), "spread": spread,
                   "weights_gb_s": round(n * k / us["dynamic"] * 1e-3, 1),
                   "qc4w_weights_gb_s": round(n * k / 2 / us["qc4w"] * 1e-3, 1),
                   "weights_mib": {"dynamic": round(n * k / 2 ** 20, 1), "qc4w": round(n * k / 2 ** 21, 1)}, "tops": round(2.0 * batch * k * n / us["dynamic"] * 1e-6, 1),
                   "kernels": kernels, "sets": args.sets, "rounds": args.rounds, "launches_per_sample": args.iters}
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        finally:
            for op in ops.values():
                lib.delete_operator(op)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": lib.device_info(), "rows": rows_out}, f, indent=1)


if __name__ == "__main__":
    main()
