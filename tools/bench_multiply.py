"""Measurement aid: the multiply operator (hip/q8mul.hip, kernel q8_mul_x16) as the scale of a squeeze-and-excite block
at batch 128, 56 x 56 x 96 on the MI355X -- broadcast (one row of `b` per image), not in place -- against the element-wise
add (q8_vadd_flat) on the same tensor and the chip's copy kernel, all in one process.

The three operands of each operator are checked once against the oracle (a sample of rows), then the two operators are
timed, interleaved and --rounds times over, with qnnp_gfx950_time_operator_rotating: a hipGraph of launches replayed,
median of five replays, over (a, product) buffer pairs rotated so that a buffer comes back only after >= 512 MiB of other
traffic, past the 256 MiB Infinity Cache. The median round is reported.

GB/s counts what each operator has to move through HBM per launch: the multiply `a` read + product written (its `b` is
128 rows of 96 bytes and stays in L2); the add a + b read + sum written. The second operand is not rotated by the timing
call, so the add's `b` (38.5 MB) can stay in the Infinity Cache between launches: its figure is an upper bound. The copy
kernel is roofline.hbm_copy_kernel_gbs of bench.py --full: the better of the plain and the streaming form over 1 GiB.

    python tools/bench_multiply.py [--batch 128] [--iters 20] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--pixels", type=int, default=56 * 56)
    ap.add_argument("--channels", type=int, default=96)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import qnnpack_amd
    import _multiply as mul
    import _pointwise as pw

    assert torch.cuda.is_available(), "bench_multiply needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = qnnpack_amd.load()
    lib.initialize()
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    lib.set_async(False)
    gen = torch.Generator(device="cuda").manual_seed(11)

    c, rows = args.channels, args.batch * args.pixels
    nbytes = rows * c
    nsets = max(1, -(-(512 << 20) // (2 * nbytes)))
    iters = max(args.iters, nsets)
    ins = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(nsets)]
    outs = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
    gate = torch.randint(0, 256, (args.batch * c,), dtype=torch.uint8, device="cuda", generator=gen)
    other = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=gen)

    q = mul.MID
    add_case = pw.AddCase("bench", rows, c)
    m_op = lib.create_multiply_nc_q8(c, *q.args())
    a_op = lib.create_add_nc_q8(c, add_case.a_zp, add_case.a_scale, add_case.b_zp, add_case.b_scale, add_case.y_zp,
                                add_case.y_scale, 0, 255, 0)
    try:
        lib.setup_multiply_nc_q8(m_op, args.batch, args.pixels, ins[0], c, gate, c, outs[0], c)
        lib.run_operator(m_op)
        torch.cuda.synchronize()
        m_kernel = lib.operator_kernel(m_op)
        # the first, a middle and the last image against the oracle
        host_a, host_g, host_y = ins[0].cpu().numpy(), gate.cpu().numpy(), outs[0].cpu().numpy()
        per = args.pixels * c
        for image in sorted({0, args.batch // 2, args.batch - 1}):
            s = mul.Shape(c, 1, args.pixels)
            want = mul.expected(q, s, host_a[image * per:(image + 1) * per], host_g[image * c:(image + 1) * c],
                                np.zeros(per, np.uint8))
            assert np.array_equal(host_y[image * per:(image + 1) * per], want), f"image {image} differs from the oracle"
        lib.setup_add_nc_q8(a_op, rows, ins[0], c, other, c, outs[0], c)
        lib.run_operator(a_op)
        torch.cuda.synchronize()
        a_kernel = lib.operator_kernel(a_op)
        small = pw.AddCase("bench", args.pixels, c)
        want = pw.add_expected(small, host_a[:per], other.cpu().numpy()[:per])
        assert np.array_equal(outs[0].cpu().numpy()[:per], want), "the add differs from the oracle"
        t = {"mul": [], "add": []}
        for _ in range(args.rounds):
            t["mul"].append(lib.time_operator_rotating(m_op, ins, outs, args.warmup, iters))
            t["add"].append(lib.time_operator_rotating(a_op, ins, outs, args.warmup, iters))
    finally:
        lib.delete_operator(m_op)
        lib.delete_operator(a_op)
    del ins, outs
    torch.cuda.empty_cache()
    dbg = qnnpack_amd.load_debug()
    copy_plain = dbg.copy_probe(False, 1024, 5)
    copy_streaming = dbg.copy_probe(False, 1024, 5, streaming=True)

    us = {k: statistics.median(v) * 1e3 for k, v in t.items()}
    moved = {"mul": 2 * nbytes, "add": 3 * nbytes}
    gbs = {k: moved[k] / (us[k] * 1e-6) / 1e9 for k in us}
    result = {
        "shape": f"batch {args.batch}, {args.pixels} pixels, {c} channels", "output_bytes": nbytes, "buffer_sets": nsets,
        "launches": iters, "rounds": args.rounds, "mul_kernel": m_kernel, "add_kernel": a_kernel,
        "mul_us": round(us["mul"], 2), "add_us": round(us["add"], 2),
        "mul_GBps": round(gbs["mul"], 1), "add_GBps": round(gbs["add"], 1),
        "mul_ns_per_output_MB": round(us["mul"] * 1e3 / (nbytes / 1e6), 2),
        "add_ns_per_output_MB": round(us["add"] * 1e3 / (nbytes / 1e6), 2),
        "mul_over_add_time": round(us["mul"] / us["add"], 3),
        "hbm_copy_kernel_gbs": round(max(copy_plain, copy_streaming), 1), "hbm_copy_kernel_plain_policy_gbs": round(copy_plain, 1),
        "rounds_mul_us": [round(v * 1e3, 2) for v in t["mul"]], "rounds_add_us": [round(v * 1e3, 2) for v in t["add"]],
    }
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
