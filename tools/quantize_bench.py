"""Measurement aid: the quantize and dequantize operators (hip/f32q8.hip) at the two ends of a network on the MI355X,
against the chip's copy kernel and against torch's own quantizer on the same box, all in one process.

Shapes: quantize planar (NCHW float -> NHWC uint8) 128 x 3 x 224 x 224 and 128 x 3 x 512 x 512; dequantize planar
(NHWC uint8 -> NCHW float) 8 x 21 x 512 x 512; dequantize rows 128 x 1000.

Each operator's first launch is checked against the numpy statement of tests/_quantize.py (the first and the last image),
then timed --rounds times with qnnp_gfx950_time_operator_rotating: a hipGraph of launches replayed, median of five
replays, over (input, output) buffer pairs rotated so that a buffer comes back only after >= 512 MiB of other traffic,
past the 256 MiB Infinity Cache (the 128 x 1000 rows are 640 KB a pair: at most --max-sets pairs, so that one stays
cache-resident and is a launch-latency figure). The median round is reported. GB/s counts 5 bytes per element: 4 on the
float side, 1 on the byte side.

torch: quantize = x.permute(0, 2, 3, 1).contiguous() then torch.quantize_per_tensor(..., torch.quint8); dequantize =
.dequantize() then .permute(0, 3, 1, 2).contiguous() (rows: .dequantize() alone), timed with events over the same
rotation, median of the rounds. Where this torch build has no quantized GPU backend, the same arithmetic in plain tensor
operations is timed instead and the record says so. The copy kernel is roofline.hbm_copy_kernel_gbs of bench.py --full.

    python tools/quantize_bench.py [--iters 20] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, direction, planar, batch, channels, height, width)
SHAPES = [("quantize_planar_128x3x224x224", "quantize", True, 128, 3, 224, 224),
          ("quantize_planar_128x3x512x512", "quantize", True, 128, 3, 512, 512),
          ("dequantize_planar_8x21x512x512", "dequantize", True, 8, 21, 512, 512),
          ("dequantize_rows_128x1000", "dequantize", False, 128, 1000, 1, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-sets", type=int, default=32)
    ap.add_argument("--only", default=None, help="substring of the shape names to run")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import qnnpack_amd
    import _quantize as fq

    assert torch.cuda.is_available(), "quantize_bench needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = qnnpack_amd.load()
    lib.initialize()
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    lib.set_async(False)
    gen = torch.Generator(device="cuda").manual_seed(7)
    q = fq.MID

    def torch_time(fn, nsets, iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for k in range(min(2, nsets)):
            fn(k)
        rounds = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            start.record()
            for i in range(iters):
                fn(i % nsets)
            stop.record()
            torch.cuda.synchronize()
            rounds.append(start.elapsed_time(stop) / iters * 1e3)
        return statistics.median(rounds)

    results = []
    for name, direction, planar, batch, c, h, w in SHAPES:
        if args.only and args.only not in name:
            continue
        pixels = h * w
        n = batch * c * pixels
        nsets = min(args.max_sets, max(1, -(-(512 << 20) // (5 * n))))
        iters = max(args.iters, nsets)
        floats = [(torch.rand(n, device="cuda", generator=gen) * 5.0 - 2.2) for _ in range(nsets)]
        qbytes = [torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(nsets)]
        if direction == "quantize":
            op = lib.create_quantize_nc_f32_q8(c, *q.args())
            ins, outs = floats, qbytes
        else:
            op = lib.create_dequantize_nc_q8_f32(c, q.zp, q.scale)
            ins, outs = qbytes, floats
        try:
            if direction == "quantize":
                lib.setup_quantize_nchw_f32_nhwc_q8(op, batch, pixels, ins[0], outs[0], c)
            elif planar:
                lib.setup_dequantize_nhwc_q8_nchw_f32(op, batch, pixels, ins[0], c, outs[0])
            else:
                lib.setup_dequantize_nc_q8_f32(op, batch, ins[0], c, outs[0], c)
            host_in = ins[0].cpu().numpy()
            lib.run_operator(op)
            torch.cuda.synchronize()
            kernel = lib.operator_kernel(op)
            host_out = outs[0].cpu().numpy()
            per = c * pixels
            for image in sorted({0, batch - 1}):
                s = fq.Planar(c, pixels, 1)
                piece_in, piece_out = host_in[image * per:(image + 1) * per], host_out[image * per:(image + 1) * per]
                if direction == "quantize":
                    want = fq.quantize_planar_expected(q, s, piece_in, np.zeros(per, np.uint8))
                    assert np.array_equal(piece_out, want), f"{name}: image {image} differs from the definition"
                else:
                    want = fq.dequantize_planar_expected(q, s, piece_in) if planar else fq.dequantize(piece_in, q)
                    assert np.array_equal(fq.bits(piece_out), fq.bits(want)), f"{name}: image {image} differs from the definition"
            rounds = [lib.time_operator_rotating(op, ins, outs, args.warmup, iters) * 1e3 for _ in range(args.rounds)]
        finally:
            lib.delete_operator(op)

        # torch on the same buffers
        torch_form = "quantize_per_tensor"
        try:
            if direction == "quantize":
                def fn(k):
                    return torch.quantize_per_tensor(floats[k].view(batch, c, h, w).permute(0, 2, 3, 1).contiguous(),
                                                     q.scale, q.zp, torch.quint8)
            else:
                qt = [torch._make_per_tensor_quantized_tensor(t.view(batch, h, w, c), q.scale, q.zp) for t in qbytes]

                def fn(k):
                    y = qt[k].dequantize()
                    return y.permute(0, 3, 1, 2).contiguous() if planar else y
            fn(0)
            torch.cuda.synchronize()
        except Exception as e:     # no quantized GPU backend in this torch build
            torch_form = f"plain tensor operations ({type(e).__name__}: quantized tensors unavailable on this device)"
            inv = 1.0 / q.scale
            if direction == "quantize":
                def fn(k):
                    x = floats[k].view(batch, c, h, w).permute(0, 2, 3, 1).contiguous()
                    return torch.clamp(torch.round(x * inv) + q.zp, q.qmin, q.qmax).to(torch.uint8)
            else:
                def fn(k):
                    y = (qbytes[k].view(batch, h, w, c).to(torch.float32) - q.zp) * q.scale
                    return y.permute(0, 3, 1, 2).contiguous() if planar else y
        torch_us = torch_time(fn, nsets, iters)
        del floats, qbytes, ins, outs
        torch.cuda.empty_cache()

        us = statistics.median(rounds)
        results.append({
            "shape": name, "kernel": kernel, "elements": n, "buffer_sets": nsets, "launches": iters,
            "us": round(us, 2), "rounds_us": [round(v, 2) for v in rounds],
            "GBps_at_5_bytes_per_element": round(5 * n / (us * 1e-6) / 1e9, 1),
            "torch_form": torch_form, "torch_us": round(torch_us, 2), "torch_over_operator_time": round(torch_us / us, 2),
        })
        print(json.dumps(results[-1]), flush=True)

    dbg = qnnpack_amd.load_debug()
    copy_plain = dbg.copy_probe(False, 1024, 5)
    copy_streaming = dbg.copy_probe(False, 1024, 5, streaming=True)
    record = {"operators": results, "hbm_copy_kernel_gbs": round(max(copy_plain, copy_streaming), 1),
              "hbm_copy_kernel_plain_policy_gbs": round(copy_plain, 1), "torch": torch.__version__}
    print(json.dumps({k: v for k, v in record.items() if k != "operators"}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
