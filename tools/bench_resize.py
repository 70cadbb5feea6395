"""Measurement aid: the bilinear resize operator (hip/u8resize.hip) at batch 128 on the MI355X on four shapes -- two
segmentation-head upsamplings, a x2 feature-map upsampling and an input-pipeline downsampling -- against the chip's copy
kernel, all in one process:

    33 x 33 x 256  -> 129 x 129 x 256                    u8_resize_x16   (DeepLab, x4 upsampling of the ASPP output)
    65 x 65 x 21   -> 513 x 513 x 21, align corners      u8_resize_x4    (the class map at the end of a segmentation head)
    28 x 28 x 96   -> 56 x 56 x 96                       u8_resize_x16   (an LR-ASPP merge)
    256 x 256 x 3  -> 224 x 224 x 3                      u8_resize_x1    (a decoded image in front of the first convolution)

The first and the last image of each shape are checked once against the definition (tests/_resize.py), then the shapes
are timed, interleaved and --rounds times over, with qnnp_gfx950_time_operator_rotating: a hipGraph of launches replayed,
median of five replays, over (input, output) buffer pairs rotated so that a buffer comes back only after >= 512 MiB of
other traffic, past the 256 MiB Infinity Cache. The median round is reported.

Bytes are the algorithmic ones: the input read once + the output written once. An upsampling re-reads every input pixel
for several output pixels; those re-reads are served by L1 / L2 and are not counted. The copy kernel is
roofline.hbm_copy_kernel_gbs of bench.py --full: the better of the plain and the streaming form over 1 GiB (bytes read +
written).

    python tools/bench_resize.py [--batch 128] [--iters 20] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [   # (input height, input width, output height, output width, channels, align corners)
    (33, 33, 129, 129, 256, False),
    (65, 65, 513, 513, 21, True),
    (28, 28, 56, 56, 96, False),
    (256, 256, 224, 224, 3, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import qnnpack_amd
    import _resize as rs

    assert torch.cuda.is_available(), "bench_resize needs the MI355X"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = qnnpack_amd.load()
    lib.initialize()
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    lib.set_async(False)
    gen = torch.Generator(device="cuda").manual_seed(13)

    rows = []
    times = {}
    state = []
    try:
        for ih, iw, oh, ow, ch, align in SHAPES:
            c = rs.Case(args.batch, ih, iw, oh, ow, ch, align=align)
            nsets = max(2, -(-(512 << 20) // (c.in_span + c.out_span)))
            iters = max(args.iters, nsets)
            ins = [torch.randint(0, 256, (c.in_span,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(nsets)]
            outs = [torch.empty(c.out_span, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
            op = lib.create_resize_bilinear2d_nhwc_u8(ch, c.flags)
            state.append((c, op, ins, outs, iters))
            lib.setup_resize_bilinear2d_nhwc_u8(op, *c.setup_args(ins[0], outs[0]))
            lib.run_operator(op)
            torch.cuda.synchronize()
            # the first and the last image against the definition
            in_image, out_image = ih * iw * ch, oh * ow * ch
            for image in (0, args.batch - 1):
                x = ins[0][image * in_image:(image + 1) * in_image].cpu().numpy().reshape(1, ih, iw, ch)
                got = outs[0][image * out_image:(image + 1) * out_image].cpu().numpy()
                assert np.array_equal(got, rs.resize(x, oh, ow, align).reshape(-1)), f"{c}: image {image} differs from the definition"
            times[str(c)] = []
        for _ in range(args.rounds):
            for c, op, ins, outs, iters in state:
                times[str(c)].append(lib.time_operator_rotating(op, ins, outs, args.warmup, iters))
        for c, op, ins, outs, iters in state:
            t = times[str(c)]
            us = statistics.median(t) * 1e3
            moved = c.in_span + c.out_span
            rows.append({
                "shape": f"{c.in_h}x{c.in_w}x{c.channels} -> {c.out_h}x{c.out_w}x{c.channels}" + (", align corners" if c.align else ""),
                "batch": args.batch, "kernel": lib.operator_kernel(op), "buffer_sets": len(ins), "launches": iters,
                "us": round(us, 2), "rounds_us": [round(v * 1e3, 2) for v in t],
                "input_bytes": c.in_span, "output_bytes": c.out_span, "algorithmic_bytes": moved,
                "TBps": round(moved / (us * 1e-6) / 1e12, 3),
                "ns_per_output_MB": round(us * 1e3 / (c.out_span / 1e6), 1),
            })
    finally:
        for _, op, _, _, _ in state:
            lib.delete_operator(op)
    del state, ins, outs
    torch.cuda.empty_cache()
    dbg = qnnpack_amd.load_debug()
    copy_plain = dbg.copy_probe(False, 1024, 5)
    copy_streaming = dbg.copy_probe(False, 1024, 5, streaming=True)
    copy = max(copy_plain, copy_streaming)
    for r in rows:
        r["fraction_of_copy_kernel"] = round(r["TBps"] * 1e3 / copy, 3)
    result = {"rows": rows, "rounds": args.rounds, "hbm_copy_kernel_gbs": round(copy, 1),
              "hbm_copy_kernel_plain_policy_gbs": round(copy_plain, 1)}
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
