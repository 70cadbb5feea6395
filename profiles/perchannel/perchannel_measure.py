"""Per-channel against per-tensor operators on the same kernel family and against the automatic dispatch: MobileNetV2 layers
at batch 128 on one MI355X (README.md beside this file has the method and the result).
usage: python profiles/perchannel/perchannel_measure.py [rounds]"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import qnnpack_amd  # noqa: E402
import _perchannel as pc  # noqa: E402

BATCH, SETS, WARMUP, ITERS = 128, 4, 3, 40
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
LAYERS = [("pw 56x56 24->144", 56, dict(gic=24, goc=144)), ("pw 14x14 384->96", 14, dict(gic=384, goc=96)),
          ("pw 7x7 960->320", 7, dict(gic=960, goc=320)),
          ("dw 112x112x32 s1", 112, dict(groups=32, stride=1)), ("dw 56x56x144 s2", 56, dict(groups=144, stride=2)),
          ("dw 14x14x576 s1", 14, dict(groups=576, stride=1))]


def main():
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    lib = qnnpack_amd.load()
    lib.initialize()
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    lib.set_async(False)
    print("device", lib.device_info(), "batch", BATCH, "sets", SETS, "iters", ITERS, "rounds", ROUNDS, flush=True)
    rng = np.random.default_rng(5)
    print(f"{'layer':20s} {'per-channel us':>15s} {'kernel':28s} {'same family us':>15s} {'kernel':24s} {'auto us':>9s} {'kernel':28s} pc/family pc/auto")
    for name, hw, geo in LAYERS:
        dw = "groups" in geo
        groups = geo.get("groups", 1)
        gic, goc = geo.get("gic", 1), geo.get("goc", 1)
        stride = geo.get("stride", 1)
        k = 3 if dw else 1
        pad = 1 if dw else 0
        cin, cout = groups * gic, groups * goc
        ohw = (hw + 2 * pad - k) // stride + 1
        kernel = rng.integers(0, 256, (groups, goc, k, k, gic), dtype=np.uint8)
        bias = rng.integers(-10000, 10001, cout, dtype=np.int32)
        ks = pc.channel_scales(cout)
        head = (pad, pad, pad, pad, k, k, stride, stride, 1, 1, groups, gic, goc, 127, 1.0, 128)
        tail = (kernel, bias, 120, 1.0, 0, 255)
        ins = [torch.randint(0, 256, (BATCH * hw * hw * cin,), dtype=torch.uint8, device="cuda") for _ in range(SETS)]
        outs = [torch.zeros(BATCH * ohw * ohw * cout, dtype=torch.uint8, device="cuda") for _ in range(SETS)]
        family = ("dwconv_kernel", 9) if dw else ("gemm_kernel", 1)
        ops = {}
        for which in ("pc", "family", "auto"):
            lib.set_option(*family) if which == "family" else lib.set_option(family[0], 0)
            if which == "pc":
                op = lib.create_convolution2d_nhwc_q8_per_channel(*head, ks, *tail)
            else:
                op = lib.create_convolution2d_nhwc_q8(*head, float(2.0 ** -8), *tail)
            lib.setup_convolution2d_nhwc_q8(op, BATCH, hw, hw, ins[0], cin, outs[0], cout)
            lib.run_operator(op)
            ops[which] = op
        lib.set_option(family[0], 0)
        times = {which: [] for which in ops}
        for _ in range(ROUNDS):                      # alternating, so that drift hits all three alike
            for which, op in ops.items():
                times[which].append(1000.0 * lib.time_operator_rotating(op, ins, outs, WARMUP, ITERS))
        med = {which: statistics.median(t) for which, t in times.items()}
        names = {which: lib.operator_kernel(op) for which, op in ops.items()}
        print(f"{name:20s} {med['pc']:15.2f} {names['pc']:28s} {med['family']:15.2f} {names['family']:24s} {med['auto']:9.2f} "
              f"{names['auto']:28s} {med['pc'] / med['family']:9.3f} {med['pc'] / med['auto']:7.3f}"
              f"   spread pc {min(times['pc']):.2f}-{max(times['pc']):.2f} family {min(times['family']):.2f}-{max(times['family']):.2f}",
              flush=True)
        for op in ops.values():
            lib.delete_operator(op)


if __name__ == "__main__":
    main()
