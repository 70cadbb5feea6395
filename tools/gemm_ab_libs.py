#!/usr/bin/env python3
"""Same-process, interleaved A/B of one fully connected operator across BUILDS of the library (tools/gemm_ab.py compares
kernel structures inside one build; this compares, say, the parent commit's build with the working tree's, or measurement
builds under different QNNP_GFX950_ABLATE / QNNP_C16_OPT values). Every build is loaded beside the others (RTLD_LOCAL: each
keeps its own state and kernels), creates the operator on the same operands, and is timed as a 32-launch hipGraph replayed
for >= 150 ms per round, the variants in alternating order round by round.

    python tools/gemm_ab_libs.py --variant parent=build_alt/parent/libqnnpack_gfx950.so --variant new=qnnpack_amd/libqnnpack_gfx950.so
    python tools/gemm_ab_libs.py --variant abl8=build_abl/libqnnpack_gfx950.so,ABLATE=8 ...      (measurement builds)

Prints one JSON line per variant (median / min / max over the rounds and every round's value) and one summary line per
variant after the first: its gain over the first in every round, and the first's own round-to-round spread (the noise
floor). Variants without ABLATE must give the first variant's bytes."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", action="append", required=True, help="label=path[,ABLATE=n][,OPT=n]")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--code", type=int, default=23, help='"gemm_kernel" option (0: the automatic choice)')
    ap.add_argument("--kzp", type=int, default=127)
    ap.add_argument("--scale", type=float, default=0.75)
    args = ap.parse_args()
    import torch
    from qnnpack_amd.binding import Gfx950Library
    torch.cuda.set_device(0); torch.zeros(1, device="cuda")
    M, N, K = args.m, args.n, args.k
    rng = np.random.default_rng(0x51A0 + 2)
    w = rng.integers(0, 256, size=(N, K), dtype=np.uint8)
    bias = rng.integers(-10000, 10001, size=N, dtype=np.int32)
    gen = torch.Generator(device="cuda"); gen.manual_seed(0x51A0)
    a = torch.randint(0, 256, (M * K,), dtype=torch.uint8, device="cuda", generator=gen)
    libs, variants = {}, []
    for spec in args.variant:
        label, rest = spec.split("=", 1)
        parts = rest.split(",")
        path = os.path.abspath(parts[0])
        env = dict(p.split("=", 1) for p in parts[1:])
        if path not in libs:
            lib = Gfx950Library(path)
            lib.initialize(); lib.set_stream(torch.cuda.current_stream().cuda_stream)
            libs[path] = lib
        variants.append({"label": label, "lib": libs[path], "env": env})

    def with_env(v):
        for key, name in (("ABLATE", "QNNP_GFX950_ABLATE"), ("OPT", "QNNP_C16_OPT")):
            os.environ.pop(name, None)
            if key in v["env"]:
                os.environ[name] = v["env"][key]

    ref = None
    for v in variants:                               # the launcher reads the measurement knobs at every launch / capture
        lib = v["lib"]
        with_env(v)
        lib.set_option("gemm_kernel", args.code)
        v["op"] = lib.create_fully_connected_nc_q8(K, N, 127, 0.75, args.kzp, 1.0, w, bias, 127, 0.75 / args.scale, 1, 254)
        lib.set_option("gemm_kernel", 0)
        v["out"] = torch.zeros(M * N, dtype=torch.uint8, device="cuda")
        lib.setup_fully_connected_nc_q8(v["op"], M, a, K, v["out"], N)
        lib.run_operator(v["op"])
        torch.cuda.synchronize()
        v["kernel"] = lib.operator_kernel(v["op"])
        if "ABLATE" not in v["env"]:
            if ref is None:
                ref = v["out"]
            else:
                assert torch.equal(v["out"], ref), f"variant {v['label']} differs from the first"
    for v in variants:
        lib = v["lib"]
        with_env(v)
        lib.set_async(True)
        lib.graph_begin()
        for _ in range(32):
            lib.run_operator(v["op"])
        v["graph"] = lib.graph_end()
        v["times"] = []
    for v in variants:                               # sustained-clock warm-up
        v["lib"].graph_time(v["graph"], 2, 40)
    for r in range(args.rounds):
        for v in (variants if r % 2 == 0 else variants[::-1]):
            v["times"].append(v["lib"].graph_time(v["graph"], 1, 80) / 32.0 * 1e3)
    shape = f"{M}x{N}x{K}"
    for v in variants:
        t = sorted(v["times"])
        print(json.dumps({"variant": v["label"], "env": v["env"], "shape": shape, "kzp": args.kzp, "scale": args.scale, "kernel": v["kernel"],
                          "us_median": round(t[len(t) // 2], 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2),
                          "us_rounds": [round(x, 2) for x in v["times"]]}), flush=True)
    base = variants[0]
    spread = max(base["times"]) - min(base["times"])
    for v in variants[1:]:
        gains = [b - x for b, x in zip(base["times"], v["times"])]
        g = sorted(gains)
        print(json.dumps({"variant": v["label"], "against": base["label"], "shape": shape, "gain_us_median": round(g[len(g) // 2], 2),
                          "gain_us_min": round(g[0], 2), "gain_us_max": round(g[-1], 2), "faster_in_rounds": sum(x > 0 for x in gains),
                          "rounds": len(gains), "spread_of_first_us": round(spread, 2)}), flush=True)
    for v in variants:
        v["lib"].graph_destroy(v["graph"]); v["lib"].delete_operator(v["op"])


if __name__ == "__main__":
    main()
