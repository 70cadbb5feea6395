"""CPU tier: the kernel choice of the implicit-GEMM dispatcher and the launch plan of the pointwise streaming kernels.
`make -C qnnpack_amd/csrc igemm-plan` builds tests/host_igemm_plan_test.c, plain C, against libqnnpack_gfx950.so itself; the
program calls qnnp_hip_igemm_plan (hip/qnnp_hip.h: the first half of an implicit-GEMM run, which launches nothing and needs
no device) on a fixed list of argument blocks and prints one line per case: the status, the dispatcher's choice and, for a
streaming kernel, the kernel a run would report and every field of its launch that is not zero. The output must equal tests/golden/igemm_plans.txt line for line. The plan decides speed, not
bytes -- which kernel, which flavour, the grid, the LDS, the channel columns -- so the parity tests cannot see it change. The
file was recorded while one translation unit held every streaming kernel and its launchers filled the plan in place of
launching; a line that differs means a layer is launched differently."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "igemm_plans.txt")
SHAPES = os.path.join(ROOT, "tests", "golden", "reference_bench_shapes.json")
# measurement knobs that enter the plan (q8pwconv.hip), and everything the library reads under its own prefix
KNOBS = ("QNNP_PW_BLOCKS", "QNNP_PW_ABL", "QNNP_PW_NBP", "QNNP_GW_SPLITK")
# what the automatic path reaches from a 1x1, fully connected or 3-channel first layer
AUTO_KERNELS = ("Generic", "Rows16", "Rows32", "C3", "Mid", "U", "Pw", "LongK", "Gw", "Big", "BigX")


def test_every_igemm_plan_is_the_recorded_one():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "igemm-plan"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "host", "host_igemm_plan_test")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS and not k.startswith("QNNP_GFX950_")}
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    got = run.stdout.splitlines()
    want = open(GOLDEN).read().splitlines()
    for number, (g, w) in enumerate(zip(got, want), 1):
        assert g == w, f"line {number}:\n  got  {g}\n  want {w}"
    assert len(got) == len(want), (len(got), len(want))

    # ---- what the record has to show ----
    cases = {line.split()[0]: dict(f.split("=", 1) for f in line.split()[1:]) for line in want}
    assert len(cases) == len(want), "case names are unique"
    ok = {name: f for name, f in cases.items() if f["rc"] == "0"}

    def some(flags=(), **fields):     # the cases with these fields (a field that is not printed is 0) and these flags on
        return [name for name, f in ok.items() if all(f.get(k, "0") == str(v) for k, v in fields.items()) and
                set(flags) <= set(f.get("flags", "").split("+"))]

    def without(names, flag):
        return [n for n in names if flag not in ok[n].get("flags", "").split("+")]

    # every pointwise / fully connected layer and every 3-channel first layer of the reference's networks, at batch 1 and
    # 128, on the automatic path
    lists = json.load(open(SHAPES))["lists"]
    auto = set()
    for shapes in lists.values():
        for h, w, kh, kw, s, d, g, gic, goc in shapes:
            for tail in ("b1", "b128"):
                if kh == 1 and kw == 1:
                    name = f"net_{h}x{w}_s{s}_g{g}_{gic}to{goc}_{tail}"
                elif g == 1 and gic == 3:
                    name = f"net_first_{h}x{w}_k{kh}_s{s}_d{d}_3to{goc}_{tail}"
                else:
                    continue
                assert name in ok, name
                auto.add(ok[name]["kernel"])
    auto |= {f["kernel"] for name, f in ok.items() if "_auto_" in name or name.startswith("first_dilated")}
    assert auto == set(AUTO_KERNELS), sorted(auto)

    # the stream kernel
    assert {f["kb"] for f in (ok[n] for n in without(some(family="stream", kvec=16), "d2s"))} >= {str(kb) for kb in range(1, 9)}
    assert {f["kb"] for f in (ok[n] for n in some(family="stream", kvec=8))} >= {"1", "3", "8"}
    assert some(family="stream", flags=["d2s"])
    assert any(n.startswith("stream_dword_stores") for n in some(family="stream", store_mode=1))
    # the staged kernel: whole rows dense and strided, columns of 2 / 4 / 8, dense8, the strided 1x1 form, both widths
    assert "staged_whole_dense_112x112x16to96_b128" in without(some(family="staged", nbp=3, lds=16384), "dense8")
    assert "staged_whole_strided_112x112x16to96_b128" in without(some(family="staged", nbp=3), "dense8")
    columns = [ok[n] for n in some(family="staged") if ok[n]["grid"].split("x")[1] != "1"]
    assert {f["nbp"] for f in columns} >= {"2", "4", "8"}
    assert some(family="staged", flags=["dense8"])
    assert "staged_strided1x1_56x56_s2_64to128_b128" in some(family="staged")
    assert some(family="staged", kvec=16) and some(family="staged", kvec=8)
    # the long-K kernel
    for kbmax in (12, 20, 32):
        assert some(family="longk", kb=kbmax), kbmax
    assert some(family="longk", kb=20, flags=["pf"])
    assert without(some(family="longk", kb=20), "pf") and without(some(family="longk", kb=12), "pf")
    assert [n for n in some(family="longk") if ok[n]["grid"].endswith("x1")]
    assert [n for n in some(family="longk") if not ok[n]["grid"].endswith("x1")]
    # the global-weights kernels and the 3-channel streaming kernels
    assert some(family="gw") and some(family="gwk", depth=4) and some(family="gwk", depth=8)
    assert some(family="c3", flags=["staged"]) and without(some(family="c3"), "staged")
    # flavours: a residual, a table that folds; a table that does not, for residency and for the LDS budget
    for family in ("stream", "staged", "longk", "gw", "gwk"):
        assert without(some(family=family, flags=["res"], folded="residual"), "tab"), family
        assert without(some(family=family, flags=["tab"], folded="table"), "res"), family
    for family in ("stream", "staged", "longk"):
        for reason in ("residency", "budget"):
            names = [n for n in without(some(family=family, folded=0), "tab") if n.startswith(f"flavour_{family}_table_{reason}")]
            assert names, (family, reason)
    assert "folded" not in ok["flavour_residual_other_stride_56x56x144to48_b128"]
    assert "folded" not in ok["flavour_residual_misaligned_56x56x144to48_b128"]
    assert cases["flavour_table_with_residual_refused"]["rc"] != "0"
    # alignments, and the refusals
    assert {f["store_mode"] for f in ok.values()} == {"0", "1", "2"}
    assert {f["vec"] for f in ok.values()} >= {"16", "8", "4"}
    refused = {name for name, f in cases.items() if f["rc"] != "0"}
    assert refused >= {"forced5_k512_refused", "forced6_in8_refused", "forced7_pointwise_refused", "forced9_k128_refused",
                       "forced5_per_channel_refused", "stream_d2s_auto_refused"}, refused
