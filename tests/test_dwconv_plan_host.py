"""CPU tier: the launch plan of the depthwise kernels. `make -C qnnpack_amd/csrc dwconv-plan` builds
tests/host_dwconv_plan_test.c, plain C, against libqnnpack_gfx950.so itself; the program calls qnnp_hip_dwconv_plan
(hip/qnnp_hip.h: the first half of a depthwise run, which launches nothing and needs no device) on a fixed list of
argument blocks and prints one line per case: the status, the kernel a run would report and every field of the plan. The
output must equal tests/golden/dwconv_plans.txt line for line. The plan decides speed, not bytes -- rows per segment,
bands, slabs, the staged band -- so the parity tests cannot see it change. The file was recorded while one translation
unit held every depthwise kernel with its plan_* function; a line that differs means a layer is launched differently."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dwconv_plans.txt")
# measurement knobs that enter the plan (dwconv_params.h, q8dwlds.hip), and those that only measurement builds read
# (q8dwrow.hip, q8dwcol.hip, q8dwmfma16.hip)
KNOBS = ("QNNP_GFX950_DW_COL_ROWS", "QNNP_GFX950_DW_LDS_KB", "QNNP_DW_ROW_WAVES", "QNNP_GFX950_DW_COL_QUAD", "QNNP_DW_M16_TN")
PLAN_KERNELS = ("kPlanDirect", "kPlanLds33", "kPlanLds55", "kPlanRow", "kPlanMfma", "kPlanMfmaLds", "kPlanCol", "kPlanCol5",
                "kPlanM16", "kPlanDirect4", "kPlanRowAny")


def test_every_depthwise_plan_is_the_recorded_one():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "dwconv-plan"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "host", "host_dwconv_plan_test")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    got = run.stdout.splitlines()
    want = open(GOLDEN).read().splitlines()
    for number, (g, w) in enumerate(zip(got, want), 1):
        assert g == w, f"line {number}:\n  got  {g}\n  want {w}"
    assert len(got) == len(want), (len(got), len(want))
    # what the record has to show: every kernel of the plan, both staging widths, the three store modes, and a refusal
    # of every forced code
    fields = [dict(f.split("=", 1) for f in line.split()[1:]) for line in want]
    assert {f["kernel"] for f in fields} >= set(PLAN_KERNELS)
    assert {f["vec16"] for f in fields if f["rc"] == "0"} == {"0", "1"}
    assert {f["store_mode"] for f in fields if f["rc"] == "0"} == {"0", "1", "2"}
    refused = {line.split()[0].split("_")[0] for line, f in zip(want, fields) if f["rc"] != "0"}
    assert refused >= {f"forced{code}" for code in range(1, 10)}, refused
