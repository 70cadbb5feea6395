"""CPU tier of the operators' shared create / setup lifecycle: tests/host_asan_lifecycle_test.c asks every public create
and setup the same questions (before qnnp_initialize, bad arguments outside and inside a graph capture, NULL and foreign
handles, batch 0, failing staging allocations, the NC overlap rules) and compares the statuses with one table, under
AddressSanitizer + UBSan against the HIP stub (Makefile target asan-lifecycle).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lifecycle_of_every_operator_matches_the_recorded_statuses_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-lifecycle"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "asan", "host_asan_lifecycle_test")
    # the ASan runtime is linked statically (Makefile asan-lifecycle), so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-lifecycle-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]
