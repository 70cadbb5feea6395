"""CPU tier: what every operator of the host tier hands to its kernel entry point. `make -C qnnpack_amd/csrc
asan-launch-args` builds tests/host_launch_args_test.c with the host sources against tests/hip_stub.c under
AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program; it walks a fixed list of operators on host
tensors and on stub "device" tensors, and the stub writes one line per kernel launch: the entry point, every field of its
argument block (pointers by name, never by address) and the status it returned. The log must equal
tests/golden/launch_args.txt line for line. That file was recorded from the run path as it was while one switch in
operator-run.c built every block; a line that differs means a launch changed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_args.txt")


def test_every_launch_hands_over_the_recorded_argument_block(tmp_path):
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-launch-args"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "asan", "host_launch_args_test")
    log = tmp_path / "launch_args.txt"
    # the ASan runtime is linked statically (Makefile asan-launch-args), so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe, str(log)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "launch-args-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-6000:]
    got = log.read_text().splitlines()
    want = open(GOLDEN).read().splitlines()
    for number, (g, w) in enumerate(zip(got, want), 1):
        assert g == w, f"line {number}:\n  got  {g}\n  want {w}"
    assert len(got) == len(want), (len(got), len(want))
