"""CPU tier of the 256 x 256 16x16x64 GEMM's K-pair staging: the index maps and the LDS-DMA schedule the kernel calls
(qnnpack_amd/csrc/hip/gemm256x_map.h) are proven on the host by tests/gemm256x_map_check.cc, a stand-alone program
built with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer:

1. the DMA map of an activation pair is a bijection of rows x chunks onto the pair slot's 16-byte cells, a wave
   instruction writes 1 KiB of contiguous LDS, eight consecutive lanes fetch one row's 128 bytes;
2. the fragment reads return the (row, chunk) the MFMA operand layout requires;
3. every ds_read_b128 lane group touches sixteen different bank quads;
4. for every tile count from 8 to 40, rows in {1, 255, 256, 257}, dense, strided and table rows: no lane reads outside
   its row (the unpaired last tile of an odd count included), every piece is issued once and two K tiles ahead of the
   barrier that needs it, every counted wait covers what the reads behind its barrier need, and no slot is refilled
   before the barrier behind its last read.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR_DIR = os.path.join(ROOT, "qnnpack_amd", "csrc", "hip")
SRC = os.path.join(ROOT, "tests", "gemm256x_map_check.cc")


def test_gemm256x_maps_and_schedule_hold_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gemm256x_map_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-static-libasan", "-I", HDR_DIR, SRC, "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    # the ASan runtime is linked statically, so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and "all checks hold" in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
