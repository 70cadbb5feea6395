"""CPU tier of channel shuffle (qnnp_*_channel_shuffle_nc_x8) and clamp (qnnp_*_clamp_nc_u8):

 * live: with oracle/_ref present, every case of tests/_x8.py's restated reference test lists (and the extra and bench
   cases) runs on the compiled reference, which must give the bytes of the numpy model, FILL between strided pixels
   included;
 * interface: the prototypes in include/qnnpack_gfx950.h are token-identical to the reference header's, the library
   exports them, and without a GPU create answers uninitialized (no CPU fallback);
 * host code under AddressSanitizer + UBSan (Makefile target asan-x8), and no scratch in the kernels of hip/x8shuffle.hip.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import _x8 as x8
from oracle import ref
from qnnpack_amd import Status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X8_FUNCTIONS = ["qnnp_create_channel_shuffle_nc_x8", "qnnp_setup_channel_shuffle_nc_x8", "qnnp_create_clamp_nc_u8",
                "qnnp_setup_clamp_nc_u8"]


def test_case_lists_restate_the_reference_tests():
    # test/channel-shuffle.cc: 21 tests, test/clamp.cc: 9 tests
    assert len({c.name.rsplit("/", 1)[0] for c in x8.reference_shuffle_cases()}) == 21
    assert len({c.name.rsplit("/", 1)[0] for c in x8.reference_clamp_cases()}) == 9
    names = [c.name for c in x8.all_cases() + x8.bench_cases(128)]
    assert len(names) == len(set(names)), "case names must be unique"


def test_bench_shapes_are_the_shufflenet_units():
    got = {(g, gc) for _, g, gc, _ in x8.shufflenet_shuffles()}
    want = {(2, 25), (2, 50), (2, 100), (3, 20), (3, 40), (3, 80), (4, 17), (4, 34), (4, 68), (8, 12), (8, 24), (8, 48)}
    want |= {(2, gc) for gc in (24, 48, 96, 58, 116, 232, 88, 176, 352, 122, 244, 488)}
    assert got == want


def test_numpy_model_small_examples():
    x = np.arange(12, dtype=np.uint8)
    assert x8.channel_shuffle(x, 1, 3, 4).tolist() == [[0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]]
    case = x8.X8Case("clamp", "example", 2, clamp_channels=3, in_stride=4, out_stride=5, qmin=3, qmax=9)
    x = x8.input_tensor(case)
    y = x8.expected_one(case, x, 2)
    assert y.size == 8 and y[3] == x8.FILL and y[4] == x8.FILL
    assert np.array_equal(y[[0, 1, 2, 5, 6, 7]], np.clip(x[[0, 1, 2, 4, 5, 6]], 3, 9))


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libqnnpack_ref.so not built")
@pytest.mark.parametrize("kind", ["shuffle", "clamp"])
def test_numpy_model_matches_the_compiled_reference_on_every_case(kind):
    lib = ref.lib()
    for case in [c for c in x8.all_cases() if c.kind == kind]:
        got, _ = x8.run(lib, case)
        want = x8.expected(case)
        assert len(got) == len(want), case.name
        for g, w in zip(got, want):
            assert np.array_equal(g, w), case.name


def _prototypes(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    out = {}
    for name in X8_FUNCTIONS:
        m = re.search(r"enum\s+qnnp_status\s+" + name + r"\s*\((.*?)\)\s*;", text, re.S)
        assert m, (path, name)
        out[name] = re.findall(r"\w+|[^\s\w]", m.group(0))
    return out


REFERENCE_HEADER = "/root/reference/include/qnnpack.h"


@pytest.mark.skipif(not os.path.exists(REFERENCE_HEADER), reason="reference tree not present")
def test_prototypes_are_token_identical_to_the_reference():
    assert _prototypes(os.path.join(ROOT, "include", "qnnpack_gfx950.h")) == _prototypes(REFERENCE_HEADER)


def test_library_exports_the_x8_entry_points(product):
    for name in X8_FUNCTIONS:
        assert hasattr(product.lib, name), name


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="CPU-only behaviour")
def test_without_a_gpu_create_is_uninitialized(product):
    assert product.initialize_status() == Status.unsupported_hardware
    st, handle = product.create_channel_shuffle_nc_x8_status(2, 4)
    assert st == Status.uninitialized and not handle       # reference channel-shuffle.c:30-33
    st, handle = product.create_clamp_nc_u8_status(8, 0, 255)
    assert st == Status.uninitialized and not handle       # reference clamp.c:30-33


def test_x8_host_code_is_clean_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-x8"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "asan", "host_asan_x8_test")
    # the ASan runtime is linked statically (Makefile asan-x8), so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-x8-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]


def test_x8_kernels_use_no_scratch_and_fit_their_launch_bounds(tmp_path):
    """the checks of tests/test_kernel_resources.py for hip/x8shuffle.hip: 256-thread workgroups, no spills"""
    from test_kernel_resources import READELF, _code_objects
    lib = os.path.join(ROOT, "qnnpack_amd", "libqnnpack_gfx950.so")
    if not os.path.exists(lib) or not os.path.exists(READELF):
        pytest.skip("library or llvm-readelf not available")
    found = {}
    for k, elf in enumerate(_code_objects(open(lib, "rb").read())):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(elf)
        notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for entry in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            if "x8_shuffle_" in name or "u8_clamp_" in name:
                found[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", entry).group(1)))
    # shuffle: register {g2, g4} x {x4, x16}, lds, gather; clamp: {flat, rows} x {x16, x4, x1}
    assert len(found) == 12, sorted(found)
    for name, (vgpr, scratch, spill, wg) in found.items():
        assert scratch == 0 and spill == 0, (name, scratch, spill)
        assert wg == 256 and vgpr <= 64, (name, vgpr, wg)
