"""CPU tier of the windowed pooling operators (qnnp_create/setup_max_pooling2d_nhwc_u8, ..._average_pooling2d_nhwc_q8):

 * golden: tests/golden/reference_pooling_outputs.npz holds what the COMPILED REFERENCE produced for a spread of the
   cases of tests/_pooling.py; the numpy model there must reproduce every byte;
 * live: with oracle/_ref present, the whole restated reference test lists are compared against the compiled reference;
 * interface: the prototypes in include/qnnpack_gfx950.h are token-identical to the reference header's, the library
   exports them, and without a GPU create answers uninitialized (no CPU fallback);
 * host code under AddressSanitizer + UBSan (Makefile target asan-pool), and no scratch in the pooling kernels.
"""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import _pooling as pl
from oracle import ref
from qnnpack_amd import Status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_GOLDEN = dict(np.load(os.path.join(ROOT, "tests", "golden", "reference_pooling_outputs.npz")))
_CASES = {c.name: c for c in pl.all_cases()}
_GOLDEN_INDEX = {str(name): i for i, name in enumerate(_GOLDEN["names"])}
_GOLDEN_NAMES = sorted(_GOLDEN_INDEX)
POOLING_FUNCTIONS = ["qnnp_create_average_pooling2d_nhwc_q8", "qnnp_setup_average_pooling2d_nhwc_q8",
                     "qnnp_create_max_pooling2d_nhwc_u8", "qnnp_setup_max_pooling2d_nhwc_u8"]


def test_case_lists_restate_the_reference_tests():
    # test/max-pooling.cc: 51 tests, test/average-pooling.cc: 57 tests
    assert len({c.name.rsplit("/", 1)[0] for c in pl.reference_max_cases()}) == 51
    assert len({c.name.rsplit("/", 1)[0] for c in pl.reference_avg_cases()}) == 57
    assert len(_CASES) == len(pl.all_cases()), "case names must be unique"
    assert len(_GOLDEN_NAMES) > 800


@pytest.mark.parametrize("name", _GOLDEN_NAMES)
def test_numpy_model_reproduces_the_reference(name):
    """every golden output is pinned by its CRC-32; the small ones (tests/golden/generate_golden_pooling.py) are also
    stored whole and compared byte for byte"""
    case, k = _CASES[name], _GOLDEN_INDEX[name]
    x = pl.input_tensor(case)
    assert zlib.crc32(x.tobytes()) == int(_GOLDEN["input_crc32"][k]), "the case's input changed"
    outs = pl.expected(case, x)
    assert len(outs) == int(_GOLDEN["output_count"][k]), name
    lo, hi = int(_GOLDEN["output_offsets"][k]), int(_GOLDEN["output_offsets"][k + 1])
    if hi > lo:
        assert np.array_equal(np.concatenate(outs), _GOLDEN["output_bytes"][lo:hi]), name
    for i, out in enumerate(outs):
        assert zlib.crc32(out.tobytes()) == int(_GOLDEN["output_crc32"][k][i]), (name, i)


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libqnnpack_ref.so not built")
@pytest.mark.parametrize("kind", ["max", "avg"])
def test_numpy_model_matches_the_compiled_reference_on_every_case(kind):
    lib = ref.lib()
    cases = [c for c in pl.all_cases() if c.kind == kind and not (c.misalign_in or c.misalign_out or c.host)]
    for case in cases:
        x = pl.input_tensor(case)
        got, _ = pl.run(lib, case, x)
        for g, w in zip(got, pl.expected(case, x)):
            assert np.array_equal(g, w), case.name


def _prototypes(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    out = {}
    for name in POOLING_FUNCTIONS:
        m = re.search(r"enum\s+qnnp_status\s+" + name + r"\s*\((.*?)\)\s*;", text, re.S)
        assert m, (path, name)
        out[name] = re.findall(r"\w+|[^\s\w]", m.group(0))
    return out


REFERENCE_HEADER = "/root/reference/include/qnnpack.h"


@pytest.mark.skipif(not os.path.exists(REFERENCE_HEADER), reason="reference tree not present")
def test_prototypes_are_token_identical_to_the_reference():
    assert _prototypes(os.path.join(ROOT, "include", "qnnpack_gfx950.h")) == _prototypes(REFERENCE_HEADER)


def test_library_exports_the_pooling_entry_points(product):
    for name in POOLING_FUNCTIONS:
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
    st, handle = product.create_max_pooling2d_nhwc_u8_status(0, 0, 0, 0, 3, 3, 2, 2, 1, 1, 8, 0, 255)
    assert st == Status.uninitialized and not handle       # reference max-pooling.c:56-59
    st, handle = product.create_average_pooling2d_nhwc_q8_status(0, 0, 0, 0, 3, 3, 2, 2, 8, 0, 1.0, 0, 1.0, 0, 255)
    assert st == Status.uninitialized and not handle       # reference average-pooling.c:56-59


def test_pooling_host_code_is_clean_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-pool"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "asan", "host_asan_pool_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-pool-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]


def test_pooling_kernels_use_no_scratch_and_fit_their_launch_bounds(tmp_path):
    """the checks of tests/test_kernel_resources.py for hip/q8pool.hip: 256-thread workgroups, no spills"""
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
            if "q8_maxpool_kernel" in name or "q8_avgpool_kernel" in name:
                found[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", entry).group(1)))
    assert len(found) == 6, sorted(found)       # {max, avg} x {16, 4, 1 bytes per lane}
    for name, (vgpr, scratch, spill, wg) in found.items():
        assert scratch == 0 and spill == 0, (name, scratch, spill)
        assert wg == 256 and vgpr <= 128, (name, vgpr, wg)   # 256 threads = 4 waves: at least 4 waves per SIMD
