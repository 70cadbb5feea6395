"""CPU tier of the multiply operator (qnnp_gfx950_*_multiply_nc_q8) and of the hardswish and hardsigmoid table builders
(qnnp_gfx950_create_{hardswish,hardsigmoid}_nc_q8):

 * interface: the prototypes in include/qnnpack_gfx950.h are the specified ones, the library exports the four entry
   points, and without a GPU the three creates answer uninitialized (no CPU fallback);
 * the case code of tests/_multiply.py: the oracle on the exhaustive input reaches the distinct values each parameter
   set promises, the numpy tables are plausible, the kernel rule of the alignment classes;
 * host code under AddressSanitizer + UBSan as a stand-alone program (Makefile target asan-mul), and the kernels of
   hip/q8mul.hip: no scratch, no spills, 256-thread workgroups, at most 64 VGPRs, no LDS.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import _multiply as mul
from qnnpack_amd import Status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["qnnp_gfx950_create_multiply_nc_q8", "qnnp_gfx950_setup_multiply_nc_q8",
             "qnnp_gfx950_create_hardswish_nc_q8", "qnnp_gfx950_create_hardsigmoid_nc_q8"]


def test_entry_points_are_declared_as_specified():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "qnnpack_gfx950.h")).read(), flags=re.S)
    text = re.sub(r"\s+", " ", text).replace("( ", "(")
    assert ("enum qnnp_status qnnp_gfx950_create_multiply_nc_q8(size_t channels, uint8_t a_zero_point, float a_scale, "
            "uint8_t b_zero_point, float b_scale, uint8_t product_zero_point, float product_scale, uint8_t product_min, "
            "uint8_t product_max, uint32_t flags, qnnp_operator_t* multiply);") in text
    assert ("enum qnnp_status qnnp_gfx950_setup_multiply_nc_q8(qnnp_operator_t multiply, size_t b_rows, "
            "size_t a_rows_per_b_row, const uint8_t* a, size_t a_stride, const uint8_t* b, size_t b_stride, "
            "uint8_t* product, size_t product_stride);") in text
    for name in ("hardswish", "hardsigmoid"):
        assert (f"enum qnnp_status qnnp_gfx950_create_{name}_nc_q8(size_t channels, uint8_t input_zero_point, "
                "float input_scale, uint8_t output_zero_point, float output_scale, uint8_t output_min, "
                f"uint8_t output_max, uint32_t flags, qnnp_operator_t* {name});") in text
    # no new setup entry points: the table operator's setup takes the two activations
    assert "setup_hardswish" not in text and "setup_hardsigmoid" not in text


def test_library_exports_the_entry_points(product):
    for name in FUNCTIONS:
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
    st, handle = product.create_multiply_nc_q8_status(8, *mul.MID.args())
    assert st == Status.uninitialized and not handle
    st, handle = product.create_hardswish_nc_q8_status(8, 121, 0.05, 133, 0.04, 0, 255)
    assert st == Status.uninitialized and not handle
    st, handle = product.create_hardsigmoid_nc_q8_status(8, 121, 0.05, 0, 1.0 / 256, 0, 255)
    assert st == Status.uninitialized and not handle
    x = np.zeros(8, np.uint8)
    assert product.setup_multiply_nc_q8_status(None, 1, 1, x, 8, x, 8, x, 8) == Status.uninitialized


def test_exhaustive_sets_reach_the_values_they_promise():
    """every (a, b) pair once; the oracle accepts every ratio, and a kernel writing a constant cannot pass a set that
    states two values or more"""
    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    names = [name for name, _, _ in mul.EXHAUSTIVE]
    assert len(names) == len(set(names))
    for name, q, distinct in mul.EXHAUSTIVE:
        want = mul.product_rows(q, a, a.T)
        assert 2.0 ** -32 <= q.ratio < 1.0, name
        assert np.unique(want).size >= distinct, (name, np.unique(want).size)
        if distinct == 1:
            # |acc| * ratio < 1/2: every product rounds to 0, the tensor is the clamped zero point
            assert float(q.ratio) * 65025 < 0.5 and np.all(want == min(max(q.y_zp, q.qmin), q.qmax)), name
            assert want[0, 0] != mul.FILL
        else:
            assert float(q.ratio) * 65025 >= 0.5, name
    by_name = {name: q for name, q, _ in mul.EXHAUSTIVE}
    assert by_name["shift0"].ratio >= 0.5 and by_name["late_zero_point"].ratio < 2.0 ** -23
    assert by_name["smallest_ratio"].ratio == np.float32(2.0 ** -32)
    assert by_name["largest_ratio"].ratio == np.nextafter(np.float32(1), np.float32(0))
    # a hand-made value: (200 - 121) * (64 - 0) = 5056; * 0.0048828125 = 24.6875 -> 25; + 133
    assert mul.product_rows(mul.MID, np.array([[200]], np.uint8), np.array([[64]], np.uint8))[0, 0] == 158


def test_expected_keeps_the_fill_and_broadcasts_by_rows():
    s = mul.Shape(3, 2, 2, a_stride=4, b_stride=5, y_stride=6)
    a, b, y = mul.tensors("example", s)
    out = mul.expected(mul.MID, s, a, b, y)
    assert out.size == 3 * 6 + 3 and np.all(out[[3, 4, 5, 9, 10, 11, 15, 16, 17]] == mul.FILL)
    for r in range(4):
        want = mul.product_rows(mul.MID, a[r * 4:r * 4 + 3][None], b[(r // 2) * 5:(r // 2) * 5 + 3][None])[0]
        assert np.array_equal(out[r * 6:r * 6 + 3], want), r
    assert mul.kernel_for(mul.Shape(32, 1, 1), 0, 16, 32) == "q8_mul_x16"
    assert mul.kernel_for(mul.Shape(32, 1, 1), 0, 16, 4) == "q8_mul_x4"
    assert mul.kernel_for(mul.Shape(32, 1, 1, b_stride=36), 0, 0, 0) == "q8_mul_x4"
    assert mul.kernel_for(mul.Shape(30, 1, 1), 0, 0, 0) == "q8_mul_x1"
    assert mul.kernel_for(mul.Shape(32, 1, 1), 0, 2, 0) == "q8_mul_x1"


def test_numpy_tables_are_plausible():
    t = mul.hardsigmoid_table(128, 1.0 / 32, 0, 1.0 / 256, 0, 255)
    assert t[128] == 128 and t[32] == 0 and t[224] == 255 and t[176] == 192 and np.all(np.diff(t.astype(int)) >= 0)
    t = mul.hardswish_table(128, 1.0 / 16, 32, 1.0 / 16, 0, 255)
    assert t[128] == 32 and t[80] == 32 and t[104] == 26 and t[176] == 80 and t[255] == 159
    t = mul.hardswish_table(128, 1.0 / 16, 32, 1.0 / 16, 30, 100)
    assert t.min() == 30 and t.max() == 100


def test_multiply_host_code_is_clean_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-mul"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "asan", "host_asan_mul_test")
    # the ASan runtime is linked statically (Makefile asan-mul), so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-mul-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]


def test_mul_kernels_use_no_scratch_and_fit_their_launch_bounds(tmp_path):
    """the checks of tests/test_kernel_resources.py for hip/q8mul.hip"""
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
            if "q8_mul_" in name:
                found[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.sgpr_spill_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", entry).group(1)))
    # 16-byte pieces with and without the streaming hint, 4-byte pieces, single bytes: four instantiations
    assert len(found) == 4, sorted(found)
    assert sum("ILi16ELb1E" in n for n in found) == 1 and sum("ILi16ELb0E" in n for n in found) == 1, sorted(found)
    assert sum("ILi4ELb0E" in n for n in found) == 1 and sum("ILi1ELb0E" in n for n in found) == 1, sorted(found)
    for name, (vgpr, scratch, vspill, sspill, wg, lds) in found.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert wg == 256 and vgpr <= 64, (name, vgpr, wg)
        assert lds == 0, (name, lds)
