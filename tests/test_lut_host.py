"""CPU tier of the byte lookup-table operators: sigmoid (qnnp_*_sigmoid_nc_q8), leaky ReLU (qnnp_*_leaky_relu_nc_q8) and
the product's table operator (qnnp_gfx950_*_lut_nc_x8):

 * live: with oracle/_ref present, every sigmoid and leaky ReLU case of tests/_lut.py runs on the compiled reference on
   its own tensors, which must give the bytes of the reference's table (its answer on the identity input) applied by
   numpy, FILL between strided pixels included; in place and strided among them;
 * interface: the prototypes in include/qnnpack_gfx950.h are token-identical to the reference header's, the library
   exports all six entry points, and without a GPU create answers uninitialized (no CPU fallback);
 * host code under AddressSanitizer + UBSan as a stand-alone program (Makefile target asan-lut), and the six kernels of
   hip/x8lut.hip: no scratch, 256-thread workgroups, at most 64 VGPRs, 256 bytes of LDS.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import _lut as lut
from oracle import ref
from qnnpack_amd import Status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_FUNCTIONS = ["qnnp_create_sigmoid_nc_q8", "qnnp_setup_sigmoid_nc_q8", "qnnp_create_leaky_relu_nc_q8",
                       "qnnp_setup_leaky_relu_nc_q8"]
LUT_FUNCTIONS = REFERENCE_FUNCTIONS + ["qnnp_gfx950_create_lut_nc_x8", "qnnp_gfx950_setup_lut_nc_x8"]


def test_case_lists_restate_the_reference_tests():
    # test/sigmoid.cc: 18 tests, test/leaky-relu.cc: 13 tests
    assert len({c.name.rsplit("/", 1)[0] for c in lut.reference_sigmoid_cases()}) == 18
    assert len({c.name.rsplit("/", 1)[0] for c in lut.reference_leaky_relu_cases()}) == 13
    names = [c.name for c in lut.all_cases()]
    assert len(names) == len(set(names)), "case names must be unique"


def test_float_loops_are_the_reference_tests_loops():
    # for (float s = 1.0e-2f; s < 1.0e+2f; s *= 10.0f): five steps, the float32 products staying just below the powers
    # of ten (the last is 99.99999); *= 3.14159265f: nine; slopes from 1.0e-4f: nine
    tens = lut._float_loop(1.0e-2, 1.0e+2, 10.0)
    assert len(tens) == 5 and tens[0] == float(np.float32(0.01)) and 99.9999 < tens[-1] < 100.0
    assert len(lut._float_loop(1.0e-2, 1.0e+2, 3.14159265)) == 9
    slopes = lut._float_loop(1.0e-4, 1.0, 3.14159265)
    assert len(slopes) == 9 and all(0 < s < 1 for s in slopes)
    by_test = {}
    for c in lut.reference_sigmoid_cases() + lut.reference_leaky_relu_cases():
        by_test.setdefault(c.name.rsplit("/", 1)[0], []).append(c)
    assert len(by_test["sigmoid/strided_batch_with_input_scale"]) == 7 * 5
    assert len(by_test["leaky/unit_batch_with_negative_slope"]) == 7 * 9
    assert len(by_test["leaky/unit_batch"]) == 99


def test_input_tensors_hold_every_byte_value():
    for case in lut.extra_cases() + lut.flat_edge_cases(4) + lut.reference_sigmoid_cases():
        for b in case.batches():
            x = lut.input_tensor(case, b)
            distinct = np.unique(x).size
            assert distinct == min(x.size, 256), (case.name, x.size, distinct)


def test_numpy_applies_a_table_and_keeps_the_fill():
    case = lut.LutCase("table", "example", 2, 3, in_stride=4, out_stride=5)
    table = lut.permutation(1)
    assert sorted(table.tolist()) == list(range(256)) and not np.array_equal(table, lut.permutation(2))
    x = np.array([9, 8, 7, 0, 6, 5, 4], np.uint8)
    y = lut.apply_table(case, table, x, 2)
    assert y.size == 8 and y[3] == lut.FILL and y[4] == lut.FILL
    assert y[[0, 1, 2, 5, 6, 7]].tolist() == table[[9, 8, 7, 6, 5, 4]].tolist()
    in_place = lut.LutCase("table", "example_in_place", 2, 3, in_stride=4, in_place=True)
    z = lut.apply_table(in_place, table, x, 2)
    assert z.tolist() == table[[9, 8, 7]].tolist() + [0] + table[[6, 5, 4]].tolist()


needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libqnnpack_ref.so not built")


@needs_reference
@pytest.mark.parametrize("kind", ["sigmoid", "leaky"])
def test_compiled_reference_matches_its_table_on_every_case(kind):
    reference = ref.lib()
    cases = [c for c in lut.all_cases() if c.kind == kind]
    assert any(c.in_place and c.in_stride for c in cases) and any(c.next_batch for c in cases)
    for case in cases:
        lut.check_reference(reference, case)


@needs_reference
def test_reference_tables_are_plausible():
    """the identity-input recovery gives the operator's table: monotone, saturating at the output range, and the
    sigmoid's midpoint at the input zero point"""
    reference = ref.lib()
    t = lut.reference_table(reference, lut.LutCase("sigmoid", "t", 1, 1, input_scale=0.1, input_zero_point=128))
    assert t[128] == 128 and np.all(np.diff(t.astype(int)) >= 0) and t[0] < 5 and t[255] > 250
    t = lut.reference_table(reference, lut.LutCase("sigmoid", "t", 1, 1, qmin=30, qmax=99, input_scale=10.0))
    assert t.min() == 30 and t.max() == 99
    t = lut.reference_table(reference, lut.LutCase("leaky", "t", 1, 1, slope=1.0, input_scale=0.5, output_scale=0.5,
                                                   input_zero_point=9, output_zero_point=9))
    assert np.array_equal(t, np.arange(256, dtype=np.uint8))


@needs_reference
def test_reference_create_statuses():
    """the compiled reference answers invalid_parameter for an invalid range and a zero scale, unsupported_parameter
    for an output scale other than 1/256"""
    reference = ref.lib()
    assert reference.create_sigmoid_nc_q8_status(8, 0, 1.0, 0, 1.0 / 256, 200, 100)[0] == Status.invalid_parameter
    assert reference.create_sigmoid_nc_q8_status(8, 0, 0.0, 0, 1.0 / 256, 0, 255)[0] == Status.invalid_parameter
    assert reference.create_sigmoid_nc_q8_status(8, 0, 1.0, 0, 0.5, 0, 255)[0] == Status.unsupported_parameter


def _prototypes(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    out = {}
    for name in REFERENCE_FUNCTIONS:
        m = re.search(r"enum\s+qnnp_status\s+" + name + r"\s*\((.*?)\)\s*;", text, re.S)
        assert m, (path, name)
        out[name] = re.findall(r"\w+|[^\s\w]", m.group(0))
    return out


REFERENCE_HEADER = "/root/reference/include/qnnpack.h"


@pytest.mark.skipif(not os.path.exists(REFERENCE_HEADER), reason="reference tree not present")
def test_prototypes_are_token_identical_to_the_reference():
    assert _prototypes(os.path.join(ROOT, "include", "qnnpack_gfx950.h")) == _prototypes(REFERENCE_HEADER)


def test_generic_pair_is_declared_as_specified():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "qnnpack_gfx950.h")).read())
    assert ("enum qnnp_status qnnp_gfx950_create_lut_nc_x8(size_t channels, const uint8_t table[256], uint32_t flags, "
            "qnnp_operator_t* lut);") in text
    assert ("enum qnnp_status qnnp_gfx950_setup_lut_nc_x8(qnnp_operator_t lut, size_t batch_size, const uint8_t* input, "
            "size_t input_stride, uint8_t* output, size_t output_stride);") in text


def test_library_exports_the_lut_entry_points(product):
    for name in LUT_FUNCTIONS:
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
    st, handle = product.create_sigmoid_nc_q8_status(8, 121, 0.75, 0, 1.0 / 256, 0, 255)
    assert st == Status.uninitialized and not handle       # reference sigmoid.c:34-37
    st, handle = product.create_leaky_relu_nc_q8_status(8, 0.5, 121, 1.25, 133, 0.75, 0, 255)
    assert st == Status.uninitialized and not handle       # reference leaky-relu.c:35-38
    st, handle = product.create_lut_nc_x8_status(8, lut.permutation(1))
    assert st == Status.uninitialized and not handle


def test_lut_host_code_is_clean_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-lut"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "asan", "host_asan_lut_test")
    # the ASan runtime is linked statically (Makefile asan-lut), so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-lut-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]


def test_lut_kernels_use_no_scratch_and_fit_their_launch_bounds(tmp_path):
    """the checks of tests/test_kernel_resources.py for hip/x8lut.hip: 256-thread workgroups, no spills, one table in LDS"""
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
            if "x8_lut_" in name:
                found[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", entry).group(1)))
    # {flat, rows} x {x16, x4, x1}
    assert len(found) == 6, sorted(found)
    for name, (vgpr, scratch, spill, wg, lds) in found.items():
        assert scratch == 0 and spill == 0, (name, scratch, spill)
        assert wg == 256 and vgpr <= 64, (name, vgpr, wg)
        assert lds == 256, (name, lds)
        assert "x8_shuffle_" not in name and "u8_clamp_" not in name, name
