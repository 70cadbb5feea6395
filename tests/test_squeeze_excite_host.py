"""CPU tier of the fused squeeze-and-excite operator (qnnp_gfx950_{create,setup}_squeeze_excite: squeeze-excite.c,
hip/q8segate.hip):

 * interface: the prototypes in include/qnnpack_gfx950_squeeze_excite.h are the specified ones, qnnpack_gfx950.h includes
   that header, binding.SQUEEZE_EXCITE_API is its image while API stays the 65 functions of the three older headers, the
   library exports the two entry points, and without a GPU they answer uninitialized (no CPU fallback);
 * the cases of tests/_squeeze_excite.py: the oracle's expectation of every case is not degenerate -- the hidden row hits
   its ReLU floor, the gate is not saturated, the output has many values -- so a kernel writing constants cannot pass;
 * host code under AddressSanitizer + UBSan as a stand-alone program (Makefile target asan-se): the fused operator over
   stubs that compute the gate from the packed device images, against values computed from the raw weights;
 * the kernels of hip/q8segate.hip: no scratch, no spills, 1024-thread workgroups, static LDS only.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import _squeeze_excite as se
from _headers import HEADERS, prototypes
from qnnpack_amd import Status, binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "qnnpack_gfx950_squeeze_excite.h"
FUNCTIONS = ["qnnp_gfx950_create_squeeze_excite", "qnnp_gfx950_setup_squeeze_excite"]
PROTOTYPES = [
    "enum qnnp_status qnnp_gfx950_create_squeeze_excite(qnnp_operator_t pool, qnnp_operator_t fc1, qnnp_operator_t fc2, "
    "qnnp_operator_t gate, qnnp_operator_t multiply, qnnp_operator_t* squeeze_excite);",
    "enum qnnp_status qnnp_gfx950_setup_squeeze_excite(qnnp_operator_t squeeze_excite, size_t batch_size, size_t pixels, "
    "const uint8_t* input, size_t input_pixel_stride, uint8_t* output, size_t output_pixel_stride);"]


def test_entry_points_are_declared_as_specified():
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)).replace("( ", "(")
    for prototype in PROTOTYPES:
        assert prototype in text, prototype
    assert sorted(prototypes(HEADER)) == sorted(FUNCTIONS)
    # a caller of qnnpack_gfx950.h has them, beside the fused block
    assert '#include "qnnpack_gfx950_squeeze_excite.h"' in open(os.path.join(ROOT, "include", "qnnpack_gfx950.h")).read()
    # the limit is named once in the header and once in the code, and the two are held equal at compile time
    assert re.search(r"#define QNNP_GFX950_SQUEEZE_EXCITE_MAX_CHANNELS 4096\b", raw)
    seam = open(os.path.join(ROOT, "qnnpack_amd", "csrc", "hip", "qnnp_hip.h")).read()
    assert re.search(r"#define QNNP_HIP_SE_MAX_CHANNELS 4096u\b", seam)
    host = open(os.path.join(ROOT, "qnnpack_amd", "csrc", "squeeze-excite.c")).read()
    assert "QNNP_GFX950_SQUEEZE_EXCITE_MAX_CHANNELS == QNNP_HIP_SE_MAX_CHANNELS" in host
    # and the three older headers declare neither
    for header in HEADERS:
        assert not set(prototypes(header)) & set(FUNCTIONS), header


def test_squeeze_excite_api_is_the_image_of_the_header_and_api_is_untouched():
    from test_binding_signatures import SCALARS, is_c_pointer, is_pointer, python_name
    declared = prototypes(HEADER)
    assert [f.symbol for f in binding.SQUEEZE_EXCITE_API] == FUNCTIONS
    for f in binding.SQUEEZE_EXCITE_API:
        ret, params = declared[f.symbol]
        assert ret == "enum qnnp_status" and f.restype is SCALARS[ret]
        assert f.bound == binding.IF_PRESENT and f.methods
        assert len(f.params) == len(params), f.symbol
        for (c_type, header_name), p, ctype in zip(params, f.params, f.argtypes):
            if is_c_pointer(c_type):
                assert is_pointer(ctype), (f.symbol, header_name, c_type, ctype)
            else:
                assert ctype is SCALARS[c_type], (f.symbol, header_name, c_type, ctype)
            assert p.name == python_name(f, c_type, header_name), (f.symbol, p.name, header_name)
            if c_type == "uint8_t*":
                assert p.kind == "tensor", (f.symbol, p.name, p.kind)
    assert len(binding.API) == 65 and not set(FUNCTIONS) & set(binding.API)
    for name in ("create_squeeze_excite", "setup_squeeze_excite"):
        for method in (name, name + "_status"):
            assert method in vars(binding.Gfx950Library) and not hasattr(binding.QnnpackLibrary, method), method


def test_library_exports_the_entry_points(product):
    for name in FUNCTIONS:
        assert hasattr(product.lib, name), name
        assert getattr(product.lib, name).argtypes == binding.SQUEEZE_EXCITE_API[FUNCTIONS.index(name)].argtypes


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="CPU-only behaviour")
def test_without_a_gpu_create_and_setup_are_uninitialized(product):
    assert product.initialize_status() == Status.unsupported_hardware
    st, handle = product.create_squeeze_excite_status(None, None, None, None, None)
    assert st == Status.uninitialized and not handle
    x = np.zeros(8, np.uint8)
    assert product.setup_squeeze_excite_status(None, 1, 1, x, 8, x, 8) == Status.uninitialized


@pytest.mark.parametrize("case", se.CASES, ids=lambda c: c.name)
def test_the_oracle_expectation_of_every_case_is_not_degenerate(case):
    """what tests/test_squeeze_excite_gpu.py asserts before it runs anything, here without a GPU"""
    block = se.block(case)
    se.assert_not_degenerate(block)
    # the expectation is a pure function of the case
    again = se.Block(case)
    assert np.array_equal(block.want, again.want) and np.array_equal(block.gate, again.gate)


def test_the_pooling_case_is_chosen_from_the_kernels_constants():
    src = open(os.path.join(ROOT, "qnnpack_amd", "csrc", "hip", "q8segate.hip")).read()
    assert int(re.search(r"constexpr int kSeThreads = (\d+);", src).group(1)) == se.SE_THREADS
    assert int(re.search(r"constexpr int kSePoolUnroll = (\d+);", src).group(1)) == se.SE_POOL_UNROLL
    case = next(c for c in se.CASES if c.name == "pool_passes")
    lanes = 1
    while lanes < case.c // 4:
        lanes *= 2
    split = se.SE_THREADS // lanes
    per_pass = se.SE_POOL_UNROLL * split
    # more than one pass of the unrolled loop, then a remainder that is neither empty nor a whole slice round
    assert case.c % 4 == 0 and case.pixels > 2 * per_pass and case.pixels % per_pass not in (0, split), (split, per_pass)
    assert case.pixels % split != 0


def test_squeeze_excite_host_code_is_clean_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-se"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "asan", "host_asan_se_test")
    # the ASan runtime is linked statically (Makefile asan-se), so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-se-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]


def test_se_gate_kernels_use_no_scratch_and_fit_their_launch_bounds(tmp_path):
    """the checks of tests/test_kernel_resources.py for hip/q8segate.hip"""
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
            if "q8_se_gate_kernel" in name:
                found[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.sgpr_spill_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", entry).group(1)))
    # pooling inside with dword and with byte loads, and the pooled rows read from the scratch: three instantiations
    assert len(found) == 3, sorted(found)
    assert sum("ILb1ELi4E" in n for n in found) == 1 and sum("ILb1ELi1E" in n for n in found) == 1, sorted(found)
    assert sum("ILb0ELi1E" in n for n in found) == 1, sorted(found)
    for name, (vgpr, scratch, vspill, sspill, wg, lds) in found.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        # sixteen waves of a workgroup on one compute unit: four per SIMD, 128 VGPRs each at the most
        assert wg == se.SE_THREADS and vgpr <= 128, (name, vgpr, wg)
        assert 0 < lds <= 65536, (name, lds)
