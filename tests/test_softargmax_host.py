"""CPU tier of the softargmax operator (qnnp_*_softargmax_nc_q8):

 * the case list of tests/_softargmax.py restates the reference's 12 tests, and the model is what the module says;
 * live: with oracle/_ref present, every case not marked zero_sum runs on the compiled reference on its own tensors, which
   must give the bytes of the model, FILL in front of, between and behind strided rows included; in place, strided,
   wrapped sums and re-setup among them;
 * the fence: a row whose table sum is 0 modulo 2^32 raises before the reference is reached (tested with the model alone:
   such a row would kill this process in the reference);
 * interface: the prototypes in include/qnnpack_gfx950.h are token-identical to the reference header's, the library
   exports both entry points, and without a GPU create answers uninitialized (no CPU fallback);
 * host code under AddressSanitizer + UBSan as a stand-alone program (Makefile target asan-softargmax), and the six kernels
   of hip/q8softargmax.hip: no scratch, 256-thread workgroups, at most 128 VGPRs; 1024 bytes of LDS (the table) for the
   group kernels, 1056 for the stream kernels (table + reduction words), 33840 for the LDS kernels (+ 32768 + 16 of row).
   Compiled with ROCm 7.2: group x16 85 VGPRs, group x1 125, lds x16 44, lds x1 41, stream x16 42, stream x1 57.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import _softargmax as sam
from oracle import ref
from qnnpack_amd import Status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["qnnp_create_softargmax_nc_q8", "qnnp_setup_softargmax_nc_q8"]


def test_case_list_restates_the_reference_tests():
    cases = sam.reference_cases()
    by_test = {}
    for c in cases:
        by_test.setdefault(c.name.rsplit("/", 1)[0], []).append(c)
    assert len(by_test) == 12       # the TEST()s of test/softargmax.cc
    assert [c.channels for c in by_test["ref/many_classes"]] == list(range(3, 100))
    assert [c.channels for c in by_test["ref/imagenet_classes"]] == [1000, 1001, 21841]
    # for (float s = 1.0e-2f; s < 1.0e+2f; s *= 3.14159265f): nine steps, for channels 1, 6, ..., 96
    assert len(by_test["ref/many_channels_with_input_scale"]) == 20 * 9
    assert len(by_test["ref/many_channels_with_input_zero_point"]) == 20 * 6
    assert all(c.batch == 3 and c.strides_at(0) == (129, 117)
               for c in by_test["ref/strided_batch_with_input_and_output_stride"])
    assert by_test["ref/zero_batch"][0].batch == 0
    assert all(c.scale == float(np.float32(0.176080093)) for c in by_test["ref/small_batch"])
    names = [c.name for c in sam.all_cases()]
    assert len(names) == len(set(names)), "case names must be unique"


def test_selection_boundaries_and_the_cases_around_them():
    assert sam.selection_boundaries() == [16, 17, 32, 49, 64, 113, 128, 241, 256, 497, 512, 1009, 1024, 32768]
    assert sam.group_lanes(21, 16) == 2 and sam.group_lanes(21, 1) == 2 and sam.group_lanes(1024, 16) == 64
    assert sam.kernel_name(1024, 16) == "q8_softargmax_group1024_x16"
    assert sam.kernel_name(1025, 1) == "q8_softargmax_lds32768_x1"
    assert sam.kernel_name(32769, 16) == "q8_softargmax_stream_x16"
    channels = {c.channels for c in sam.boundary_cases()}
    for b in sam.selection_boundaries():
        assert {b - 1, b, b + 1} <= channels, b
    assert set(range(1, 71)) <= channels
    for case in sam.sweep_cases():
        assert case.batch * case.channels < 64 << 20, case.name


def test_model_on_rows_worked_by_hand():
    # one class: table[255] * 256 / table[255] = 256 -> 255
    one = sam.Case("one", 2, 1)
    out, sums = sam.model(one, np.array([0, 200], np.uint8))
    assert out.tolist() == [255, 255] and sums.tolist() == [8388607, 8388607]
    # two equal classes: 128 each; the strided output keeps its FILL
    two = sam.Case("two", 2, 2, in_stride=3, out_stride=4)
    out, _ = sam.model(two, np.array([9, 9, 77, 250, 250], np.uint8))
    assert out.tolist() == [128, 128, sam.FILL, sam.FILL, 128, 128]
    # a constant row of 513 channels: the sum wraps to a small value and every quotient saturates
    wrap = sam.Case("wrap", 1, 513)
    t255 = int(sam.table(wrap.scale, 513)[255])
    out, sums = sam.model(wrap, np.full(513, 50, np.uint8))
    assert t255 * 513 >= 1 << 32 and sums[0] == (t255 * 513) % (1 << 32) and 0 < sums[0] < 1000
    assert np.all(out == 255)
    # a constant row of 1024 channels: the sum is 0 modulo 2^32 and the output all 0, in place too
    for c in sam.ZERO_SUM_CHANNELS:
        zero = sam.Case("zero", 1, c, in_place=True)
        out, sums = sam.model(zero, np.full(c, 113, np.uint8))
        assert sums[0] == 0 and int(sam.table(zero.scale, c)[255]) * c == 1 << 32 and np.all(out == 0)


def test_input_rows_are_what_the_cases_ask_for():
    for case in sam.content_cases() + sam.zero_sum_cases():
        x = sam.input_tensor(case)
        rows = x.reshape(case.batch, case.channels)
        if case.rows == "top":
            assert rows.min() >= 250
        elif case.rows == "dominant":
            assert np.all((rows == 200).sum(axis=1) == 1) and np.all((rows == 7).sum(axis=1) == case.channels - 1)
        elif case.rows == "tie":
            assert np.all((rows == 200).sum(axis=1) == 2)
            assert np.all((sam.model(case, x)[0].reshape(rows.shape) == 128).sum(axis=1) == 2)
        elif case.rows == "constant":
            assert np.all(rows == rows[:, :1])
        elif case.rows == "max_first":
            assert np.all(rows.argmax(axis=1) == 0) and np.all(rows[:, 1:] < 200)
        elif case.rows == "max_last":
            assert np.all(rows.argmax(axis=1) == case.channels - 1)
        elif case.rows == "zero_sum_middle":
            sums = sam.row_sums(case, x)
            assert sums[1] == 0 and sums[0] != 0 and sums[2] != 0, case.name
    # constant rows beyond 512 channels wrap to a nonzero sum; for 1025 channels to a single digit
    wrapped = {c.channels: sam.row_sums(c, sam.input_tensor(c)) for c in sam.content_cases() if c.rows == "constant"}
    assert all(np.all(s != 0) for s in wrapped.values())
    assert np.all(wrapped[1025] < 10) and np.all(wrapped[513] < 1000)


class _Unreachable:
    """stands where the compiled reference would: the fence must raise before it is touched"""

    def __getattr__(self, name):
        raise AssertionError(f"the fence let a zero-sum row through to the reference ({name})")


def test_the_fence_raises_on_a_zero_sum_row():
    for case in sam.zero_sum_cases():
        with pytest.raises(sam.ZeroSumRow):
            sam.run_reference(_Unreachable(), case)
        # the same rows in a case NOT marked zero_sum: the model's row sums stop it
        unmarked = sam.Case(case.name + "_unmarked", case.batch, case.channels, rows=case.rows)
        with pytest.raises(sam.ZeroSumRow, match="rows \\[1\\]"):
            sam.run_reference(_Unreachable(), unmarked)
    # at any input scale, and for an input handed in by the caller
    for scale in (1e-6, 1.0, 97.0):
        case = sam.Case("fill", 2, 65536, input_scale=scale)
        with pytest.raises(sam.ZeroSumRow):
            sam.run_reference(_Unreachable(), case, inputs=[np.zeros(2 * 65536, np.uint8)])


needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libqnnpack_ref.so not built")

_GROUPS = {
    "reference_list": sam.reference_cases,
    "extra": sam.extra_cases,
    "misaligned": lambda: [c for ch in sam.MISALIGNED_CHANNELS for c in sam.misaligned_cases(ch)],
    "sweep": sam.sweep_cases,
}


@needs_reference
@pytest.mark.parametrize("group", sorted(_GROUPS))
def test_model_matches_the_compiled_reference_on_every_case(group):
    reference = ref.lib()
    cases = _GROUPS[group]()
    assert cases and not any(c.zero_sum for c in cases)
    for case in cases:
        sam.check_model(reference, case)


def test_every_case_is_in_a_group_or_marked_zero_sum():
    grouped = {c.name for make in _GROUPS.values() for c in make()}
    rest = [c for c in sam.all_cases() if c.name not in grouped]
    assert rest and all(c.zero_sum for c in rest) and [c.name for c in rest] == [c.name for c in sam.zero_sum_cases()]
    extra = sam.extra_cases()
    assert any(c.in_place and c.in_stride for c in extra) and any(c.next_out_of_place for c in extra)


@needs_reference
def test_reference_create_statuses():
    """the compiled reference answers invalid_parameter for no channels and a zero scale, unsupported_parameter for an
    output scale other than 1/256 and an output zero point other than 0"""
    reference = ref.lib()
    assert reference.create_softargmax_nc_q8_status(0, 1.0, 0, 1.0 / 256)[0] == Status.invalid_parameter
    assert reference.create_softargmax_nc_q8_status(8, 0.0, 0, 1.0 / 256)[0] == Status.invalid_parameter
    assert reference.create_softargmax_nc_q8_status(8, 1.0, 0, 0.5)[0] == Status.unsupported_parameter
    assert reference.create_softargmax_nc_q8_status(8, 1.0, 1, 1.0 / 256)[0] == Status.unsupported_parameter


def _prototypes(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    out = {}
    for name in FUNCTIONS:
        m = re.search(r"enum\s+qnnp_status\s+" + name + r"\s*\((.*?)\)\s*;", text, re.S)
        assert m, (path, name)
        out[name] = re.findall(r"\w+|[^\s\w]", m.group(0))
    return out


REFERENCE_HEADER = "/root/reference/include/qnnpack.h"


@pytest.mark.skipif(not os.path.exists(REFERENCE_HEADER), reason="reference tree not present")
def test_prototypes_are_token_identical_to_the_reference():
    assert _prototypes(os.path.join(ROOT, "include", "qnnpack_gfx950.h")) == _prototypes(REFERENCE_HEADER)
    # the lines the product's header cites: the reference header's 311-324
    lines = open(REFERENCE_HEADER).read().splitlines()[310:324]
    assert lines[0].startswith("enum qnnp_status qnnp_create_softargmax_nc_q8(")
    assert any(line.startswith("enum qnnp_status qnnp_setup_softargmax_nc_q8(") for line in lines)


def test_no_document_says_softargmax_stays_on_the_cpu():
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("include", "qnnpack_gfx950.h")):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, name)).read())
        assert "it stays on the CPU" not in text and "still left on the CPU" not in text, name
        assert "qnnp_create_softargmax_nc_q8" in text or "softargmax_nc_q8" in text, name


def test_library_exports_the_softargmax_entry_points(product):
    for name in FUNCTIONS + ["qnnp_hip_softargmax_run"]:
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
    st, handle = product.create_softargmax_nc_q8_status(8, 0.176080093, 0, 1.0 / 256)
    assert st == Status.uninitialized and not handle       # reference softargmax.c:31-34


def test_softargmax_host_code_is_clean_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-softargmax"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "asan", "host_asan_softargmax_test")
    # the ASan runtime is linked statically (Makefile asan-softargmax), so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-softargmax-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]


def test_softargmax_kernels_use_no_scratch_and_fit_their_launch_bounds(tmp_path):
    """the checks of tests/test_kernel_resources.py for hip/q8softargmax.hip: 256-thread workgroups, no scratch, no
    spills, at most 128 VGPRs (two workgroups of 256 lanes a SIMD quarter stay resident), and the LDS of the module
    docstring: the table alone, table + reduction words, table + reduction words + the longest staged row"""
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
            if "q8_softargmax_" in name:
                found[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", entry).group(1)))
    # group x {x16, x1}, block x {x16, x1} x {row in LDS, row re-read}
    assert len(found) == 6, sorted(found)
    for name, (vgpr, scratch, spill, wg, lds) in found.items():
        assert scratch == 0 and spill == 0, (name, scratch, spill)
        assert wg == 256 and vgpr <= 128, (name, vgpr, wg)
        if "group_kernel" in name:
            assert lds == 1024, (name, lds)
        elif "Lb1E" in name:                      # block kernel, STAGE = true
            assert lds == 1024 + 32 + sam.LDS_MAX + 16, (name, lds)
        else:
            assert "Lb0E" in name and lds == 1024 + 32, (name, lds)
