"""CPU tier of the quantize and dequantize operators (include/qnnpack_gfx950_float.h, quantize.c, dequantize.c,
hip/f32q8.hip):

 * interface: the six prototypes in the new header are the specified ones, the library exports them, the binding's
   FLOAT_API is their image (types, names, order) while API stays the 65 functions of the three older headers, and
   without a GPU the creates answer uninitialized (no CPU fallback);
 * the numpy statement of tests/_quantize.py against an independent implementation, torch's CPU quantizer, where the two
   definitions agree (finite inputs with |x| / scale <= 2^24): no mismatch allowed; and by hand where they do not;
 * the kernel rule of tests/_quantize.py:kernel_for;
 * host code under AddressSanitizer + UBSan as a stand-alone program (Makefile target asan-quantize), and the kernels of
   hip/f32q8.hip: no scratch, no spills, 256-thread workgroups, at most 64 VGPRs, LDS only in the two planar kernels.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import _quantize as fq
from _headers import HEADERS, prototypes
from qnnpack_amd import Status, binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "qnnpack_gfx950_float.h"
FUNCTIONS = ["qnnp_gfx950_create_quantize_nc_f32_q8", "qnnp_gfx950_setup_quantize_nc_f32_q8",
             "qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8", "qnnp_gfx950_create_dequantize_nc_q8_f32",
             "qnnp_gfx950_setup_dequantize_nc_q8_f32", "qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32"]
PROTOTYPES = [
    "enum qnnp_status qnnp_gfx950_create_quantize_nc_f32_q8(size_t channels, uint8_t output_zero_point, "
    "float output_scale, uint8_t output_min, uint8_t output_max, uint32_t flags, qnnp_operator_t* quantize);",
    "enum qnnp_status qnnp_gfx950_setup_quantize_nc_f32_q8(qnnp_operator_t quantize, size_t batch_size, "
    "const float* input, size_t input_stride, uint8_t* output, size_t output_stride);",
    "enum qnnp_status qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(qnnp_operator_t quantize, size_t batch_size, "
    "size_t pixels, const float* input, uint8_t* output, size_t output_pixel_stride);",
    "enum qnnp_status qnnp_gfx950_create_dequantize_nc_q8_f32(size_t channels, uint8_t input_zero_point, "
    "float input_scale, uint32_t flags, qnnp_operator_t* dequantize);",
    "enum qnnp_status qnnp_gfx950_setup_dequantize_nc_q8_f32(qnnp_operator_t dequantize, size_t batch_size, "
    "const uint8_t* input, size_t input_stride, float* output, size_t output_stride);",
    "enum qnnp_status qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(qnnp_operator_t dequantize, size_t batch_size, "
    "size_t pixels, const uint8_t* input, size_t input_pixel_stride, float* output);"]


# ---- interface ------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_as_specified():
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)).replace("( ", "(")
    for prototype in PROTOTYPES:
        assert prototype in text, prototype
    assert '#include "qnnpack_gfx950.h"' in raw
    assert sorted(prototypes(HEADER)) == sorted(FUNCTIONS)
    # the header says what the scale range buys
    assert "denormal mode" in re.sub(r"\s+", " ", raw)
    # and the three older headers declare none of them
    for header in HEADERS:
        assert not set(prototypes(header)) & set(FUNCTIONS), header


def test_library_exports_the_entry_points(product):
    for name in FUNCTIONS:
        assert hasattr(product.lib, name), name
        assert getattr(product.lib, name).argtypes == binding.FLOAT_API[FUNCTIONS.index(name)].argtypes


def test_float_api_is_the_image_of_the_header_and_api_is_untouched():
    from test_binding_signatures import SCALARS, is_c_pointer, is_pointer, python_name
    declared = prototypes(HEADER)
    assert [f.symbol for f in binding.FLOAT_API] == FUNCTIONS
    for f in binding.FLOAT_API:
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
            if c_type in ("float*", "uint8_t*"):
                assert p.kind == "tensor", (f.symbol, p.name, p.kind)
    # a table of its own: API and its two halves are what they were, and only the product class has the methods
    assert len(binding.API) == 65
    assert len(binding.QNNPACK_API) + len(binding.GFX950_API) == 65
    assert not set(FUNCTIONS) & set(binding.API)
    for name in ("create_quantize_nc_f32_q8", "setup_quantize_nc_f32_q8", "setup_quantize_nchw_f32_nhwc_q8",
                 "create_dequantize_nc_q8_f32", "setup_dequantize_nc_q8_f32", "setup_dequantize_nhwc_q8_nchw_f32"):
        for method in (name, name + "_status"):
            assert method in vars(binding.Gfx950Library) and not hasattr(binding.QnnpackLibrary, method), method


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="CPU-only behaviour")
def test_without_a_gpu_create_is_uninitialized(product):
    assert product.initialize_status() == Status.unsupported_hardware
    st, handle = product.create_quantize_nc_f32_q8_status(8, *fq.MID.args())
    assert st == Status.uninitialized and not handle
    st, handle = product.create_dequantize_nc_q8_f32_status(8, fq.MID.zp, fq.MID.scale)
    assert st == Status.uninitialized and not handle
    x, y = np.zeros(8, np.float32), np.zeros(8, np.uint8)
    assert product.setup_quantize_nc_f32_q8_status(None, 1, x, 8, y, 8) == Status.uninitialized
    assert product.setup_quantize_nchw_f32_nhwc_q8_status(None, 1, 1, x, y, 8) == Status.uninitialized
    assert product.setup_dequantize_nc_q8_f32_status(None, 1, y, 8, x, 8) == Status.uninitialized
    assert product.setup_dequantize_nhwc_q8_nchw_f32_status(None, 1, 1, y, 8, x) == Status.uninitialized


# ---- the numpy statement --------------------------------------------------------------------------------------------
TORCH_SETS = [(0.0186, 114), (1.0 / 256, 0), (0.5, 255), (3.1e-5, 7), (17.0, 128), (2.0 ** -20, 1)]


@pytest.mark.parametrize("scale,zp", TORCH_SETS)
def test_numpy_statement_equals_torch_cpu_where_the_definitions_agree(scale, zp):
    """100 000 normal values, 600 exact ties, +-0 and denormals: finite and |x| / scale <= 2^24 (a condition, not a
    tolerance: beyond it torch's CPU path answers 0 where this definition saturates). Zero mismatches."""
    import torch
    q = fq.Quant(zp, scale)
    rng = np.random.default_rng(fq._seed(f"torch/{scale}/{zp}"))
    x = np.concatenate([rng.normal(0, scale * 80, 100000).astype(np.float32),
                        (np.arange(-300, 300, dtype=np.float32) + np.float32(0.5)) * np.float32(scale),
                        np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45], np.float32)])
    assert np.all(np.isfinite(x)) and np.all(np.abs(x.astype(np.float64)) / scale <= 2.0 ** 24)
    want = torch.quantize_per_tensor(torch.from_numpy(x), float(scale), zp, torch.quint8).int_repr().numpy()
    got = fq.quantize(x, q)
    bad = np.flatnonzero(want != got)
    assert bad.size == 0, (bad.size, x[bad[:4]], want[bad[:4]], got[bad[:4]])
    assert np.unique(got).size > 100
    every = np.arange(256, dtype=np.uint8)
    want = torch.dequantize(torch._make_per_tensor_quantized_tensor(torch.from_numpy(every), float(scale), zp)).numpy()
    assert np.array_equal(fq.bits(fq.dequantize(every, q)), fq.bits(want))


def test_numpy_statement_by_hand_where_torch_differs():
    """saturation, NaN, infinities, the clamped zero point, ties to even, a narrow range"""
    f = np.float32
    q = fq.Quant(100, 0.25, 90, 250)
    x = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 3.4e38, -3.4e38, 1e30, 0.125, 0.375, -0.125, -0.375,
                  0.625, 37.5, 37.6, -2.5, -2.6, 1e-40], f)
    want = [100, 100, 100, 100, 250, 90, 250, 90, 250, 100, 102, 100, 98, 102, 250, 250, 90, 90, 100]
    assert fq.quantize(x, q).tolist() == want
    # the zero point outside [min, max]: NaN and zero give the nearer bound
    assert fq.quantize(np.array([np.nan, 0.0, -0.0], f), fq.Quant(5, 1.0, 10, 20)).tolist() == [10, 10, 10]
    assert fq.quantize(np.array([np.nan, 0.0], f), fq.Quant(200, 1.0, 10, 20)).tolist() == [20, 20]
    # every denormal rounds to the zero point at the largest reciprocal, flushed or not
    tiny = np.array([1.1754942e-38, -1.1754942e-38, 1e-40, -1e-40], f)
    assert fq.quantize(tiny, fq.Quant(128, fq.SCALE_MIN)).tolist() == [128] * 4
    assert float(f(tiny[0]) * (f(1) / f(fq.SCALE_MIN))) < 2.0 ** -7
    # dequantize: exact integers times the scale, both scale bounds finite and normal
    assert fq.dequantize(np.array([0, 37, 255], np.uint8), fq.Quant(37, 0.125)).tolist() == [-4.625, 0.0, 27.25]
    for scale in (fq.SCALE_MIN, fq.SCALE_MAX):
        y = fq.dequantize(np.arange(256, dtype=np.uint8), fq.Quant(0, scale))
        assert np.all(np.isfinite(y)) and np.all((y == 0) | (np.abs(y) >= np.finfo(f).tiny))
    # the value inputs of the GPU tier hold what they promise
    for name, qs in fq.SETS:
        v = fq.value_inputs(qs)
        assert np.isnan(v).sum() >= 7 and np.isinf(v).sum() >= 2 and v.size > 65536 + 256 + 3 * 512, name
        assert np.unique(fq.quantize(v, qs)).size == qs.qmax - qs.qmin + 1, name


def test_kernel_rule_examples():
    k = fq.kernel_for
    assert k("quantize", fq.Rows(32, 3), 0, 0) == "f32q8_quantize_x16"
    assert k("dequantize", fq.Rows(32, 3), 0, 0) == "f32q8_dequantize_x16"
    # dense rows are one row: the channel count and the batch do not enter
    assert k("quantize", fq.Rows(3, 50), 16, 32) == "f32q8_quantize_x16"
    assert k("quantize", fq.Rows(21, 7), 0, 0) == "f32q8_quantize_x16"
    assert k("quantize", fq.Rows(17, 1, 100, 33), 0, 0) == "f32q8_quantize_x16"       # one row: the strides do not count
    # strided rows: the byte stride on 16 and the float stride on 4 elements
    assert k("quantize", fq.Rows(17, 3, 20, 32), 0, 0) == "f32q8_quantize_x16"
    assert k("quantize", fq.Rows(17, 3, 21, 32), 0, 0) == "f32q8_quantize_x4"
    assert k("quantize", fq.Rows(17, 3, 20, 36), 0, 0) == "f32q8_quantize_x4"
    assert k("quantize", fq.Rows(17, 3, 20, 33), 0, 0) == "f32q8_quantize_x1"
    # base addresses: the float side only matters for the 16-byte pieces
    assert k("dequantize", fq.Rows(32, 3), 4, 0) == "f32q8_dequantize_x4"
    assert k("dequantize", fq.Rows(32, 3), 0, 4) == "f32q8_dequantize_x4"
    assert k("dequantize", fq.Rows(32, 3), 12, 8) == "f32q8_dequantize_x4"
    assert k("dequantize", fq.Rows(32, 3), 0, 2) == "f32q8_dequantize_x1"
    assert k("dequantize", fq.Rows(32, 3), 4, 7) == "f32q8_dequantize_x1"


def test_expected_keeps_the_fill_between_rows_and_pixels():
    s = fq.Rows(3, 2, 5, 7)
    x = np.arange(s.f_elements, dtype=np.float32) * np.float32(0.0186)
    out = fq.quantize_rows_expected(fq.MID, s, x, np.full(s.q_bytes, fq.FILL, np.uint8))
    assert out.size == 10 and np.all(out[3:7] == fq.FILL)
    assert out[[0, 1, 2, 7, 8, 9]].tolist() == [114, 115, 116, 119, 120, 121]
    back = fq.dequantize_rows_expected(fq.MID, s, out, fq.fill_f32(s.f_elements))
    assert fq.bits(back)[3:5].tolist() == [0xA5A5A5A5] * 2 and back[5] == np.float32(5) * np.float32(0.0186)
    p = fq.Planar(2, 3, 2, extra=1)
    x = (np.arange(p.f_elements, dtype=np.float32) * np.float32(0.0186)).astype(np.float32)
    out = fq.quantize_planar_expected(fq.MID, p, x, np.full(p.q_bytes, fq.FILL, np.uint8))
    # image 0: channel 0 = 0 1 2, channel 1 = 3 4 5 -> pixels (0, 3) (1, 4) (2, 5); image 1 starts at 6
    assert out.tolist() == [114, 117, fq.FILL, 115, 118, fq.FILL, 116, 119, fq.FILL, 120, 123, fq.FILL, 121, 124, fq.FILL,
                            122, 125]
    back = fq.dequantize_planar_expected(fq.MID, p, out)
    assert np.array_equal(fq.bits(back), fq.bits(fq.dequantize(np.arange(114, 126, dtype=np.uint8), fq.MID)))


# ---- host code and kernels ------------------------------------------------------------------------------------------
def test_quantize_host_code_is_clean_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-quantize"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "asan", "host_asan_quantize_test")
    # the ASan runtime is linked statically (Makefile asan-quantize), so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-quantize-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]


def test_f32q8_kernels_use_no_scratch_and_fit_their_launch_bounds(tmp_path):
    """the checks of tests/test_kernel_resources.py for hip/f32q8.hip"""
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
            if "f32q8_" in name:
                found[name] = tuple(int(re.search(rf"\.{field}:\s+(\d+)", entry).group(1)) for field in (
                    "vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
                    "max_flat_workgroup_size", "group_segment_fixed_size"))
    # rows: quantize and dequantize x (16 with and without the streaming hint, 4, 1); planar: each direction x the hint
    rows = [n for n in found if "rows_kernel" in n]
    planar = [n for n in found if "planar_kernel" in n]
    assert len(rows) == 8 and len(planar) == 4 and len(found) == 12, sorted(found)
    for quant in ("Lb1E", "Lb0E"):
        for rest in ("Li16ELb1E", "Li16ELb0E", "Li4ELb0E", "Li1ELb0E"):
            assert sum(f"rows_kernelI{quant}{rest}" in n for n in rows) == 1, (quant, rest, sorted(rows))
    assert sum("f32q8_quantize_planar_kernel" in n for n in planar) == 2
    assert sum("f32q8_dequantize_planar_kernel" in n for n in planar) == 2
    for name, (vgpr, scratch, vspill, sspill, wg, lds) in found.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert wg == 256 and vgpr <= 64, (name, vgpr, wg)
        assert lds == (16384 + 16 if "planar" in name else 0), (name, lds)
