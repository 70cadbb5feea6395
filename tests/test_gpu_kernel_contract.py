"""GPU tier: the forced-kernel contract of include/qnnpack_gfx950_test.h, checked over one matrix of
(operator case) x (input offset, output offset) x (forced code).

Every case sits in guarded device buffers (_gpu.Guarded: a per-position pattern on both sides of each tensor) at byte
offsets that change the alignment every planner derives from the actual pointers (q8igemm.hip:derive, q8dwconv.hip:make_plan,
q8gemm128u.hip's four output paths, q8convc3.hip, q8fusedstrip.hip, q8deconv.hip). For every run:
  - code 0 (the automatic choice) never refuses a valid operator;
  - a forced code either refuses -- unsupported_parameter at setup or run, the whole output still FILL -- or reports a
    kernel in that code's set (FORCED_NAMES); it never reroutes;
  - a completed run equals the scalar oracle byte for byte, the gaps between strided rows included;
  - no byte outside the output changes: both guards of both tensors and the input itself stay as they were.
Each forced code must take the cases listed in ACCEPTS at offset (0, 0), so that a code that starts refusing everything
fails; codes documented for "any base address" (ANY_BASE) take every offset of each case they take at (0, 0).
Re-setup of one operator over several base addresses catches a plan cached under a stale key."""
import dataclasses
import functools

import numpy as np
import pytest

import _pointwise as pw
from _cases import ConvCase, DeconvCase, FcCase, conv_tensors, deconv_tensors, fc_tensors
from _gpu import Guarded
from _runner import FILL, assert_bytes_equal, conv_expected, conv_run, deconv_expected, deconv_run, fc_expected, fc_run, placed_run
from qnnpack_amd import QnnpackError, Status

pytestmark = pytest.mark.gpu

OFFSETS = [(0, 0), (1, 0), (0, 1), (2, 2), (3, 5), (4, 12), (8, 8)]


def _dw(name, hw, c, k=(3, 3), **kw):
    kw.setdefault("padding", (k[0] // 2, k[1] // 2, k[0] // 2, k[1] // 2))
    return ConvCase(name, hw, k, kw.pop("padding"), groups=c, gic=1, goc=1, **kw)


# ---- GEMM-family cases ("gemm_kernel"), each with the branch it is there to reach (rules of q8igemm.hip:make_plan) ----
GEMM_CASES = [
    FcCase("fc_k58_n58", 300, 58, 58),                       # odd K and N, byte stores: 128-row unaligned GEMM (29)
    FcCase("fc_k64_n64", 2048, 64, 64),                      # 16-byte rows, rows >= 2048: pointwise streaming kernel (5)
    FcCase("fc_k100_n100", 2048, 100, 100),                  # dword rows, N % 8 != 0, N >= 56: register-staged GEMM (29)
    FcCase("fc_k256_n256", 512, 256, 256),                   # few rows, long K: one wave per 32x32 block (6)
    FcCase("fc_k512_n512", 2048, 512, 512),                  # K >= 512, N % 256 == 0, rows >= 2048: 256x256 centred (23)
    FcCase("fc_k640_n64", 16384, 640, 64),                   # 256 < K <= 1024 over many row blocks: long-K / 128-row centred
    FcCase("fc_k58_strided", 260, 58, 58, input_stride=61, output_stride=67),   # unaligned row strides on both sides
    ConvCase("pw_c64_n64", (64, 64), gic=64, goc=64),        # dense 1x1, N % 16 == 0, flat rows: 16-byte stores
    ConvCase("pw_c64_n60", (64, 64), gic=64, goc=60),        # dense 1x1, N % 16 != 0 (dword stores): 29 from 56 channels
    ConvCase("pw_c48_n40_strided", (32, 64), gic=48, goc=40, input_pixel_stride=52, output_pixel_stride=44),
    ConvCase("pw_g2_25_88", (28, 28), groups=2, gic=25, goc=88, batch=3),      # ShuffleNet v1 g2: grouped, odd K
    ConvCase("pw_g8_12_45", (28, 28), groups=8, gic=12, goc=45, batch=2),      # ShuffleNet v1 g8: 8 groups of 12 -> 45
    ConvCase("pw_s2_128_256", (56, 56), subsampling=(2, 2), gic=128, goc=256, batch=3),   # strided 1x1: offset table, one tap
    ConvCase("c33_16_16", (128, 128), (3, 3), (1, 1, 1, 1), gic=16, goc=16),   # rows >= 16384, 16 channels: ws16s (32)
    ConvCase("c33_32_32", (128, 128), (3, 3), (1, 1, 1, 1), gic=32, goc=32),   # rows >= 16384, 32 -> 32: wave (8)
    ConvCase("c33_48_48", (128, 128), (3, 3), (1, 1, 1, 1), gic=48, goc=48),   # rows >= 16384, 48 channels: ws16s (32)
    ConvCase("c33_64_64", (128, 128), (3, 3), (1, 1, 1, 1), gic=64, goc=64),   # rows >= 16384, 64 -> 64: wave, 16x16x64 flavour
    ConvCase("c33_64_256", (32, 32), (3, 3), (1, 1, 1, 1), gic=64, goc=256, batch=4),     # rows >= 4096, 256 out: patch (22)
    ConvCase("c33_32_32_mid", (28, 28), (3, 3), (1, 1, 1, 1), gic=32, goc=32, batch=2),   # below the row rules: LDS-tiled (3)
    ConvCase("c3_7x7_s2", (112, 112), (7, 7), (3, 3, 3, 3), subsampling=(2, 2), gic=3, goc=64),   # first layer, 3136 rows: c3rows32
    ConvCase("c3_3x3_s2", (96, 96), (3, 3), (1, 1, 1, 1), subsampling=(2, 2), gic=3, goc=32),     # first layer, 2304 rows: c3rows
    DeconvCase("dc_4x4_s2", (14, 14), (4, 4), (1, 1, 1, 1), subsampling=(2, 2), gic=64, goc=32, batch=2),   # stride-2 streaming (13)
]

# ---- depthwise cases ("dwconv_kernel"; rules of q8dwconv.hip:make_plan) ----
DW_CASES = [
    _dw("dw3_c27", (14, 14), 27, batch=2),                  # odd C: nothing aligned, sliding window on unaligned dwords (8)
    _dw("dw3_c32", (14, 14), 32, batch=2),                  # C % 16 == 0: column window (6), matrix cores (4, 5, 7)
    _dw("dw3_c58", (14, 14), 58, batch=2),                  # ShuffleNet v2: C % 4 != 0, dwords at two-byte offsets
    _dw("dw3_c64_s2", (28, 28), 64, subsampling=(2, 2), batch=2),   # stride 2
    _dw("dw3_c64_wide", (56, 56), 64, batch=1),             # OW >= 56, C <= 96: the LDS-staged matrix-core kernel's range (5)
    _dw("dw5_c27", (14, 14), 27, k=(5, 5), batch=2),        # 5x5, odd C: four channels per thread (9)
    _dw("dw5_c32", (14, 14), 32, k=(5, 5), batch=2),        # 5x5: column window (6), LDS-tiled (2)
    _dw("dw5_c58", (14, 14), 58, k=(5, 5), batch=2),
    _dw("dw5_c64", (14, 14), 64, k=(5, 5), batch=2),
]

GEMM_CODES = [1, 2, 3, 5, 6, 7, 8, 9, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32]
DW_CODES = [1, 2, 3, 4, 5, 6, 7, 8, 9]
# (4, 10, 11 and 16 exist in measurement builds only: test_gpu_gemm256.py::test_losing_structures_are_not_in_the_product)

# ---- the kernels each forced code may report (q8igemm.hip:forced_plan / launch, operator-run.c, q8dwconv.hip) ----
_GENERIC = {f"q8_igemm_mfma_128x{w}{s}" for w in (32, 64, 128) for s in ("", "_c3")}   # the tile kernel (1; 13 off deconvolutions)
_DECONV_S2 = {"q8_deconv_s2_stream_3x3", "q8_deconv_s2_stream_4x4"}
FORCED_NAMES = {
    "gemm_kernel": {
        1: _GENERIC,
        2: {"q8_gemm_mfma_256x256", "q8_gemm_mfma_256x256_conv"},
        3: {"q8_conv_lds_mfma"},
        5: {"q8_pw_stream_mfma", "q8_pw_stream_d2s_mfma"},
        6: {"q8_pw_stream_gw_mfma", "q8_pw_stream_gwk_mfma"},
        7: {"q8_conv_stream_c3_mfma"},
        8: {"q8_conv_wave_mfma", "q8_conv_wave_ws_mfma", "q8_conv_wave_ws_c_mfma", "q8_conv_wave_ws_c16_mfma"},
        9: {"q8_pw_stream_longk_mfma"},
        12: {"q8_conv_wave_mfma"},
        13: _GENERIC | _DECONV_S2,
        14: {"q8_conv_c3rows_mfma", "q8_conv_c3rows32_mfma"},
        15: {"q8_gemm_mfma_256x256_lean"},
        20: {"q8_gemm_mfma_256x256_c"},
        21: {"q8_gemm_mfma_256x256_c_burst"},
        22: {"q8_conv_patch_mfma"},
        23: {"q8_gemm_mfma_256x256_c16"},
        24: {"q8_gemm_mfma_128x64_c16", "q8_gemm_mfma_128x128_c16"},
        25: {"q8_gemm_mfma_128x64_c16"},
        26: {"q8_gemm_mfma_128x128_c16"},
        27: {"q8_conv_wave_mfma", "q8_conv_wave_ws_mfma", "q8_conv_wave_ws_c_mfma"},
        28: {"q8_gemm_mfma_256x256_r16"},
        29: {"q8_gemm_mfma_128x32_u16", "q8_gemm_mfma_128x64_u16", "q8_gemm_mfma_128x128_u16"},
        30: {"q8_conv_c3rows_lds_mfma", "q8_conv_c3rows32_lds_mfma"},
        31: None,   # the dense image of a grouped 1x1 under the automatic choice: any GEMM kernel, operator_ran_dense()
        32: {"q8_conv_ws16s_mfma"},
    },
    "dwconv_kernel": {
        1: {"q8_dwconv_direct"},
        2: {"q8_dwconv_lds_3x3", "q8_dwconv_lds_5x5"},
        3: {"q8_dwconv_row_3x3"},
        4: {"q8_dwconv_mfma_3x3"},
        5: {"q8_dwconv_mfma_lds_3x3"},
        6: {"q8_dwconv_col_3x3", "q8_dwconv_col_3x3_dot4", "q8_dwconv_col_3x3_dot4_dilated", "q8_dwconv_col_5x5_dot4"},
        7: {"q8_dwconv_mfma16_3x3"},
        8: {"q8_dwconv_row_3x3_any"},
        9: {"q8_dwconv_direct4"},
    },
}
# Deconvolutions pin the offset-table kernel (deconvolution.c): only 1 (the phase GEMMs) and 13 (the stride-2 streaming
# kernel) change what runs; they are run with those codes and 0.
DECONV_CODES = {1: _GENERIC, 13: _DECONV_S2}

# Codes the product library refuses on every operator, with the reason
MUST_REFUSE = {
    ("gemm_kernel", 21): "the burst-read A/B structure of the centred 256x256 kernel exists in measurement builds only",
}

# ---- what each forced code must take at offset (0, 0) ----
ACCEPTS = {
    ("dwconv_kernel", 1): ["dw3_c27", "dw3_c32", "dw3_c58", "dw3_c64_s2", "dw3_c64_wide", "dw5_c27", "dw5_c32", "dw5_c58", "dw5_c64"],
    ("dwconv_kernel", 2): ["dw3_c32", "dw3_c64_s2", "dw3_c64_wide", "dw5_c32", "dw5_c64"],
    ("dwconv_kernel", 3): ["dw3_c32", "dw3_c64_s2", "dw3_c64_wide"],
    ("dwconv_kernel", 4): ["dw3_c32", "dw3_c64_s2", "dw3_c64_wide"],
    ("dwconv_kernel", 5): ["dw3_c32", "dw3_c64_s2", "dw3_c64_wide"],
    ("dwconv_kernel", 6): ["dw3_c32", "dw3_c64_s2", "dw3_c64_wide", "dw5_c32", "dw5_c64"],
    ("dwconv_kernel", 7): ["dw3_c32", "dw3_c64_wide"],
    ("dwconv_kernel", 8): ["dw3_c27", "dw3_c32", "dw3_c58", "dw3_c64_s2", "dw3_c64_wide"],
    ("dwconv_kernel", 9): ["dw3_c27", "dw3_c32", "dw3_c58", "dw3_c64_s2", "dw3_c64_wide", "dw5_c27", "dw5_c32", "dw5_c58", "dw5_c64"],
    ("gemm_kernel", 1): ["fc_k58_n58", "fc_k64_n64", "fc_k100_n100", "fc_k256_n256", "fc_k512_n512", "fc_k640_n64", "fc_k58_strided",
        "pw_c64_n64", "pw_c64_n60", "pw_c48_n40_strided", "pw_g2_25_88", "pw_g8_12_45", "pw_s2_128_256", "c33_16_16", "c33_32_32",
        "c33_48_48", "c33_64_64", "c33_64_256", "c33_32_32_mid", "c3_7x7_s2", "c3_3x3_s2", "dc_4x4_s2"],
    ("gemm_kernel", 2): ["fc_k64_n64", "fc_k256_n256", "fc_k512_n512", "fc_k640_n64", "pw_c64_n64", "pw_c64_n60", "pw_s2_128_256",
        "c33_16_16", "c33_32_32", "c33_48_48", "c33_64_64", "c33_64_256", "c33_32_32_mid"],
    ("gemm_kernel", 3): ["c33_32_32", "c33_64_64", "c33_32_32_mid"],
    ("gemm_kernel", 5): ["fc_k64_n64", "fc_k256_n256", "pw_c64_n64", "pw_c64_n60", "pw_s2_128_256"],
    ("gemm_kernel", 6): ["fc_k64_n64", "fc_k256_n256", "fc_k512_n512", "fc_k640_n64", "pw_c64_n64", "pw_c64_n60"],
    ("gemm_kernel", 7): ["c3_3x3_s2"],
    ("gemm_kernel", 8): ["c33_32_32", "c33_64_64", "c33_32_32_mid"],
    ("gemm_kernel", 9): ["fc_k512_n512", "fc_k640_n64"],
    ("gemm_kernel", 12): ["c33_32_32", "c33_64_64", "c33_32_32_mid"],
    ("gemm_kernel", 13): ["fc_k58_n58", "fc_k64_n64", "fc_k100_n100", "fc_k256_n256", "fc_k512_n512", "fc_k640_n64", "fc_k58_strided",
        "pw_c64_n64", "pw_c64_n60", "pw_c48_n40_strided", "pw_g2_25_88", "pw_g8_12_45", "pw_s2_128_256", "c33_16_16", "c33_32_32",
        "c33_48_48", "c33_64_64", "c33_64_256", "c33_32_32_mid", "c3_7x7_s2", "c3_3x3_s2", "dc_4x4_s2"],
    ("gemm_kernel", 14): ["c3_7x7_s2", "c3_3x3_s2"],
    ("gemm_kernel", 15): ["fc_k256_n256", "fc_k512_n512"],
    ("gemm_kernel", 20): ["fc_k512_n512"],
    ("gemm_kernel", 22): ["c33_64_256"],
    ("gemm_kernel", 23): ["fc_k512_n512"],
    ("gemm_kernel", 24): ["fc_k64_n64", "fc_k256_n256", "fc_k512_n512", "fc_k640_n64", "pw_c64_n64", "pw_c64_n60", "pw_s2_128_256"],
    ("gemm_kernel", 25): ["fc_k64_n64", "fc_k256_n256", "fc_k512_n512", "fc_k640_n64", "pw_c64_n64", "pw_c64_n60", "pw_s2_128_256"],
    ("gemm_kernel", 26): ["fc_k64_n64", "fc_k256_n256", "fc_k512_n512", "fc_k640_n64", "pw_c64_n64", "pw_c64_n60", "pw_s2_128_256"],
    ("gemm_kernel", 27): ["c33_32_32", "c33_64_64", "c33_32_32_mid"],
    ("gemm_kernel", 28): ["fc_k512_n512"],
    ("gemm_kernel", 29): ["fc_k58_n58", "fc_k64_n64", "fc_k100_n100", "fc_k256_n256", "fc_k512_n512", "fc_k640_n64", "fc_k58_strided",
        "pw_c64_n64", "pw_c64_n60", "pw_c48_n40_strided", "pw_g2_25_88", "pw_g8_12_45"],
    ("gemm_kernel", 30): ["c3_7x7_s2", "c3_3x3_s2"],
    ("gemm_kernel", 31): ["pw_g2_25_88", "pw_g8_12_45"],
    ("gemm_kernel", 32): ["c33_16_16", "c33_32_32", "c33_48_48", "c33_64_64", "c33_64_256", "c33_32_32_mid"],
}

# codes documented for "any base address": they take every offset of every case they take at (0, 0)
ANY_BASE = {("gemm_kernel", 29), ("dwconv_kernel", 1), ("dwconv_kernel", 8), ("dwconv_kernel", 9)}


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """(input, kernel, bias, expected output, quantization, output extent): once per case, for every code and offset"""
    if isinstance(case, FcCase):
        inp, kern, bias = fc_tensors(case)
        expected, quant = fc_expected(case, inp, kern, bias)
        return inp, kern, bias, expected, quant, None
    if isinstance(case, DeconvCase):
        inp, kern, bias = deconv_tensors(case)
        expected, quant, out_hw = deconv_expected(case, inp, kern, bias)
    else:
        inp, kern, bias = conv_tensors(case)
        expected, quant, out_hw = conv_expected(case, inp, kern, bias)
    return inp, kern, bias, expected, quant, out_hw


def run_case(lib, case, family, code, offsets):
    """Force `code`, run `case` at (input, output) `offsets`: (output, kernel name) or (None, status) when refused.
    The guard, FILL-on-refusal and unchanged-input checks are placed_run's."""
    inp, kern, bias, _, quant, out_hw = _oracle(case)
    io = dict(in_offset=offsets[0], out_offset=offsets[1])
    lib.set_option(family, code)
    try:
        if isinstance(case, FcCase):
            return fc_run(lib, case, quant, inp, kern, bias, **io)
        if isinstance(case, DeconvCase):
            return deconv_run(lib, case, quant, out_hw, inp, kern, bias, **io)
        if code == 31:
            return _run_dense(lib, case, quant, out_hw, inp, kern, bias, io)
        return conv_run(lib, case, quant, out_hw, inp, kern, bias, **io)
    except QnnpackError as e:
        return None, e.status
    finally:
        lib.set_option(family, 0)


def _create_conv(lib, case, kern, bias, quant):
    oscale, ozp = quant
    return lib.create_convolution2d_nhwc_q8(
        case.padding[0], case.padding[1], case.padding[2], case.padding[3],
        case.kernel_size[0], case.kernel_size[1], case.subsampling[0], case.subsampling[1],
        case.dilation[0], case.dilation[1], case.groups, case.gic, case.goc,
        case.izp, 1.0, case.kzp, 1.0, kern, bias, ozp, float(oscale), case.qmin, case.qmax, 0)


def _run_dense(lib, case, quant, out_hw, inp, kern, bias, io):
    """code 31 with operator_ran_dense(): the grouped operator's dense image, not a reroute to the grouped one"""
    op = _create_conv(lib, case, kern, bias, quant)
    try:
        out = placed_run(lib, op, inp, np.full(_oracle(case)[3].size, FILL, np.uint8), io["in_offset"], io["out_offset"], case.name,
                         lambda d_in, d_out: lib.setup_convolution2d_nhwc_q8(
                             op, case.batch, case.input_size[0], case.input_size[1], d_in, case.in_stride, d_out, case.out_stride))
        assert lib.operator_ran_dense(op), f"{case.name}: gemm_kernel 31 ran, but not on the dense image"
        return out, lib.operator_kernel(op)
    finally:
        lib.delete_operator(op)


def _names(family, case, code):
    if isinstance(case, DeconvCase):
        return DECONV_CODES[code]
    return FORCED_NAMES[family][code]


def _codes(cases, family, codes):
    out = []
    for case in cases:
        for code in ([0] + sorted(DECONV_CODES) if isinstance(case, DeconvCase) else [0] + codes):
            out.append(pytest.param(case, family, code, id=f"{case.name}-{family.split('_')[0]}{code}"))
    return out


MATRIX = _codes(GEMM_CASES, "gemm_kernel", GEMM_CODES) + _codes(DW_CASES, "dwconv_kernel", DW_CODES)


@pytest.mark.parametrize("case,family,code", MATRIX)
def test_forced_kernel_runs_right_or_refuses(qnnp, case, family, code):
    expected = _oracle(case)[3]
    taken = []
    for offsets in OFFSETS:
        out, got = run_case(qnnp, case, family, code, offsets)
        what = f"{case.name} {family} {code} at offsets {offsets}"
        if out is None:
            assert code != 0, f"{what}: the automatic choice refused a valid operator ({got.name})"
            assert got == Status.unsupported_parameter, f"{what}: refused with {got.name}"
            continue
        names = None if code == 0 else _names(family, case, code)
        assert got is not None, what
        assert names is None or got in names, f"{what}: ran {got}, not one of {sorted(names)} -- a forced kernel rerouted"
        assert (family, code) not in MUST_REFUSE, f"{what}: ran {got}; {MUST_REFUSE[(family, code)]}"
        assert_bytes_equal(out, expected, f"gfx950 {got} vs oracle [{what}]")
        taken.append(offsets)
    if (family, code) in ANY_BASE and (0, 0) in taken:
        assert taken == OFFSETS, f"{case.name}: {family} {code} is documented for any base address, took only {taken}"


@pytest.mark.parametrize("family,code", sorted(ACCEPTS), ids=lambda v: str(v))
def test_forced_kernel_takes_its_cases(qnnp, family, code):
    """a code that starts refusing everything fails here (the matrix above would only see refusals)"""
    by_name = {c.name: c for c in GEMM_CASES + DW_CASES}
    for name in ACCEPTS[(family, code)]:
        out, got = run_case(qnnp, by_name[name], family, code, (0, 0))
        assert out is not None, f"{name}: {family} {code} refused ({got.name}) at offset (0, 0)"


def test_every_forced_code_is_covered():
    """each code of each family is accepted somewhere or refused everywhere on purpose -- never neither"""
    for family, codes in (("gemm_kernel", GEMM_CODES), ("dwconv_kernel", DW_CODES)):
        for code in codes:
            assert ((family, code) in ACCEPTS) != ((family, code) in MUST_REFUSE), (family, code)
    assert set(FORCED_NAMES["gemm_kernel"]) == set(GEMM_CODES) and set(FORCED_NAMES["dwconv_kernel"]) == set(DW_CODES)


# ---- the two byte-streaming operators: code 0 only, every tensor offset ----
ADD_CASES = [pw.AddCase("add_flat_c64", 64, 64),                                   # 16-byte flat path (q8pointwise.hip)
             pw.AddCase("add_strided_c58", 37, 58, a_stride=61, b_stride=64, y_stride=59)]
GAP_CASES = [pw.GapCase("gap_c64_w49", 4, 49, 64), pw.GapCase("gap_c58_strided", 3, 30, 58, in_stride=61, out_stride=59)]


@pytest.mark.parametrize("case", ADD_CASES, ids=lambda c: c.name)
def test_add_at_every_offset(qnnp, case):
    a, b, _ = pw.add_tensors(case)
    expected = pw.add_expected(case, a, b)
    sa, sb, sy = case.strides
    op = qnnp.create_add_nc_q8(case.channels, case.a_zp, case.a_scale, case.b_zp, case.b_scale, case.y_zp, case.y_scale,
                               case.qmin, case.qmax, 0)
    try:
        for oa, oy in OFFSETS:
            ob = (oa + oy + 3) % 16 if (oa, oy) != (0, 0) else 0
            db = Guarded(b, ob)
            out = placed_run(qnnp, op, a, np.full(expected.size, FILL, np.uint8), oa, oy, f"{case.name} b+{ob}",
                             lambda d_a, d_y: qnnp.setup_add_nc_q8(op, case.batch, d_a, sa, db.view, sb, d_y, sy))
            db.assert_intact(f"{case.name} at ({oa}, {ob}, {oy}), b")
            assert_bytes_equal(out, expected, f"gfx950 {qnnp.operator_kernel(op)} vs oracle [{case.name} at ({oa}, {ob}, {oy})]")
    finally:
        qnnp.delete_operator(op)


@pytest.mark.parametrize("case", GAP_CASES, ids=lambda c: c.name)
def test_global_average_pooling_at_every_offset(qnnp, case):
    inp = pw.gap_tensors(case)
    expected = pw.gap_expected(case, inp)
    si, so = case.strides
    op = qnnp.create_global_average_pooling_nwc_q8(case.channels, case.in_zp, case.in_scale, case.out_zp, case.out_scale,
                                                   case.qmin, case.qmax, 0)
    try:
        for oi, oo in OFFSETS:
            out = placed_run(qnnp, op, inp, np.full(expected.size, FILL, np.uint8), oi, oo, case.name,
                             lambda d_in, d_out: qnnp.setup_global_average_pooling_nwc_q8(op, case.batch, case.width, d_in, si, d_out, so))
            assert_bytes_equal(out, expected, f"gfx950 {qnnp.operator_kernel(op)} vs oracle [{case.name} at ({oi}, {oo})]")
    finally:
        qnnp.delete_operator(op)


# ---- the fused inverted-residual block ("fused_kernel" 0 / 1 / 2: refusals at setup) ----
_BLOCK = (ConvCase("fb_expand", (28, 28), gic=24, goc=144, batch=2),
          _dw("fb_depthwise", (28, 28), 144, batch=2),
          ConvCase("fb_project", (28, 28), gic=144, goc=24, batch=2))
FUSED_NAMES = {0: {"q8_fused_strip", "q8_fused_block"}, 1: {"q8_fused_block"}, 2: {"q8_fused_strip"}}


@functools.lru_cache(maxsize=None)
def _block_oracle():
    """(block input, stages, block output): the three stand-alone operators' oracle chain, each one's output -- zero point
    and all -- the next one's input"""
    stages, x, izp = [], conv_tensors(_BLOCK[0])[0], None
    block_input = x
    for case in _BLOCK:
        if izp is not None:
            case = dataclasses.replace(case, izp=izp)
        _, kern, bias = conv_tensors(case)
        x, quant, _ = conv_expected(case, x, kern, bias)
        stages.append((case, kern, bias, quant))
        izp = int(quant[1])
    return block_input, stages, x


def _fused(lib, stages):
    ops = [_create_conv(lib, case, kern, bias, quant) for case, kern, bias, quant in stages]
    return ops, lib.create_fused_block(*ops)


def _fused_run(lib, op, inp, expected, offsets, what):
    cin, cout = _BLOCK[0].gic, _BLOCK[2].goc
    H, W = _BLOCK[0].input_size
    try:
        return placed_run(lib, op, inp, np.full(expected.size, FILL, np.uint8), offsets[0], offsets[1], what,
                          lambda d_in, d_out: lib.setup_fused_block(op, _BLOCK[0].batch, H, W, d_in, cin, d_out, cout)), lib.operator_kernel(op)
    except QnnpackError as e:
        return None, e.status


@pytest.mark.parametrize("code", [0, 1, 2])
def test_fused_block_runs_right_or_refuses(qnnp, code):
    inp, stages, expected = _block_oracle()
    qnnp.set_option("fused_kernel", code)
    ops, op = [], None
    try:
        ops, op = _fused(qnnp, stages)
        taken = []
        for offsets in OFFSETS:
            what = f"fused block, fused_kernel {code} at offsets {offsets}"
            out, got = _fused_run(qnnp, op, inp, expected, offsets, what)
            if out is None:
                assert got == Status.unsupported_parameter, f"{what}: refused with {got.name}"
                continue
            assert got in FUSED_NAMES[code], f"{what}: ran {got}"
            assert_bytes_equal(out, expected, f"gfx950 {got} vs oracle [{what}]")
            taken.append(offsets)
        assert (0, 0) in taken, f"fused_kernel {code} refused the block at offset (0, 0)"
    finally:
        qnnp.set_option("fused_kernel", 0)
        for h in ([op] if op else []) + ops:
            qnnp.delete_operator(h)


# ---- one operator, set up again and again at other base addresses: no plan kept under a stale key ----
RESETUP = [0, 1, 0, 3, 8]


@pytest.mark.parametrize("case,family,code", [
    (GEMM_CASES[7], "gemm_kernel", 0),     # pw_c64_n64: 16-byte streaming kernel at 0, the unaligned GEMM at 1 / 3
    (GEMM_CASES[0], "gemm_kernel", 29),
    (DW_CASES[1], "dwconv_kernel", 0),     # dw3_c32: column window at 0 / 8, sliding window on unaligned dwords at 1 / 3
    (DW_CASES[1], "dwconv_kernel", 9),
], ids=lambda v: getattr(v, "name", str(v)))
def test_resetup_at_other_base_addresses(qnnp, case, family, code):
    inp, kern, bias, expected, quant, _ = _oracle(case)
    qnnp.set_option(family, code)
    op = _create_conv(qnnp, case, kern, bias, quant) if isinstance(case, ConvCase) else qnnp.create_fully_connected_nc_q8(
        case.input_channels, case.output_channels, case.izp, 1.0, case.kzp, 1.0, kern, bias, quant[1], float(quant[0]),
        case.qmin, case.qmax, 0)
    try:
        names = []
        for off in RESETUP:
            what = f"{case.name} {family} {code}, setup at offset {off}"
            if isinstance(case, FcCase):
                setup = lambda d_in, d_out: qnnp.setup_fully_connected_nc_q8(op, case.batch, d_in, case.in_stride, d_out, case.out_stride)
            else:
                setup = lambda d_in, d_out: qnnp.setup_convolution2d_nhwc_q8(
                    op, case.batch, case.input_size[0], case.input_size[1], d_in, case.in_stride, d_out, case.out_stride)
            out = placed_run(qnnp, op, inp, np.full(expected.size, FILL, np.uint8), off, off, what, setup)
            names.append(qnnp.operator_kernel(op))
            assert_bytes_equal(out, expected, f"gfx950 {names[-1]} vs oracle [{what}]")
        assert names[0] == names[2], names
    finally:
        qnnp.set_option(family, 0)
        qnnp.delete_operator(op)


def test_resetup_fused_block_at_other_base_addresses(qnnp):
    inp, stages, expected = _block_oracle()
    ops, op = _fused(qnnp, stages)
    try:
        for off in RESETUP:
            what = f"fused block, setup at offset {off}"
            out, got = _fused_run(qnnp, op, inp, expected, (off, off), what)
            if out is None:    # (the caller's cue to run the stand-alone operators; placed_run checked the output is untouched)
                assert off % 4 != 0 and got == Status.unsupported_parameter, f"{what}: refused ({got.name})"
                continue
            assert_bytes_equal(out, expected, f"gfx950 {got} vs oracle [{what}]")
    finally:
        for h in [op] + ops:
            qnnp.delete_operator(h)
