"""The cases of tests/test_large_guards_gpu.py and the size guards they stand on, restated in Python.

A Pair is one term of one guard: `case` is the largest tensor the guard accepts, and the same case with one more image
(or row) is the smallest it refuses. `guard(case)` restates the guard's size expressions as {term: (value, bound)} -- the
kernel takes the tensor while every value is BELOW its bound -- with the file and function it restates in its docstring.
tests/test_large_guard_cases_host.py holds every pair to its arithmetic on the CPU (the intended term, and only that one,
crosses between the two sizes; both sizes pass the operator's setup limits and fit the memory budget of one case);
the GPU file runs them. Batch counts are computed here from the bounds, never written down.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, Optional

import _large as lg
from _cases import ConvCase, DeconvCase, FcCase
from oracle import o1

B31, B32 = 1 << 31, 1 << 32
ROWS = 37                   # rows per unit of the row-wise problems (test_gpu_large_tensors.ROWS)


# ---- geometry ----
def output_hw(case):
    H, W = case.input_size
    shape = o1.conv_shape(1, H, W, case.padding, case.kernel_size, case.subsampling, case.dilation, case.groups, case.gic,
                          case.goc, case.in_stride)
    if isinstance(case, DeconvCase):
        return o1.deconv_output_hw(shape, case.adjustment)
    return o1.conv_output_hw(shape)


def spans(case):
    """(input span, output span) in bytes, as the operator's setup computes them"""
    if isinstance(case, FcCase):
        return ((case.batch - 1) * case.in_stride + case.input_channels,
                (case.batch - 1) * case.out_stride + case.output_channels)
    H, W = case.input_size
    oh, ow = output_hw(case)
    return ((case.batch * H * W - 1) * case.in_stride + case.groups * case.gic,
            (case.batch * oh * ow - 1) * case.out_stride + case.groups * case.goc)


def nbytes(case) -> int:
    """device memory of the case at its peak (test_gpu_large_tensors.Problem.nbytes): both tensors and the comparison's chunks"""
    return sum(spans(case)) + 2 * lg.CHUNK


def setup_limits(case) -> Dict[str, tuple]:
    """{limit: (value, largest accepted)} of convolution.c / deconvolution.c (rows and bytes per input image) and
    fully-connected.c (rows) at setup"""
    if isinstance(case, FcCase):
        return {"rows": (case.batch, (B32 - 1) // 2)}
    H, W = case.input_size
    oh, ow = output_hw(case)
    return {"rows": (case.batch * oh * ow, (B32 - 1) // 2), "image bytes": (H * W * case.in_stride, B31 - 1)}


# ---- the guards ----
def c3rows_guard(case: ConvCase):
    """q8convc3.hip: conv_c3rows_supported and conv_c3rows32_supported (the same four size terms)"""
    oh, ow = output_hw(case)
    segs, pairs = (ow + 15) // 16, (oh + 1) // 2
    units = case.batch * pairs * segs
    return {"input": (spans(case)[0], B31), "output": (case.batch * oh * ow * case.out_stride, B31),
            "units*segs": (units * segs, B32), "units*pairs": (units * pairs, B32)}


def c3lds_plan(case: ConvCase) -> Optional[dict]:
    """q8convc3.hip: c3lds_plan for a 16-byte aligned base: None where the LDS flavour leaves the shape to the register
    flavour, else its bands and the product its one batch-dependent term bounds"""
    H, W = case.input_size
    oh, ow = output_hw(case)
    (kh, kw), (sh, sw), pad_left = case.kernel_size, case.subsampling, case.padding[3]
    segs, pairs = (ow + 15) // 16, (oh + 1) // 2
    if (W * 3) % 16 or (H * W * 3) % 16:
        return None
    c0 = (pad_left * 3 + 15) // 16
    last_end, data_end = ((ow - 1) * sw + kw) * 3, (pad_left + W) * 3
    cpr = c0 + W * 3 // 16 + (max(last_end - data_end, 0) + 15) // 16 + 1
    cpr += 1 - cpr % 2
    best = 0
    for ppb in range(1, min(pairs, 16) + 1):
        if ((2 * ppb - 1) * sh + kh) * cpr * 16 > 24 * 1024:
            break
        if best == 0 or (ppb * segs) % 4 == 0 or (best * segs) % 4 != 0:
            best = ppb
    if best == 0:
        return None
    bands = (pairs + best - 1) // best
    nrows = (2 * best - 1) * sh + kh
    if nrows * cpr * cpr >= B32:
        return None
    return {"bands": bands, "pairs": pairs, "wgs*bands": case.batch * bands * bands, "grid": case.batch * bands * 256}


def c3lds_guard(case: ConvCase):
    """q8convc3.hip: conv_c3rows_supported's terms and the two batch terms of c3lds_plan (a shape its plan takes)"""
    plan = c3lds_plan(case)
    return dict(c3rows_guard(case), **{"wgs*bands": (plan["wgs*bands"], B32), "grid": (plan["grid"], B32)})


def stream_c3_guard(case: ConvCase):
    """q8convc3s.hip: convstream_c3_plan, the condition of the staged flavour (the unstaged one takes what fails it)"""
    oh, ow = output_hw(case)
    return {"input": (spans(case)[0], B31), "table": (oh * ow * case.kernel_size[0] * case.kernel_size[1] * 4, B31)}


def gw_guard(case: FcCase):
    """q8pwconv.hip: pwstream_gw_plan"""
    n_pad = (case.output_channels + 31) // 32 * 32
    return {"input": ((case.batch - 1) * case.in_stride + case.input_channels, B31),
            "units": ((case.batch + 31) // 32 * (n_pad // 32), B31)}


def dwmfma16_plan(case: ConvCase, cu_count: int = 256):
    """q8dwmfma16.hip: dwmfma16_plan. (segs, and with it the third term, depends on the device's CU count only while
    batch x strips x channel groups is below 12 waves per CU: the host tier asserts that the cases are far above it.)"""
    H, W = case.input_size
    oh, ow = output_hw(case)
    blocks = case.groups // 16
    tn = 3 if blocks % 3 == 0 else (2 if blocks % 2 == 0 else 1)
    cgroups, strips = blocks // tn, (ow + 15) // 16
    per_seg = case.batch * strips * cgroups
    segs = max(1, min((cu_count * 12 + per_seg - 1) // per_seg, max(oh // 9, 1)))
    toh = ((oh + segs - 1) // segs + 5) // 6 * 6
    slabs = (oh + toh - 1) // toh
    waves = per_seg * slabs
    return {"input": (case.batch * H * W * case.in_stride, B31), "output": (case.batch * oh * ow * case.out_stride, B31),
            "(waves+8)*dmax": ((waves + 8) * max(strips, slabs, cgroups), B32), "grid": ((waves + 3) // 4 * 256, B32)}, per_seg


def dwmfma16_guard(case: ConvCase):
    return dwmfma16_plan(case)[0]


def deconv_s2_guard(case: DeconvCase):
    """q8deconv.hip: qnnp_hip_deconv_s2_run"""
    H, W = case.input_size
    oh, ow = output_hw(case)
    bh, bw = (oh - 1 + case.padding[0]) // 2 + 1, (ow - 1 + case.padding[3]) // 2 + 1
    return {"input": (case.batch * H * W * case.in_stride, B32), "output": (case.batch * oh * ow * case.out_stride, B32),
            "bases+32": (case.batch * bh * bw + 32, B31)}


def crossed(terms) -> set:
    return {t for t, (value, bound) in terms.items() if value >= bound}


def last_below(bound: int, per_unit: int) -> int:
    """the most units of per_unit bytes (or index steps) whose total stays below `bound`"""
    return (bound - 1) // per_unit


# ---- kernel names ----
C3_REG, C3_LDS = {"q8_conv_c3rows_mfma"}, {"q8_conv_c3rows_lds_mfma"}
C3_REG32, C3_LDS32 = {"q8_conv_c3rows32_mfma"}, {"q8_conv_c3rows32_lds_mfma"}
C3_STREAM = {"q8_conv_stream_c3_mfma"}
GW, GWK, LONGK = {"q8_pw_stream_gw_mfma"}, {"q8_pw_stream_gwk_mfma"}, {"q8_pw_stream_longk_mfma"}
DW_M16 = {"q8_dwconv_mfma16_3x3"}
DECONV_S2 = {"q8_deconv_s2_stream_3x3"}
PHASE_GEMM = {f"q8_igemm_mfma_128x{w}" for w in (32, 64, 128)}
D2S = {"q8_pw_stream_d2s_mfma"}


@dataclasses.dataclass(frozen=True)
class Pair:
    name: str
    case: object                    # the last accepted size; one more image / row is the first refused
    guard: Callable                 # case -> {term: (value, bound)}
    term: str                       # the term that is crossed between the two sizes
    family: str
    forced: dict                    # {forced code: the kernels it must report at the last accepted size}
    auto: Optional[set] = None      # the kernels the automatic choice runs at the last accepted size; None: it runs another
    past: Optional[set] = None      # the kernels the automatic choice must run past the bound; None: any but the pair's

    @property
    def refused(self):
        return dataclasses.replace(self.case, name=f"{self.case.name}_refused", batch=self.case.batch + 1)

    @property
    def names(self) -> set:
        return set().union(*self.forced.values())


def _c3(name, hw, k, pad, stride, n, batch):
    return ConvCase(name, hw, (k, k), (pad,) * 4, subsampling=(stride, stride), gic=3, goc=n, batch=batch)


def _dw16(name, hw, c, batch, **kw):
    return ConvCase(name, hw, (3, 3), (1, 1, 1, 1), groups=c, gic=1, goc=1, batch=batch, **kw)


def _up(name, cin, n, batch, adjustment=(0, 0)):
    return DeconvCase(name, (16, 16), (3, 3), (1, 1, 1, 1), subsampling=(2, 2), gic=cin, goc=n, batch=batch, adjustment=adjustment)


# 1.1  3x3 / stride 2 / pad 1 on 64 x 64 x 3: 12288 bytes per image in, 32 x 32 pixels out
C3_OUT_LAST = last_below(B31, 32 * 32 * 32)               # 3 -> 32: the output term
C3_IN_LAST = last_below(B31, 64 * 64 * 3)                 # 3 -> 8: the input term
# 1.2  2048 x 2 x 3: 512 row pairs of one segment, units * pairs = batch * 512 * 512; 2 x 16384 x 3: one row pair of 512
# segments, units * segs = batch * 512 * 512
C3_DIV_LAST = last_below(B32, 512 * 512)
# 1.4  the LDS flavour's grid, one workgroup of 256 work-items per image and band, below 2^32 work-items: 1 x 16 x 3 images
# under a 3x3 window at stride 1 x 16 are one output pixel, one band and 48 bytes each
C3_GRID_LAST = last_below(B32, 256)
# 1.3  7x7 / stride 2 / pad 3 on 32 x 32 x 3, 3 -> 64: 16 x 16 x 64 bytes per image out; at stride 3 with 16 channels an image
# writes 11 x 11 x 16 = 1936 bytes against the 3072 it holds, and the input term binds first
C3_32_OUT_LAST = last_below(B31, 16 * 16 * 64)
C3_32_IN_LAST = last_below(B31, 32 * 32 * 3)
# 2.1  64 -> 64 rows: the span (rows - 1) * 64 + 64
GW_LAST = last_below(B31, 64)
# 3    16 channels at 56 x 56, one tensor with 32-byte pixels
M16_LAST = last_below(B31, 56 * 56 * 32)
# 3.3  1 x 1 images of 1040 channels: 65 channel blocks (coprime to 6: one block per wave), so waves = 65 * batch and
# dmax = 65: (65 * batch + 8) * 65 < 2^32, with 66 M waves -- a grid of 2^32 work-items is 2^26 = 67 M waves
M16_WAVES_LAST = (last_below(B32, 65) - 8) // 65
# 3.4  the launch's grid, four waves of 64 work-items per workgroup, below 2^32 work-items: 1 x 1 images of 560 channels
# are 35 waves each (this shape first ran at the (waves+8)*dmax bound of 3.5 M images, where the grid had wrapped)
M16_GRID_LAST = 4 * last_below(B32, 256) // 35
# 4.1  16 x 16 images: 32 x 32 x 32 bytes out with adjustment (1, 1); 16 x 16 x 128 bytes in
UP_LAST = last_below(B32, 32 * 32 * 32)

_C3 = {14: C3_REG, 30: C3_LDS}
_C3_32 = {14: C3_REG32, 30: C3_LDS32}

PAIRS = [
    Pair("c3rows_output", _c3("c3_64x64_n32", (64, 64), 3, 1, 2, 32, C3_OUT_LAST), c3rows_guard, "output", "gemm_kernel", _C3, C3_LDS),
    Pair("c3rows_input", _c3("c3_64x64_n8", (64, 64), 3, 1, 2, 8, C3_IN_LAST), c3rows_guard, "input", "gemm_kernel", _C3, C3_LDS),
    Pair("c3rows_units_pairs", _c3("c3_2048x2_n8", (2048, 2), 3, 1, 2, 8, C3_DIV_LAST), c3rows_guard, "units*pairs", "gemm_kernel",
         {14: C3_REG}, C3_REG),
    Pair("c3rows_units_segs", _c3("c3_2x16384_n8", (2, 16384), 3, 1, 2, 8, C3_DIV_LAST), c3rows_guard, "units*segs", "gemm_kernel",
         {14: C3_REG}, C3_REG),
    Pair("c3lds_grid", ConvCase("c3_1x16_s1x16_n8", (1, 16), (3, 3), (1, 1, 1, 1), subsampling=(1, 16), gic=3, goc=8, batch=C3_GRID_LAST),
         c3lds_guard, "grid", "gemm_kernel", {30: C3_LDS}, C3_LDS, C3_REG),
    Pair("c3rows32_output", _c3("c3_7x7_32x32_n64", (32, 32), 7, 3, 2, 64, C3_32_OUT_LAST), c3rows_guard, "output", "gemm_kernel",
         _C3_32, C3_LDS32),
    Pair("c3rows32_input", _c3("c3_7x7_s3_32x32_n16", (32, 32), 7, 3, 3, 16, C3_32_IN_LAST), c3rows_guard, "input", "gemm_kernel",
         _C3_32, C3_LDS32),
    Pair("gw_input", FcCase("gw_64_64", GW_LAST, 64, 64), gw_guard, "input", "gemm_kernel", {6: GW}),
    Pair("dwmfma16_output", _dw16("m16_c16_o32", (56, 56), 16, M16_LAST, output_pixel_stride=32), dwmfma16_guard, "output",
         "dwconv_kernel", {7: DW_M16}),
    Pair("dwmfma16_input", _dw16("m16_c16_i32", (56, 56), 16, M16_LAST, input_pixel_stride=32), dwmfma16_guard, "input",
         "dwconv_kernel", {7: DW_M16}),
    Pair("dwmfma16_waves", _dw16("m16_c1040_1x1", (1, 1), 1040, M16_WAVES_LAST), dwmfma16_guard, "(waves+8)*dmax", "dwconv_kernel",
         {7: DW_M16}),
    Pair("dwmfma16_grid", _dw16("m16_c560_1x1", (1, 1), 560, M16_GRID_LAST), dwmfma16_guard, "grid", "dwconv_kernel", {7: DW_M16}),
    Pair("deconv_s2_output", _up("up_32_32_adjust", 32, 32, UP_LAST, (1, 1)), deconv_s2_guard, "output", "gemm_kernel",
         {13: DECONV_S2}, DECONV_S2, PHASE_GEMM),
    Pair("deconv_s2_input", _up("up_128_32", 128, 32, UP_LAST), deconv_s2_guard, "input", "gemm_kernel", {13: DECONV_S2}, DECONV_S2,
         PHASE_GEMM),
]
PAIR_IDS = [p.name for p in PAIRS]

# 1.5  q8_conv_stream_c3_mfma (code 7): the staged flavour up to an input of 2^31 - 1 bytes, the unstaged one from 2^31, one
# name for both; and 3 -> 32 with an output past 2^32 (131072 images write 2^32 bytes)
STREAM_C3 = [
    _c3("c3s_64x64_n16_staged_last", (64, 64), 3, 1, 2, 16, C3_IN_LAST),
    _c3("c3s_64x64_n16_unstaged_first", (64, 64), 3, 1, 2, 16, C3_IN_LAST + 1),
    _c3("c3s_64x64_n32_out_past_4g", (64, 64), 3, 1, 2, 32, B32 // (32 * 32 * 32) + 3),
]

# 2.3  q8_pw_stream_longk_mfma (code 9): pwstream_longk_plan and plan_staged hold no size term (LDS, channel and K conditions only), so
# it is run past 2^32 on each side: 512 -> 64 (K blocks 16: the 20-block flavour) and 272 -> 256 (9 blocks: the 12-block one)
LONGK_CASES = [
    FcCase("longk_512_64_in_past_4g", (1 << 23) + 7, 512, 64),
    FcCase("longk_272_256_out_past_4g", (1 << 24) + 7, 272, 256),
]

# 2.2  q8_pw_stream_gwk_mfma: 512 -> 64 over rows 2^25 bytes apart: 64 rows span 2^31 - 2^25 + 512 bytes, 65 rows 2^31 + 512
GWK_STRIDE = 1 << 25
GWK_LAST = (B31 - 1 - 512) // GWK_STRIDE + 1
GWK_CASE = FcCase("gwk_512_64_stride_2p25", GWK_LAST, 512, 64, input_stride=GWK_STRIDE)

# 4.2  q8_pw_stream_d2s_mfma: 2x2 / stride 2, 64 -> 32 at 14 x 14: 28 x 28 x 32 bytes out per image
D2S_CASE = DeconvCase("d2s_2x2_64_32_out_past_4g", (14, 14), (2, 2), subsampling=(2, 2), gic=64, goc=32, batch=B32 // (28 * 28 * 32) + 3)

# 5  the residual add folded into a 16 -> 64 pointwise layer: output and residual past 2^32
RESIDUAL_ROWS = (1 << 26) + 7

# 7  per-channel operators
PC_FC_ROWS = (1 << 26) + 7
PC_DW_BATCH = B32 // (28 * 28 * 58) + 3

# 8  multiply: three b rows 2^31 + 16 bytes apart in a, b and the product; + 17: a stride that is 1 (mod 4)
MUL_STRIDE_X16 = B31 + 16
MUL_STRIDE_X1 = B31 + 17
