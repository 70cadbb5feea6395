"""The output table folded behind a convolution (qnnp_gfx950_attach_output_table, output-table.c): cases, their oracle
expectation and the drivers of tests/test_output_table_gpu.py (numpy and the scalar oracle only here, no GPU).

A `Case` is one convolution (pointwise, depthwise, dense, or a fully connected layer) with a table behind it. Its
expectation is the ORACLE's convolution bytes (oracle.o1: accumulators, then the scalar Q31 requantization with the case's
clamp) mapped through the table in numpy -- table[b] for every pixel byte, the bytes between strided pixels left at FILL.

Tables: a seeded random permutation of 0..255 (a missed, doubled or misplaced lookup changes nearly every byte; an identity
or monotone table would hide it), or the hardswish table of tests/_multiply.py, which the library's hardswish operator is
held to elsewhere.

Requantization classes: `mode` is a class of tests/_fused.py's table (0 1 2 3 6 7 8) and the stage is made by that file's
recipe, restated here for any window: weights around the kernel zero point as wide as spreads the outputs over some 45
steps, a bias that puts every channel at its own spot of the range, a quantile clamp in the clamped classes.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import _fused as F
import _lut
import _multiply
from _cases import output_quantization, seed_for
from _runner import FILL
from oracle import o1

f32 = np.float32
HARDSWISH = dict(input_scale=0.046875, output_zero_point=21, output_scale=0.03125, output_min=0, output_max=255)
PW_KERNELS = ("q8_pw_stream_mfma", "q8_pw_stream_longk_mfma", "q8_pw_stream_gw_mfma", "q8_pw_stream_gwk_mfma")
DW_KERNELS = ("q8_dwconv_col_3x3", "q8_dwconv_col_3x3_dot4", "q8_dwconv_col_3x3_dot4_dilated", "q8_dwconv_col_5x5_dot4")


@dataclass(frozen=True)
class Case:
    name: str
    gic: int = 24                       # pointwise / dense: input channels; depthwise: 1
    goc: int = 48
    groups: int = 1                     # depthwise: the channel count
    batch: int = 2
    size: Tuple[int, int] = (5, 7)      # 2 x 5 x 7 = 70 rows: a partial last 32-row unit
    kernel: int = 1                     # square window, "same" padding
    stride: int = 1
    dilation: int = 1
    out_extra: int = 0                  # output pixel stride = channels + out_extra
    family: str = "gemm_kernel"         # the forcing hook the code goes to
    code: int = 0
    mode: Optional[int] = None          # requantization class (tests/_fused.py), or None: the testers' quantization
    clamp: Tuple[int, int] = (0, 255)
    table: str = "perm"                 # "perm" | "hardswish"
    kzp: int = 127
    wide: bool = False                  # weights over all of 0..255 (outside the depthwise dot-product flavour's range)
    fc: bool = False                    # a fully connected layer of `batch` rows
    want: str = ""                      # kernel name
    folded: int = 1

    @property
    def channels(self) -> int:
        return self.groups * self.goc

    @property
    def out_stride(self) -> int:
        return self.channels + self.out_extra

    @property
    def pad(self) -> int:
        return self.dilation * (self.kernel // 2)


class Problem:
    """the tensors of a case, how to create its operator, and the oracle's bytes"""

    def __init__(self, case: Case):
        self.case = c = case
        rng = np.random.default_rng(seed_for("output_table/" + c.name))
        self.izp = 119
        cin = c.groups * c.gic
        h, w = (1, 1) if c.fc else c.size
        self.x = rng.integers(0, 256, c.batch * h * w * cin, dtype=np.uint8)
        self.shape = o1.conv_shape(c.batch, h, w, (c.pad,) * 4, (c.kernel,) * 2, (c.stride,) * 2, (c.dilation,) * 2,
                                   c.groups, c.gic, c.goc)
        self.out_hw = o1.conv_output_hw(self.shape)
        self.rows = c.batch * self.out_hw[0] * self.out_hw[1]
        kshape = (c.groups, c.goc, c.kernel, c.kernel, c.gic)
        reduction = c.kernel * c.kernel * c.gic
        acc_of = lambda kernel, bias: o1.conv2d_acc(self.shape, self.x, kernel, bias, self.izp, c.kzp).reshape(-1, c.channels)
        self.qmin, self.qmax = c.clamp
        if c.mode is None:
            if c.wide:
                self.kernel = rng.integers(0, 256, kshape, dtype=np.uint8)
            else:
                self.kernel = np.clip(np.rint(c.kzp + rng.normal(0.0, 20.0, kshape)), 0, 255).astype(np.uint8)
            self.bias = rng.integers(-5000, 5000, c.channels).astype(np.int32)
            acc = acc_of(self.kernel, self.bias)
            oscale, self.ozp = output_quantization(acc)
            self.kernel_scale, self.output_scale = 1.0, float(oscale)
            self.scale = f32(f32(1.0) * f32(1.0) / f32(oscale))
        else:
            # tests/_fused.py make_stage, for any window
            self.kernel_scale, self.output_scale, self.scale = F.scale_arguments(F.MODE_SCALE[c.mode])
            sigma_a = max(8.0, float(np.sqrt(np.mean((self.x.astype(np.float64) - self.izp) ** 2))))
            sigma_w = min(60.0, 45.0 / (float(self.scale) * sigma_a * np.sqrt(reduction)))
            self.kernel = F._weights(rng, kshape, 0 if c.groups > 1 else 1, c.kzp, sigma_w)
            self.ozp = int(rng.integers(70, 186))
            if c.mode == 8:
                target = rng.uniform(8.0, 248.0, c.channels)
                bias = np.rint((target - self.ozp) / float(self.scale))
                self.bias = np.clip(bias, -2 ** 31 + 2 ** 22, 2 ** 31 - 2 ** 22).astype(np.int32)
            else:
                acc0 = acc_of(self.kernel, np.zeros(c.channels, np.int32))
                spot = rng.uniform(0.08, 0.25, c.channels) * rng.choice([-1.0, 1.0], c.channels) * 255 + (127.5 - self.ozp)
                self.bias = np.clip(np.rint(spot / float(self.scale) - acc0.mean(axis=0)), -2 ** 29, 2 ** 29).astype(np.int32)
                if c.mode == 6:
                    self.bias[[1, c.channels - 2]] = [2 ** 30 - 1000, -(2 ** 30 - 1000)]
            acc = acc_of(self.kernel, self.bias)
            if c.mode in F.CLAMPED_MODES:
                y = o1.q31_requantize(acc, self.scale, self.ozp, 0, 255)
                self.qmin, self.qmax = int(np.quantile(y, 0.2)), int(np.quantile(y, 0.8))
            got = F.mode_of(F.stage_class(self.scale, self.ozp, self.qmin, self.qmax, self.bias, reduction))
            assert got == c.mode, (c.name, c.mode, got)
        self.conv = o1.q31_requantize(acc, self.scale, self.ozp, self.qmin, self.qmax)      # [rows, channels]
        if c.table == "hardswish":
            self.table = _multiply.hardswish_table(self.ozp, HARDSWISH["input_scale"], HARDSWISH["output_zero_point"],
                                                   HARDSWISH["output_scale"], HARDSWISH["output_min"], HARDSWISH["output_max"])
        else:
            self.table = _lut.permutation(seed_for("output_table/table/" + c.name) & 0xFFFF)
        assert self.table.dtype == np.uint8 and self.table.size == 256

    def flat(self, pixels: np.ndarray, out_stride: Optional[int] = None) -> np.ndarray:
        """[rows, channels] bytes as the strided output buffer, FILL between the pixels"""
        stride = out_stride or self.case.out_stride
        rows, ch = pixels.shape
        out = np.full((rows - 1) * stride + ch, FILL, np.uint8)
        np.lib.stride_tricks.as_strided(out, shape=(rows, ch), strides=(stride, 1))[...] = pixels
        return out

    def plain(self) -> np.ndarray:
        return self.flat(self.conv)

    def expected(self, table: Optional[np.ndarray] = None) -> np.ndarray:
        return self.flat((self.table if table is None else table)[self.conv])

    def not_degenerate(self) -> None:
        """the clamp bites where one is set, the outputs have many values, and the table moves nearly all of them"""
        c = self.case
        # (class 8: no dot product moves an output, every channel is the constant its bias makes)
        assert np.unique(self.conv).size >= (min(6, c.channels) if c.mode == 8 else 24), (c.name, np.unique(self.conv).size)
        if (self.qmin, self.qmax) != (0, 255):
            # (the testers' quantization maps the accumulator range onto 0..255: both ends are there to be clamped)
            assert self.conv.min() == self.qmin and self.conv.max() == self.qmax, (c.name, self.conv.min(), self.conv.max())
            inside = (self.conv > self.qmin) & (self.conv < self.qmax)
            assert inside.mean() > 0.5, c.name
        if c.table == "perm":
            assert np.mean(self.table[self.conv] != self.conv) > 0.9, c.name

    # ---- operators ----
    def create(self, lib):
        c = self.case
        if c.fc:
            return lib.create_fully_connected_nc_q8(c.gic, c.goc, self.izp, 1.0, c.kzp, self.kernel_scale,
                                                    self.kernel.reshape(c.goc, c.gic), self.bias, self.ozp, self.output_scale,
                                                    self.qmin, self.qmax, 0)
        return lib.create_convolution2d_nhwc_q8(c.pad, c.pad, c.pad, c.pad, c.kernel, c.kernel, c.stride, c.stride, c.dilation,
                                                c.dilation, c.groups, c.gic, c.goc, self.izp, 1.0, c.kzp, self.kernel_scale,
                                                self.kernel, self.bias, self.ozp, self.output_scale, self.qmin, self.qmax, 0)

    def setup(self, lib, op, d_in, d_out, out_stride: Optional[int] = None):
        c = self.case
        stride = out_stride or c.out_stride
        if c.fc:
            lib.setup_fully_connected_nc_q8(op, c.batch, d_in, c.gic, d_out, stride)
        else:
            lib.setup_convolution2d_nhwc_q8(op, c.batch, c.size[0], c.size[1], d_in, c.groups * c.gic, d_out, stride)

    def create_table(self, lib, table: Optional[np.ndarray] = None):
        c = self.case
        if c.table == "hardswish" and table is None:
            return lib.create_hardswish_nc_q8(c.channels, self.ozp, HARDSWISH["input_scale"], HARDSWISH["output_zero_point"],
                                              HARDSWISH["output_scale"], HARDSWISH["output_min"], HARDSWISH["output_max"], 0)
        return lib.create_lut_nc_x8(c.channels, self.table if table is None else table, 0)


@functools.lru_cache(maxsize=None)
def problem(case: Case) -> Problem:
    return Problem(case)


def run_chain_and_attached(lib, case: Case):
    """The library's own chain (convolution, then the stand-alone table operator in place on its output) and the convolution
    with the table attached, each on a guarded output; returns (chain bytes, attached bytes, kernel name, folded)."""
    from _gpu import Guarded, to_device
    p = problem(case)
    d_in = to_device(p.x)
    blank = np.full(p.plain().size, FILL, np.uint8)
    d_chain, d_one = Guarded(blank, 0), Guarded(blank, 0)
    conv, lut = p.create(lib), p.create_table(lib)
    try:
        lib.set_option(case.family, case.code)
        p.setup(lib, conv, d_in, d_chain.view)
        assert lib.operator_table_folded(conv) == -1
        lib.run_operator(conv)
        plain_name = lib.operator_kernel(conv)
        lib.setup_lut_nc_x8(lut, p.rows, d_chain.view, case.out_stride, d_chain.view, case.out_stride)
        lib.run_operator(lut)
        chain = d_chain.read()
        d_chain.assert_intact(f"{case.name}: chain output")
        lib.attach_output_table(conv, lut)
        lib.delete_operator(lut)                # the 256 bytes were copied
        lut = None
        p.setup(lib, conv, d_in, d_one.view)
        lib.run_operator(conv)
        got = d_one.read()
        d_one.assert_intact(f"{case.name}: output of the convolution with the table attached")
        name, folded = lib.operator_kernel(conv), lib.operator_table_folded(conv)
        assert name == plain_name, f"{case.name}: the attachment changed the kernel, {plain_name} -> {name}"
    finally:
        lib.set_option(case.family, 0)
        lib.delete_operator(conv)
        if lut is not None:
            lib.delete_operator(lut)
    return chain, got, name, folded


def hold(lib, case: Case):
    """the case against the oracle and against the library's chain; kernel name and fold as the case states them"""
    from _runner import assert_bytes_equal
    p = problem(case)
    p.not_degenerate()
    chain, got, name, folded = run_chain_and_attached(lib, case)
    what = f"{case.name} [{name}, folded {folded}]"
    assert_bytes_equal(chain, p.expected(), what + ": the library's chain against the oracle")
    assert_bytes_equal(got, p.expected(), what + ": the attached table against the oracle")
    assert np.array_equal(got, chain), what + ": differs from the library's chain"
    if case.want:
        assert name == case.want, f"{case.name}: ran {name}, expected {case.want}"
    else:
        assert name not in PW_KERNELS + DW_KERNELS, f"{case.name}: ran {name}, expected a kernel without a table flavour"
    assert folded == case.folded, f"{case.name}: table_folded {folded} on {name}, expected {case.folded}"
    return name, folded
