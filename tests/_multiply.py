"""Cases and drivers for the product's multiply operator (qnnp_gfx950_*_multiply_nc_q8) and for the two table builders
beside it, hardswish and hardsigmoid (qnnp_gfx950_create_{hardswish,hardsigmoid}_nc_q8).

No reference operator exists to compare with, so the expectations come from the oracle that is already there:

 * multiply: oracle.o1.q31_requantize -- the reference's scalar qnnp_q31_requantize -- on the int32 products formed in
   numpy, with ratio = float32(float32(a_scale) * float32(b_scale)) / float32(product_scale);
 * the tables: the formulas of include/qnnpack_gfx950.h evaluated in numpy float32, one rounding per operation.

Every output buffer starts filled with FILL; the bytes between strided rows must come back as FILL.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from oracle import o1

FILL = 0xA5


def _seed(name: str) -> int:
    return 0x3A11 ^ (zlib.crc32(name.encode()) & 0x7FFFFFFF)


@dataclass(frozen=True)
class Quant:
    """the create arguments of a multiply operator after `channels`"""
    a_zp: int = 121
    a_scale: float = 0.05
    b_zp: int = 0
    b_scale: float = 1.0 / 256.0
    y_zp: int = 133
    y_scale: float = 0.04
    qmin: int = 0
    qmax: int = 255

    def args(self):
        return (self.a_zp, self.a_scale, self.b_zp, self.b_scale, self.y_zp, self.y_scale, self.qmin, self.qmax)

    @property
    def ratio(self) -> np.float32:
        """a_scale * b_scale / product_scale in float32, left to right"""
        return np.float32(np.float32(self.a_scale) * np.float32(self.b_scale)) / np.float32(self.y_scale)


MID = Quant()                                                  # ratio 0.00488: shift 7, the bounded form with the full clamp
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))   # the largest float32 below 1

# (name, quantization, distinct expected bytes the exhaustive input must reach at least). A product of two centred bytes
# is at most 65025 in magnitude, so for a ratio below 0.5 / 65025 = 2^-17 every product rounds to 0 and the expected
# tensor is the clamped zero point everywhere: those sets (the late zero point, 2^-32) can only be held to "equals the
# oracle", and state 1. Their zero points differ from each other and from FILL, so a constant from elsewhere fails.
EXHAUSTIVE = [
    ("shift0", Quant(128, 0.5, 128, 0.5, 128, 0.2501), 2),
    ("mid_full_clamp", MID, 64),
    ("mid_clamp_100_101", Quant(qmin=100, qmax=101), 2),
    ("mid_clamp_0_128", Quant(qmin=0, qmax=128), 64),
    ("late_zero_point", Quant(121, 2.0 ** -12, 7, 2.0 ** -13, 77, 1.0), 1),          # ratio 2^-25 < 2^-23
    ("late_zero_point_clamped", Quant(121, 2.0 ** -12, 7, 2.0 ** -13, 77, 1.0, 80, 90), 1),
    ("smallest_ratio", Quant(3, 2.0 ** -16, 250, 2.0 ** -16, 200, 1.0), 1),          # 2^-32
    ("largest_ratio", Quant(128, BELOW_ONE, 128, 1.0, 128, 1.0), 2),
    ("largest_ratio_clamped", Quant(128, BELOW_ONE, 128, 1.0, 7, 1.0, 5, 250), 2),
    ("half", Quant(100, 1.0, 90, 0.5, 0, 1.0), 2),                                   # 0.5 exactly: the edge of shift 0
    ("just_below_half", Quant(100, float(np.nextafter(np.float32(0.5), np.float32(0.0))), 90, 1.0, 255, 1.0), 2),
    ("zero_points_0", Quant(0, 0.05, 0, 1.0 / 256.0, 0, 0.04), 64),
    ("zero_points_255", Quant(255, 0.05, 255, 1.0 / 256.0, 0, 0.04), 64),           # products >= 0: output zero point 0
    ("zero_points_0_255_255", Quant(0, 0.05, 255, 1.0 / 256.0, 255, 0.04), 64),     # products <= 0: output zero point 255
    ("zero_points_0_255", Quant(0, 0.05, 255, 1.0 / 256.0, 128, 0.04), 64),
    ("zero_points_255_0", Quant(255, 0.05, 0, 1.0 / 256.0, 128, 0.04), 64),
    ("shift_16", Quant(0, 2.0 ** -8, 0, 2.0 ** -9, 128, 0.9), 2),                    # the last shift with more than one value
    ("shift_20", Quant(128, 2.0 ** -10, 128, 2.0 ** -10, 99, 0.9), 1),               # the last shift of the bounded form
    ("shift_21", Quant(128, 2.0 ** -10, 128, 2.0 ** -11, 101, 0.9), 1),              # the first past it: the general form
]


def span(rows: int, stride: int, channels: int) -> int:
    return (rows - 1) * stride + channels if rows else 0


def rows_view(buf: np.ndarray, rows: int, stride: int, channels: int) -> np.ndarray:
    """the [rows][channels] view of a strided tensor (no copy)"""
    return np.lib.stride_tricks.as_strided(buf, shape=(rows, channels), strides=(stride, 1))


def product_rows(q: Quant, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """the oracle on [rows][channels] operands that are already matched row for row"""
    acc = (a.astype(np.int32) - q.a_zp) * (b.astype(np.int32) - q.b_zp)
    return o1.q31_requantize(acc, q.ratio, q.y_zp, q.qmin, q.qmax).reshape(acc.shape)


@dataclass(frozen=True)
class Shape:
    channels: int
    b_rows: int
    per: int                  # a_rows_per_b_row
    a_stride: int = 0         # 0: the channel count
    b_stride: int = 0
    y_stride: int = 0

    @property
    def rows(self):
        return self.b_rows * self.per

    @property
    def strides(self):
        return (self.a_stride or self.channels, self.b_stride or self.channels, self.y_stride or self.channels)


def tensors(name: str, s: Shape):
    """random a and b with DIFFERENT b rows, and the FILL-ed product buffer"""
    rng = np.random.default_rng(_seed(name))
    sa, sb, sy = s.strides
    a = rng.integers(0, 256, size=span(s.rows, sa, s.channels), dtype=np.uint8)
    b = rng.integers(0, 256, size=span(s.b_rows, sb, s.channels), dtype=np.uint8)
    return a, b, np.full(span(s.rows, sy, s.channels), FILL, np.uint8)


def expected(q: Quant, s: Shape, a: np.ndarray, b: np.ndarray, into: np.ndarray) -> np.ndarray:
    """the product buffer after one run: `into` (a copy) with the product rows written, everything between them kept"""
    sa, sb, sy = s.strides
    out = into.copy()
    if s.rows:
        b_rows = rows_view(b, s.b_rows, sb, s.channels)
        matched = np.repeat(b_rows, s.per, axis=0)            # row r of a meets row r // per of b
        rows_view(out, s.rows, sy, s.channels)[...] = product_rows(q, rows_view(a, s.rows, sa, s.channels), matched)
    return out


def kernel_for(s: Shape, *addresses) -> str:
    """hip/q8mul.hip's rule: the widest piece that divides the channel count, the three base addresses and the three
    strides"""
    values = (s.channels,) + s.strides + tuple(addresses)
    for width in (16, 4):
        if all(v % width == 0 for v in values):
            return f"q8_mul_x{width}"
    return "q8_mul_x1"


def setup_status(lib, op, s: Shape, a, b, y):
    sa, sb, sy = s.strides
    return lib.setup_multiply_nc_q8_status(op, s.b_rows, s.per, a, sa, b, sb, y, sy)


# ---- hardswish and hardsigmoid ------------------------------------------------------------------------------------
def _h(izp: int, iscale: float):
    f = np.float32
    x = f(iscale) * (np.arange(256, dtype=np.int32) - izp).astype(np.float32)
    return x, np.minimum(np.maximum(x + f(3.0), f(0.0)), f(6.0))


def hardswish_table(izp, iscale, ozp, oscale, qmin, qmax) -> np.ndarray:
    f = np.float32
    x, h = _h(izp, iscale)
    y = (f(1.0) / f(oscale)) * ((x * h) / f(6.0)) + f(ozp)
    assert y.dtype == np.float32
    return np.rint(np.minimum(np.maximum(y, f(qmin)), f(qmax))).astype(np.uint8)


def hardsigmoid_table(izp, iscale, ozp, oscale, qmin, qmax) -> np.ndarray:
    f = np.float32
    _, h = _h(izp, iscale)
    y = f(256.0) * (h / f(6.0))
    assert y.dtype == np.float32
    return np.rint(np.minimum(np.maximum(y, f(qmin)), f(qmax))).astype(np.uint8)
