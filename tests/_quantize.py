"""Cases and drivers for the product's quantize and dequantize operators (include/qnnpack_gfx950_float.h,
qnnp_gfx950_*_quantize_* / qnnp_gfx950_*_dequantize_*).

No reference operator exists, and the definition is bit-exact float32 with every operation rounded once, so the
expectations are its numpy restatement below (tests/test_quantize_host.py pins it to torch's CPU quantizer where the two
definitions agree). Float tensors are compared as uint32 bit patterns; every output buffer starts filled with FILL bytes
(0xA5A5A5A5 as a float pattern), and what lies between strided rows or pixels must come back unchanged.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

FILL = 0xA5
F32 = np.float32
SCALE_MIN, SCALE_MAX = 2.0 ** -118, 2.0 ** 118


def _seed(name: str) -> int:
    return 0x0F32 ^ (zlib.crc32(name.encode()) & 0x7FFFFFFF)


@dataclass(frozen=True)
class Quant:
    """(zero point, scale, min, max): the create arguments of quantize after `channels`; dequantize takes the first two"""
    zp: int = 114
    scale: float = 0.0186
    qmin: int = 0
    qmax: int = 255

    def args(self):
        return (self.zp, self.scale, self.qmin, self.qmax)


MID = Quant()
# the parameter sets of the value tests: a mid scale, 1/256 from 0, zero point 255, a narrow range, the two scale bounds
SETS = [("mid", MID), ("unit_interval", Quant(0, 1.0 / 256)), ("zero_point_255", Quant(255, 0.5)),
        ("narrow", Quant(100, 0.05, 90, 110)), ("smallest_scale", Quant(128, SCALE_MIN)),
        ("largest_scale", Quant(7, SCALE_MAX, 1, 254))]


# ---- the definition ---------------------------------------------------------------------------------------------
def quantize(x: np.ndarray, q: Quant) -> np.ndarray:
    """inv = 1 / scale; t = x * inv; NaN -> 0; clamp to [min - zp, max - zp]; rint (ties to even) + zp"""
    with np.errstate(all="ignore"):
        inv = F32(1.0) / F32(q.scale)
        t = x.astype(F32, copy=False) * inv
        assert t.dtype == np.float32
        t = np.where(np.isnan(t), F32(0.0), t)
        t = np.minimum(np.maximum(t, F32(q.qmin - q.zp)), F32(q.qmax - q.zp))
        return (np.rint(t).astype(np.int32) + q.zp).astype(np.uint8)


def dequantize(y: np.ndarray, q: Quant) -> np.ndarray:
    """(float) (x - zp) * scale: one float32 multiply"""
    out = (y.astype(np.int32) - q.zp).astype(F32) * F32(q.scale)
    assert out.dtype == np.float32
    return out


def bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x).view(np.uint32)


def value_inputs(q: Quant) -> np.ndarray:
    """every bucket centre, every tie with its two float neighbours, the special values, 65 536 random bit patterns"""
    s = F32(q.scale)
    with np.errstate(all="ignore"):
        centres = (np.arange(256, dtype=np.int32) - q.zp).astype(F32) * s
        ties = (np.arange(-256, 256, dtype=np.int32).astype(F32) + F32(0.5)) * s
    ties = np.concatenate([ties, np.nextafter(ties, F32(np.inf)), np.nextafter(ties, F32(-np.inf))])
    fmax = np.finfo(np.float32).max
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.1754942e-38, np.inf, -np.inf, fmax, -fmax, 1e30,
                        -1e30, 1.0, -1.0], F32)
    nans = np.array([0x7FC00000, 0x7F800001, 0xFFC00000, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA5A5A5],
                    np.uint32).view(F32)
    random = np.random.default_rng(_seed(f"values/{q}")).integers(0, 2 ** 32, size=65536, dtype=np.uint64)
    return np.concatenate([centres, ties, special, nans, random.astype(np.uint32).view(F32)]).astype(F32)


# ---- rows -------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Rows:
    channels: int
    batch: int
    f_stride: int = 0         # float side, in elements; 0: the channel count
    q_stride: int = 0         # byte side, in bytes; 0: the channel count

    @property
    def strides(self):
        return (self.f_stride or self.channels, self.q_stride or self.channels)

    @property
    def f_elements(self):
        return (self.batch - 1) * self.strides[0] + self.channels

    @property
    def q_bytes(self):
        return (self.batch - 1) * self.strides[1] + self.channels


def rows_view(buf: np.ndarray, rows: int, stride: int, channels: int) -> np.ndarray:
    """the [rows][channels] view of a strided tensor (no copy); the stride is in elements of buf"""
    return np.lib.stride_tricks.as_strided(buf, shape=(rows, channels), strides=(stride * buf.itemsize, buf.itemsize))


def fill_f32(n: int) -> np.ndarray:
    return np.full(n, 0xA5A5A5A5, np.uint32).view(F32)


def float_inputs(name: str, n: int, q: Quant) -> np.ndarray:
    """n floats that spread over the whole byte range and beyond both ends, with ties and specials mixed in"""
    rng = np.random.default_rng(_seed(name))
    x = ((rng.random(n, dtype=np.float32) * F32(300.0) - F32(22.0 + q.zp)) * F32(q.scale)).astype(F32)
    k = rng.integers(-256, 256, size=n).astype(F32)
    pick = rng.integers(0, 8, size=n)
    x = np.where(pick == 0, (k + F32(0.5)) * F32(q.scale), x).astype(F32)
    x = np.where(pick == 1, np.array([np.nan, np.inf, -np.inf, -0.0], F32)[rng.integers(0, 4, size=n)], x)
    return x.astype(F32)


def quantize_rows_expected(q: Quant, s: Rows, x: np.ndarray, into: np.ndarray) -> np.ndarray:
    fs, qs = s.strides
    out = into.copy()
    rows_view(out, s.batch, qs, s.channels)[...] = quantize(rows_view(x, s.batch, fs, s.channels), q)
    return out


def dequantize_rows_expected(q: Quant, s: Rows, y: np.ndarray, into: np.ndarray) -> np.ndarray:
    fs, qs = s.strides
    out = into.copy()
    rows_view(out, s.batch, fs, s.channels)[...] = dequantize(rows_view(y, s.batch, qs, s.channels), q)
    return out


def kernel_for(direction: str, s: Rows, f_address: int, q_address: int) -> str:
    """hip/f32q8.hip's rule. Rows dense on both sides, or a single row, are one row. Then the widest piece of 16, 4, 1
    for which the byte base -- and, with more than one row, the byte stride -- is a multiple of it; 16 also needs the
    float base on 16 bytes and, with more than one row, the float stride on 4 elements. The channel count does not enter."""
    assert direction in ("quantize", "dequantize")
    fs, qs = s.strides
    many = s.batch > 1 and not (fs == s.channels and qs == s.channels)
    if q_address % 16 == 0 and f_address % 16 == 0 and (not many or (qs % 16 == 0 and fs % 4 == 0)):
        width = 16
    elif q_address % 4 == 0 and (not many or qs % 4 == 0):
        width = 4
    else:
        width = 1
    return f"f32q8_{direction}_x{width}"


# ---- planar -----------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Planar:
    channels: int
    pixels: int
    batch: int
    extra: int = 0            # bytes between pixels beyond the channel count

    @property
    def stride(self):
        return self.channels + self.extra

    @property
    def f_elements(self):
        return self.batch * self.channels * self.pixels

    @property
    def q_bytes(self):
        return (self.batch * self.pixels - 1) * self.stride + self.channels


def quantize_planar_expected(q: Quant, s: Planar, x: np.ndarray, into: np.ndarray) -> np.ndarray:
    """x: dense [batch][channels][pixels] floats -> bytes [batch * pixels][stride]"""
    out = into.copy()
    nhwc = quantize(x.reshape(s.batch, s.channels, s.pixels), q).transpose(0, 2, 1).reshape(s.batch * s.pixels, s.channels)
    rows_view(out, s.batch * s.pixels, s.stride, s.channels)[...] = nhwc
    return out


def dequantize_planar_expected(q: Quant, s: Planar, y: np.ndarray) -> np.ndarray:
    """bytes [batch * pixels][stride] -> dense [batch][channels][pixels] floats, flat"""
    nhwc = dequantize(rows_view(y, s.batch * s.pixels, s.stride, s.channels), q).reshape(s.batch, s.pixels, s.channels)
    return np.ascontiguousarray(nhwc.transpose(0, 2, 1)).reshape(-1)
