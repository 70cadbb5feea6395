"""Cases and drivers for the two byte-streaming operators (add, global average pooling).

Case lists restate the reference's operator tests: test/add.cc (31 tests: batch 1 / 3 / strided, channels
1..91 step 15, qmin / qmax 128, scales 1e-2..1e1, zero points 0..255 step 51; defaults of
test/add-operator-tester.h:251-258) and test/global-average-pooling.cc (34 tests over the SSE2 tile nr = 8,
mr = 7: channels 8..24 x width 1..7 and 7..28, channels 1..7 x width 1..16, strides 5*nr, scales 0.01*pi^k,
zero points step 51, min / max 128; defaults of test/global-average-pooling-operator-tester.h:221-226).
The reference testers compare against a float model with a 0.5-0.6 LSB tolerance; here the scalar oracle
(qnnp_add_quantize / qnnp_avgpool_quantize restated) is the bit-exact expectation.

The oracle restates the integer algorithm, so it cannot notice a defect of the algorithm itself. The second half of
this file holds it to real arithmetic: float64 models of both operators and lists of parameter sets at the edges of
the accepted scale ratios ([2^-14, 2^8) for add, [2^-8, 2^8) for the pooling). Those lists are kept apart from
add_cases() / gap_cases(): these also run against the compiled reference, which is undefined at some of the edges.
tests/test_pointwise_range_host.py checks the oracle against the models, tests/test_pointwise_range_gpu.py the
kernels against the oracle.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import List

import numpy as np

from oracle import o1

FILL = 0xA5


def _seed(name: str) -> int:
    return 0x51A0 ^ (zlib.crc32(name.encode()) & 0x7FFFFFFF)


@dataclass(frozen=True)
class AddCase:
    name: str
    batch: int
    channels: int
    a_stride: int = 0
    b_stride: int = 0
    y_stride: int = 0
    a_scale: float = 0.75
    b_scale: float = 1.25
    y_scale: float = 0.96875
    a_zp: int = 121
    b_zp: int = 127
    y_zp: int = 133
    qmin: int = 0
    qmax: int = 255

    @property
    def strides(self):
        return (self.a_stride or self.channels, self.b_stride or self.channels, self.y_stride or self.channels)


def add_cases() -> List[AddCase]:
    out = [AddCase("a_zero_batch", 0, 2)]
    scales = [1.0e-2, 1.0e-1, 1.0, 1.0e+1]
    for prefix, batch, strides in (("unit", 1, {}), ("small", 3, {}),
                                   ("strided", 3, dict(a_stride=129, b_stride=123, y_stride=117))):
        for ch in range(1, 100, 15):
            base = dict(batch=batch, channels=ch, **strides)
            out.append(AddCase(f"a_{prefix}_c{ch}", **base))
            out.append(AddCase(f"a_{prefix}_c{ch}_qmin", qmin=128, **base))
            out.append(AddCase(f"a_{prefix}_c{ch}_qmax", qmax=128, **base))
            for s in scales:
                out.append(AddCase(f"a_{prefix}_c{ch}_as{s:g}", a_scale=s, **base))
                out.append(AddCase(f"a_{prefix}_c{ch}_bs{s:g}", b_scale=s, **base))
                out.append(AddCase(f"a_{prefix}_c{ch}_ys{s:g}", y_scale=s, **base))
            for zp in range(0, 256, 51):
                out.append(AddCase(f"a_{prefix}_c{ch}_azp{zp}", a_zp=zp, **base))
                out.append(AddCase(f"a_{prefix}_c{ch}_bzp{zp}", b_zp=zp, **base))
                out.append(AddCase(f"a_{prefix}_c{ch}_yzp{zp}", y_zp=zp, **base))
    # beyond the reference's list: the dense 16-byte-vector path, ragged tails, a residual-sized tensor
    out += [
        AddCase("ax_dense_vec16", 4, 64),
        AddCase("ax_dense_c24_b6", 6, 24),                # 144 bytes: 9 vectors
        AddCase("ax_dense_odd_total", 3, 7),
        AddCase("ax_residual_56x56x24", 56 * 56, 24),
        AddCase("ax_residual_strided", 14 * 14, 96, a_stride=128, b_stride=96, y_stride=112),
        AddCase("ax_clamp_tight", 5, 33, qmin=100, qmax=101),
    ]
    return out


def add_tensors(case: AddCase):
    rng = np.random.default_rng(_seed(case.name))
    sa, sb, sy = case.strides
    n = case.batch
    a = rng.integers(0, 256, size=max(n - 1, 0) * sa + case.channels if n else 0, dtype=np.uint8)
    b = rng.integers(0, 256, size=max(n - 1, 0) * sb + case.channels if n else 0, dtype=np.uint8)
    y = np.full(max(n - 1, 0) * sy + case.channels if n else 0, FILL, dtype=np.uint8)
    return a, b, y


def add_expected(case: AddCase, a, b):
    sa, sb, sy = case.strides
    y = np.full(max(case.batch - 1, 0) * sy + case.channels if case.batch else 0, FILL, dtype=np.uint8)
    if case.batch:
        o1.add_q8(case.batch, case.channels, case.a_zp, case.a_scale, case.b_zp, case.b_scale, case.y_zp, case.y_scale,
                  case.qmin, case.qmax, a, sa, b, sb, y, sy)
    return y


def add_run(lib, case: AddCase, a, b, to_device=None, from_device=None):
    sa, sb, sy = case.strides
    y = np.full(max(case.batch - 1, 0) * sy + case.channels if case.batch else 0, FILL, dtype=np.uint8)
    op = lib.create_add_nc_q8(case.channels, case.a_zp, case.a_scale, case.b_zp, case.b_scale,
                              case.y_zp, case.y_scale, case.qmin, case.qmax, 0)
    try:
        if to_device is not None and case.batch:
            d_a, d_b, d_y = to_device(a), to_device(b), to_device(y)
            lib.setup_add_nc_q8(op, case.batch, d_a, sa, d_b, sb, d_y, sy)
            lib.run_operator(op)
            y = from_device(d_y)
        else:
            one = np.zeros(1, np.uint8)
            lib.setup_add_nc_q8(op, case.batch, a if a.size else one, sa, b if b.size else one, sb,
                                y if y.size else one, sy)
            lib.run_operator(op)
        kname = lib.operator_kernel(op) if hasattr(lib, "operator_kernel") else None
    finally:
        lib.delete_operator(op)
    return y, kname


@dataclass(frozen=True)
class GapCase:
    name: str
    batch: int
    width: int
    channels: int
    in_stride: int = 0
    out_stride: int = 0
    in_scale: float = 1.0
    out_scale: float = 1.0
    in_zp: int = 121
    out_zp: int = 133
    qmin: int = 0
    qmax: int = 255

    @property
    def strides(self):
        return (self.in_stride or self.channels, self.out_stride or self.channels)


def gap_cases(full: bool = True) -> List[GapCase]:
    nr, mr = 8, 7
    out = [GapCase("g_zero_batch", 0, 1, 8)]
    pis = []
    s = 0.01
    while s < 100.0:
        pis.append(float(np.float32(s)))
        s *= 3.14159265
    regimes = [("many_small", range(nr, 3 * nr + 1), range(1, mr + 1)),
               ("many_large", range(nr, 3 * nr + 1), range(mr, 4 * mr + 1)),
               ("few", range(1, nr), range(1, 2 * nr + 1))]
    for rname, chans, widths in regimes:
        chans, widths = list(chans), list(widths)
        if not full:
            chans, widths = chans[::3] + chans[-1:], widths[::3] + widths[-1:]
        for ch in chans:
            for w in widths:
                tag = f"g_{rname}_c{ch}_w{w}"
                out.append(GapCase(tag, 1, w, ch))
                out.append(GapCase(tag + "_istride", 1, w, ch, in_stride=5 * nr))
                out.append(GapCase(tag + "_omin", 1, w, ch, qmin=128))
                out.append(GapCase(tag + "_omax", 1, w, ch, qmax=128))
                out.append(GapCase(tag + "_b3", 3, w, ch))
                out.append(GapCase(tag + "_b3_istride", 3, w, ch, in_stride=5 * nr))
                out.append(GapCase(tag + "_b3_ostride", 3, w, ch, out_stride=5 * nr))
                if (ch + w) % 4 == 0 or not full:      # the scale / zero-point sweeps on a quarter of the grid
                    for sc in pis:
                        out.append(GapCase(tag + f"_is{sc:.4g}", 1, w, ch, in_scale=sc))
                        out.append(GapCase(tag + f"_os{sc:.4g}", 1, w, ch, out_scale=sc))
                    for zp in range(0, 256, 51):
                        out.append(GapCase(tag + f"_izp{zp}", 1, w, ch, in_zp=zp))
                        out.append(GapCase(tag + f"_ozp{zp}", 1, w, ch, out_zp=zp))
    # beyond the reference's list: MobileNetV2's own pooling (7x7x1280), the dword path with strides, big widths
    out += [
        GapCase("gx_mobilenetv2_7x7x1280", 4, 49, 1280),
        GapCase("gx_mobilenetv2_strided", 3, 49, 1280, in_stride=1296, out_stride=1284),
        GapCase("gx_c320_w196", 2, 196, 320),
        GapCase("gx_c4_w1000", 2, 1000, 4),
        GapCase("gx_c6_w300_unaligned", 2, 300, 6, in_stride=7),
        GapCase("gx_c1024_w2", 5, 2, 1024),
        GapCase("gx_scale_ratio_low", 2, 9, 16, in_scale=0.004, out_scale=1.0),
        GapCase("gx_scale_ratio_high", 2, 9, 16, in_scale=200.0, out_scale=1.0),
    ]
    return out


def gap_tensors(case: GapCase):
    rng = np.random.default_rng(_seed(case.name))
    si, so = case.strides
    px = case.batch * case.width
    inp = rng.integers(0, 256, size=max(px - 1, 0) * si + case.channels if px else 0, dtype=np.uint8)
    return inp


def _gap_out(case):
    si, so = case.strides
    return np.full(max(case.batch - 1, 0) * so + case.channels if case.batch else 0, FILL, dtype=np.uint8)


def gap_expected(case: GapCase, inp):
    si, so = case.strides
    out = _gap_out(case)
    if case.batch:
        o1.global_average_pooling_q8(case.batch, case.width, case.channels, case.in_zp, case.in_scale, case.out_zp,
                                     case.out_scale, case.qmin, case.qmax, inp, si, out, so)
    return out


def gap_run(lib, case: GapCase, inp, to_device=None, from_device=None):
    si, so = case.strides
    out = _gap_out(case)
    op = lib.create_global_average_pooling_nwc_q8(case.channels, case.in_zp, case.in_scale, case.out_zp, case.out_scale,
                                                  case.qmin, case.qmax, 0)
    try:
        if to_device is not None and case.batch:
            d_in, d_out = to_device(inp), to_device(out)
            lib.setup_global_average_pooling_nwc_q8(op, case.batch, case.width, d_in, si, d_out, so)
            lib.run_operator(op)
            out = from_device(d_out)
        else:
            one = np.zeros(1, np.uint8)
            lib.setup_global_average_pooling_nwc_q8(op, case.batch, case.width, inp if inp.size else one, si,
                                                    out if out.size else one, so)
            lib.run_operator(op)
        kname = lib.operator_kernel(op) if hasattr(lib, "operator_kernel") else None
    finally:
        lib.delete_operator(op)
    return out, kname


# ---- the whole accepted range, held to real arithmetic ---------------------------------------------------------------
def f32(x: float) -> float:
    return float(np.float32(x))


def f32_below(x: float) -> float:
    """the float32 just below x"""
    return float(np.nextafter(np.float32(x), np.float32(0.0)))


# Below this larger ratio the reference's right shift would be 32 ... 35 (21 - exponent): the reference is undefined,
# the product and the oracle answer clamp(sum zero point) (qnnp_compute_add_params, requantization.h of the product).
ADD_SEAM = 2.0 ** -10

# a_scale / sum_scale and b_scale / sum_scale, each in [2^-14, 2^8): both ends, both sides of the seam, and values
# with full mantissas in between and at 1
ADD_RANGE_RATIOS = [f32(v) for v in (
    2.0 ** -14, 1.37 * 2.0 ** -14, f32_below(2.0 ** -10), 2.0 ** -10, 1.5 * 2.0 ** -10, 1.11 * 2.0 ** -7, 1.37 * 2.0 ** -3,
    0.75, 1.0, 1.25, 1.11 * 2.0 ** 3, 1.37 * 2.0 ** 7, f32_below(2.0 ** 8))]
ADD_RANGE_ZERO_POINTS = [(0, 0, 0), (255, 255, 255), (0, 255, 128), (255, 0, 0)]
ADD_RANGE_CLAMPS = [(0, 255), (128, 255), (0, 128), (100, 101)]

# |y - clip(real)| <= ADD_TOL, derived (not measured). With M_a = round(r_a * 2^shift), M_b likewise, the kernel forms
# acc = (a - a_zp) * M_a + (b - b_zp) * M_b exactly (|acc| <= 2 * 255 * 2^22 < 2^31: no wrap) and rounds acc * 2^-shift
# to the nearest integer: 0.5. Each multiplier is off by at most half a unit, |M * 2^-shift - r| <= 2^-(shift + 1), and
# |a - a_zp|, |b - b_zp| <= 255, so acc * 2^-shift is within 2 * 255 * 2^-(shift + 1) = 255 * 2^-shift of the real
# sum; shift = 21 - exponent(larger ratio) >= 14 because the ratios are below 2^8. Clamping moves y and the real value
# towards each other. Below the seam y = clamp(y_zp) and |real - y_zp| <= 2 * 255 * ADD_SEAM < 0.4981.
ADD_TOL = 0.5 + 255 * 2.0 ** -14


@dataclass(frozen=True)
class AddRangeSet:
    name: str
    a_scale: float
    b_scale: float
    y_scale: float = 1.0
    a_zp: int = 121
    b_zp: int = 127
    y_zp: int = 133
    qmin: int = 0
    qmax: int = 255

    @property
    def ratios(self):
        """the two float32 quotients as qnnp_create_add_nc_q8 forms them (add.c)"""
        return (np.float32(self.a_scale) / np.float32(self.y_scale), np.float32(self.b_scale) / np.float32(self.y_scale))

    @property
    def below_seam(self) -> bool:
        return float(max(self.ratios)) < ADD_SEAM

    @property
    def band(self) -> str:
        """by the larger ratio; the GPU tier runs one test id per kernel and band"""
        top = float(max(self.ratios))
        return "below_seam" if top < ADD_SEAM else "low" if top < 0.5 else "mid" if top < 2.0 else "high"


ADD_RANGE_BANDS = ("below_seam", "low", "mid", "high")


def add_range_sets() -> List[AddRangeSet]:
    r = ADD_RANGE_RATIOS
    out = [AddRangeSet(f"r{i}_r{j}", r[i], r[j]) for i in range(len(r)) for j in range(len(r))]
    last = len(r) - 1
    for i, j in [(k, k) for k in range(len(r))] + [(0, last), (last, 0)]:
        for zps in ADD_RANGE_ZERO_POINTS:
            for qmin, qmax in ADD_RANGE_CLAMPS:
                out.append(AddRangeSet(f"r{i}_r{j}_zp{zps[0]}_{zps[1]}_{zps[2]}_q{qmin}_{qmax}", r[i], r[j], 1.0,
                                       zps[0], zps[1], zps[2], qmin, qmax))
    # a sum scale that is no power of two: the ratios are rounded float32 quotients (one third, two thirds, ...)
    out += [
        AddRangeSet("third_two_thirds", 1.0, 2.0, 3.0),
        AddRangeSet("y3_mid", 0.75, 1.25, 3.0),
        AddRangeSet("y3_lowest", 3.0 * 2.0 ** -14, 3.0 * 2.0 ** -14, 3.0),          # both quotients exactly 2^-14
        AddRangeSet("y3_below_seam", 2.9 * 2.0 ** -10, 1.0 * 2.0 ** -12, 3.0),
        AddRangeSet("y3_high_low", 700.0, 3.0 * 2.0 ** -14, 3.0, 0, 255, 128, 0, 255),
    ]
    return out


def add_range_inputs():
    """a[r][c] = r, b[r][c] = c: every (a, b) byte pair once, as [256][256] tensors"""
    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1).copy()
    return a, np.ascontiguousarray(a.T)


def add_real(s: AddRangeSet, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """the sum in real arithmetic (float64), unclamped"""
    ra, rb = (float(v) for v in s.ratios)
    return (a.astype(np.float64) - s.a_zp) * ra + (b.astype(np.float64) - s.b_zp) * rb + s.y_zp


_ADD_RANGE_EXPECTED = {}


def add_range_expected(s: AddRangeSet) -> np.ndarray:
    """the oracle's [256][256] bytes for the inputs of add_range_inputs(); computed once per set, read-only"""
    if s not in _ADD_RANGE_EXPECTED:
        a, b = add_range_inputs()
        y = np.full(65536, FILL, dtype=np.uint8)
        o1.add_q8(256, 256, s.a_zp, s.a_scale, s.b_zp, s.b_scale, s.y_zp, s.y_scale, s.qmin, s.qmax,
                  a.reshape(-1), 256, b.reshape(-1), 256, y, 256)
        y = y.reshape(256, 256)
        y.setflags(write=False)
        _ADD_RANGE_EXPECTED[s] = y
    return _ADD_RANGE_EXPECTED[s]


def worst_distance(y: np.ndarray, real: np.ndarray, qmin: int, qmax: int) -> float:
    """max |y - clip(real, qmin, qmax)| over every output, clamped or not"""
    return float(np.max(np.abs(y.astype(np.float64) - np.clip(real, qmin, qmax))))


# Average pooling, global and windowed: input_scale / output_scale in [2^-8, 2^8)
POOL_RANGE_RATIOS = [f32(v) for v in (2.0 ** -8, 1.37 * 2.0 ** -8, 1.0, 1.11 * 2.0 ** 7, f32_below(2.0 ** 8))]
POOL_RANGE_ZERO_POINTS = [(0, 0), (255, 255), (0, 255), (255, 0), (121, 133)]      # (input, output)
POOL_RANGE_CLAMPS = [(0, 255), (100, 101)]

# |y - clip(real)| <= POOL_TOL, derived (not measured). With N pixels in the divisor and n = sum - N * in_zp
# (|n| <= 255 * N), the kernels round n * s to the nearest integer exactly (64-bit product of n and the 24-bit mantissa
# of s): 0.5. s = fl(in_scale / fl(out_scale * N)) is the float32 that create / setup form: two roundings, so
# |s - ratio / N| <= (ratio / N) * (2^-23 + 2^-48) and n * s is within 255 * ratio * (2^-23 + 2^-48) of the real value,
# which is below 255 * 2^8 * 2^-23 for every float32 ratio below 2^8. The lists here have out_scale = 1, so the ratio
# itself is exact (another output scale would add a third rounding).
POOL_TOL = 0.5 + 255 * 2.0 ** 8 * 2.0 ** -23

GAP_RANGE_WIDTHS = (1, 2, 7, 49, 300)
GAP_RANGE_CHANNELS = 256


def gap_range_cases(channels: int = GAP_RANGE_CHANNELS, in_stride: int = 0) -> List[GapCase]:
    """batch 4 (the four images of gap_range_pixels) x widths x ratios x zero-point corners x clamps"""
    out = []
    for width in GAP_RANGE_WIDTHS:
        for k, ratio in enumerate(POOL_RANGE_RATIOS):
            for in_zp, out_zp in POOL_RANGE_ZERO_POINTS:
                for qmin, qmax in POOL_RANGE_CLAMPS:
                    out.append(GapCase(f"gr_c{channels}_s{in_stride}_w{width}_r{k}_zp{in_zp}_{out_zp}_q{qmin}_{qmax}", 4, width,
                                       channels, in_stride=in_stride, in_scale=ratio, out_scale=1.0, in_zp=in_zp,
                                       out_zp=out_zp, qmin=qmin, qmax=qmax))
    return out


def gap_range_pixels(width: int, channels: int = GAP_RANGE_CHANNELS) -> np.ndarray:
    """[4][width][channels]: channel c holds byte c at every pixel (the mean is exactly c); random; all 0; all 255"""
    rng = np.random.default_rng(_seed(f"gap_range_w{width}"))
    px = np.empty((4, width, GAP_RANGE_CHANNELS), np.uint8)
    px[0] = np.arange(GAP_RANGE_CHANNELS, dtype=np.uint8)[None, :]
    px[1] = rng.integers(0, 256, size=(width, GAP_RANGE_CHANNELS), dtype=np.uint8)
    px[2] = 0
    px[3] = 255
    return np.ascontiguousarray(px[:, :, :channels])


def gap_range_input(case: GapCase, pixels: np.ndarray) -> np.ndarray:
    """`pixels` laid out with the case's input stride (the bytes between pixels are 0x5A)"""
    si, _ = case.strides
    rows = case.batch * case.width
    flat = np.full((rows - 1) * si + case.channels, 0x5A, dtype=np.uint8)
    idx = np.arange(rows, dtype=np.int64)[:, None] * si + np.arange(case.channels)[None, :]
    flat[idx] = pixels.reshape(rows, case.channels)
    return flat


def pool_ratio(in_scale: float, out_scale: float) -> float:
    """the float32 quotient input_scale / output_scale as the creates form it, as a float64"""
    return float(np.float32(in_scale) / np.float32(out_scale))


def gap_real(case: GapCase, pixels: np.ndarray) -> np.ndarray:
    """[batch][channels] in real arithmetic (float64), unclamped: (mean - in_zp) * ratio + out_zp"""
    mean = pixels.astype(np.int64).sum(axis=1) / float(case.width)
    return (mean - case.in_zp) * pool_ratio(case.in_scale, case.out_scale) + case.out_zp
