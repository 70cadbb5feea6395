"""Worst-case operands for the convolution, GEMM, depthwise and deconvolution kernels (numpy only, no GPU).

The seeded generators of _cases.py draw uniform bytes: a dot product of length K then stays near sqrt(K) * 5000, far from
the bound  max|bias| + 65025 * K < 2^b  from which create time picks the requantization sequence (requantization.h:
qnnp_accumulator_bits). The builders here put real products at that bound.

Corner = (input zero point, kernel zero point) in {0, 255} x {0, 255, 127, 128}. The extreme activation byte is
255 - izp (a - izp = +-255), the extreme weight byte 255 for kzp in {0, 127} and 0 for kzp in {255, 128}
(w - kzp = 255, 128, -255, -128): a product of two extremes is P = +-65025 at the outer kernel zero points and
+-255 * 128 at the centred ones, with all four signs.

Densities, from the cycle (1, 1, 7/8, 1/2, 1/8, 0): output channel n has that share of its weights extreme and the rest
at kzp; fully-connected row m / every band of four image rows has that share of its activations extreme and the rest at
izp (1 = every element, a fraction is drawn per element; bands of eight rows under 7-row windows, see band_rows).
Row 0 / the first two bands and channel 0 have density 1, so whole extreme windows meet whole extreme channels.

Regimes:
  "A30" / "A31"  at the bound: density-1 channels get bias = sign(P) * (B - 1 - 65025 * K), B = 2^30 / 2^30 + 1, the
                 others +-10000 (depthwise: see _build_depthwise). The operator is classified b = 30 / b = 31, and at the outer corners max|acc| = B - 1.
                 Both share input and kernel; only the bias differs.
  "B"            cancelling: in density-1 channels the last input channel of the group has weight kzp in every tap but
                 the centre one (tap ((kh - 1) / 2, (kw - 1) / 2)), which is kzp +- 1; that input channel holds uniform
                 random bytes; bias = -(K - taps) * P + r -+ 127, r in +-60. Where a full window meets a full channel the
                 accumulator is r plus one centred byte, while bias2, the row term and the dot product are as large as
                 they get. Depthwise (one input channel per group): all taps stay extreme, the activations deviate
                 from the extreme by 0 or 1 on the lattice (y % kh == 0, x % kw == 0) -- one pixel per window at most --
                 and bias = -taps * P + r. Deconvolution: only 4x4 stride 2 padding 1, where an interior output sees
                 four taps: bias = -4 * (gic - 1) * P + r -+ 127.
  "E"            regime A's operands with every bias in +-10000: the reduction length alone decides the class.

SCALES are requantization scales; RUNS pairs them with the zero points and clamps of each regime."""
from __future__ import annotations

import collections
import dataclasses
import functools
import os

import numpy as np

from _cases import ConvCase, DeconvCase, FcCase, seed_for, strided_view
from _runner import FILL
from oracle import o1

CORNERS = [(izp, kzp) for izp in (0, 255) for kzp in (0, 255, 127, 128)]
OUTER_CORNERS = [c for c in CORNERS if c[1] in (0, 255)]
DENSITIES = (1.0, 1.0, 7 / 8, 1 / 2, 1 / 8, 0.0)
BOUNDS = {"A30": 2 ** 30, "A31": 2 ** 30 + 1}

# (nominal requantization scale, shift). The second-to-last is not in the issue's list: 1.5 * 2^-20 has shift 19, and
# the last shift that takes the bounded sequences (requant_math.h: 1 <= shift <= 20) is 1.5 * 2^-21.
SCALES = [(float.fromhex("0x1.FFFFFEp-1"), 0),     # the single largest multiplier: the zero point is not folded
          (0.3, 1), (0.006, 7),                    # packed tail, both ends
          (0.05, 4),
          (0.0031, 8),                             # first shift on the 32-bit lane tail
          (1.5 * 2.0 ** -20, 19),
          (1.5 * 2.0 ** -21, 20),                  # last bounded shift
          (1.5 * 2.0 ** -22, 21)]                  # general sequence
SCALE_AT_BOUND = 5                                  # index of 1.5 * 2^-20: regime A's non-vacuity scale

Run = collections.namedtuple("Run", "index kernel_scale output_scale scale zero_point qmin qmax")
Operands = collections.namedtuple("Operands", "case input kernel bias acc out_hw product")


def corner_values(corner):
    """(extreme activation byte, extreme weight byte, P)"""
    izp, kzp = corner
    a_ext = 255 - izp
    w_ext = 255 if kzp in (0, 127) else 0
    return a_ext, w_ext, (a_ext - izp) * (w_ext - kzp)


def reduction_length(case) -> int:
    if isinstance(case, FcCase):
        return case.input_channels
    return case.kernel_size[0] * case.kernel_size[1] * case.gic


def is_depthwise(case) -> bool:
    return isinstance(case, ConvCase) and not isinstance(case, DeconvCase) and case.groups > 1 and case.gic == 1 and case.goc == 1


def has_regime(case, regime: str) -> bool:
    if regime in BOUNDS and 65025 * reduction_length(case) >= 2 ** 30:
        return False
    if regime == "B" and isinstance(case, DeconvCase):
        return case.kernel_size == (4, 4) and case.subsampling == (2, 2) and case.padding == (1, 1, 1, 1) and case.dilation == (1, 1)
    return True


def regimes(case):
    return [r for r in ("A30", "A31", "B") if has_regime(case, r)]


@functools.lru_cache(maxsize=None)
def scale_arguments(index: int):
    """(kernel scale, output scale, float32 requantization scale the operator derives from them) for SCALES[index]. The
    runners pass input and kernel scales 1.0 and the requantization scale is 1 / output scale; the largest multiplier is
    no float32 reciprocal (1 / (1 + 2^-23) rounds one step lower), so it is passed as the kernel scale against output
    scale 1.0, as tests/test_gpu_requant_corners.py does."""
    nominal, shift = SCALES[index]
    out = np.float32(1.0) / np.float32(nominal)
    scale = np.float32(np.float32(1.0) * np.float32(1.0) / out)
    if index == 0 and scale != np.float32(nominal):
        out, scale, kernel_scale = np.float32(1.0), np.float32(nominal), float(np.float32(nominal))
    else:
        kernel_scale = 1.0
    assert o1.q31_params(scale, 0, 0, 255).shift == shift, (nominal, shift)
    return kernel_scale, float(out), scale


def runs(regime: str, product: int):
    """Regime B: zero point 127. Regimes A and E: 0 for positive P, 255 for negative P, and one scale (0.0031) again at
    the opposite zero point. Clamp [0, 255]; every third scale [1, 254], so that the v_med3 path runs too."""
    out = []
    for i in range(len(SCALES)):
        ks, osc, scale = scale_arguments(i)
        qmin, qmax = (1, 254) if i % 3 == 0 else (0, 255)
        if regime == "B":
            out.append(Run(i, ks, osc, scale, 127, qmin, qmax))
            continue
        zp = 0 if product > 0 else 255
        out.append(Run(i, ks, osc, scale, zp, qmin, qmax))
        if i == 4:
            out.append(Run(i, ks, osc, scale, 255 - zp, qmin, qmax))
    return out


def _density(index):
    return np.asarray(DENSITIES)[np.asarray(index) % len(DENSITIES)]


def _extreme_where(rng, density, shape, extreme, rest):
    """`extreme` with probability `density` (broadcast over `shape`; 1 = always, 0 = never), else `rest`"""
    pick = rng.random(shape) < density
    return np.where(pick, np.uint8(extreme), np.uint8(rest)).astype(np.uint8)


def _small_bias(rng, n):
    return rng.integers(-10000, 10001, size=n).astype(np.int64)


def _strided(dense: np.ndarray, stride: int, rng) -> np.ndarray:
    """[rows, channels] -> the flat strided buffer of conv_tensors / fc_tensors (gaps hold random bytes)"""
    rows, ch = dense.shape
    if stride == ch:
        return np.ascontiguousarray(dense).reshape(-1)
    flat = rng.integers(0, 256, size=(rows - 1) * stride + ch, dtype=np.uint8)
    for r in range(rows):
        flat[r * stride:r * stride + ch] = dense[r]
    return flat


def _bias_at_bound(regime, rng, full, product, k):
    bias = _small_bias(rng, full.size)
    if regime in BOUNDS:
        bias[full] = (1 if product > 0 else -1) * (BOUNDS[regime] - 1 - 65025 * k)
    return bias


def _build_fc(case: FcCase, corner, regime, rng):
    izp, kzp = corner
    a_ext, w_ext, P = corner_values(corner)
    M, K, N = case.batch, case.input_channels, case.output_channels
    a = _extreme_where(rng, _density(np.arange(M))[:, None], (M, K), a_ext, izp)
    w = _extreme_where(rng, _density(np.arange(N))[:, None], (N, K), w_ext, kzp)
    full = _density(np.arange(N)) == 1.0
    if regime == "B":
        e = 1 if w_ext == 255 else -1
        a[:, K - 1] = rng.integers(0, 256, size=M, dtype=np.uint8)
        w[full, K - 1] = kzp + e
        bias = _small_bias(rng, N)
        bias[full] = -(K - 1) * P + rng.integers(-60, 61, size=int(full.sum())) - e * (1 if izp == 0 else -1) * 127
    else:
        bias = _bias_at_bound(regime, rng, full, P, K)
    return _strided(a, case.in_stride, rng), w, bias


def band_rows(case) -> int:
    """Bands of four image rows; eight under windows taller than five rows: the two density-1 bands hold a 7-row window
    at one output row in twelve at stride 2, and regime B's share inside the clamp fell to 4.5 % (c3_7x7_s2 at 0.3)."""
    return 8 if case.kernel_size[0] > 5 else 4


def _image(case, corner, rng, all_rows=False):
    """[batch, H, W, channels] activations: bands of four rows take their density from the cycle (all_rows: density 1)"""
    a_ext = corner_values(corner)[0]
    H, W = case.input_size
    ch = case.groups * case.gic
    dens = _density(np.zeros(H, int) if all_rows else np.arange(H) // band_rows(case))[None, :, None, None]
    return _extreme_where(rng, dens, (case.batch, H, W, ch), a_ext, corner[0])


def _build_conv(case, corner, regime, rng):
    """dense, grouped and transposed convolutions; kernel [g][oc][kh][kw][ic], or [g][ic][kh][kw][oc] for a deconvolution"""
    izp, kzp = corner
    a_ext, w_ext, P = corner_values(corner)
    kh, kw = case.kernel_size
    G, gic, goc = case.groups, case.gic, case.goc
    deconv = isinstance(case, DeconvCase)
    x = _image(case, corner, rng)
    chan = np.arange(G * goc).reshape(G, goc)
    wd = _density(chan)[:, :, None, None, None]
    w = _extreme_where(rng, wd, (G, goc, kh, kw, gic), w_ext, kzp)
    full = (_density(chan) == 1.0)
    K = kh * kw * gic
    if regime == "B":
        e = 1 if w_ext == 255 else -1
        last = np.arange(G) * gic + gic - 1
        x[..., last] = rng.integers(0, 256, size=x.shape[:3] + (G,), dtype=np.uint8)
        tail = np.full((kh, kw), kzp, np.uint8)
        tail[(kh - 1) // 2, (kw - 1) // 2] = kzp + e
        w[full, :, :, gic - 1] = tail
        seen = 4 * gic if deconv else K                      # products an interior output sums
        taps = 4 if deconv else kh * kw                      # of them, those of the last input channel
        bias = _small_bias(rng, G * goc)
        bias[full.reshape(-1)] = (-(seen - taps) * P + rng.integers(-60, 61, size=int(full.sum()))
                                  - e * (1 if izp == 0 else -1) * 127)
    else:
        bias = _bias_at_bound(regime, rng, full.reshape(-1), P, K)
    if deconv:
        w = np.ascontiguousarray(w.transpose(0, 4, 2, 3, 1))
    return _strided(x.reshape(-1, G * gic), case.in_stride, rng), w, bias


def depthwise_lattice(case, rng, x, corner, all_rows=False):
    """regime B of a depthwise case: on the lattice (y % kh == 0, x % kw == 0) of the density-1 bands the activation
    moves 0 or 1 off the extreme, towards the zero point: one deviating pixel per window at most"""
    kh, kw = case.kernel_size
    H, W = case.input_size
    ys = np.array([y for y in range(0, H, kh) if all_rows or DENSITIES[(y // band_rows(case)) % len(DENSITIES)] == 1.0])
    xs = np.arange(0, W, kw)
    delta = rng.integers(0, 2, size=(x.shape[0], ys.size, xs.size, x.shape[3])).astype(np.int16)
    step = -1 if corner[0] == 0 else 1
    sub = x[:, ys[:, None], xs[None, :], :].astype(np.int16) + step * delta
    x[:, ys[:, None], xs[None, :], :] = sub.astype(np.uint8)


def _build_depthwise(case, corner, regime, rng, weight_values=None):
    """weight_values: the byte every tap of channel c holds is weight_values[c] (the weight-range classes); else densities"""
    izp, kzp = corner
    a_ext, w_ext, P = corner_values(corner)
    kh, kw = case.kernel_size
    C = case.groups
    x = _image(case, corner, rng, all_rows=weight_values is not None)
    if weight_values is None:
        w = _extreme_where(rng, _density(np.arange(C))[:, None, None, None, None], (C, 1, kh, kw, 1), w_ext, kzp)
        full = _density(np.arange(C)) == 1.0
        products = np.full(C, P, np.int64)
    else:
        w = np.broadcast_to(np.asarray(weight_values, np.uint8)[:, None, None, None, None], (C, 1, kh, kw, 1)).copy()
        full = np.ones(C, bool)
        products = (a_ext - izp) * (np.asarray(weight_values, np.int64) - kzp)
    if regime == "B":
        depthwise_lattice(case, rng, x, corner, all_rows=weight_values is not None)
        bias = _small_bias(rng, C)
        bias[full] = -kh * kw * products[full] + rng.integers(-60, 61, size=int(full.sum()))
    else:
        bias = _bias_at_bound(regime, rng, full, P, kh * kw)
        if regime in BOUNDS:
            # A depthwise window has 9 or 25 products: off the bound channels |acc| <= 10000 + taps * |P| is below half a
            # step of the scale 1.5 * 2^-20 (3x3 at the centred corners: 303760 * 1.43e-6 = 0.43) and every byte would sit
            # on the zero point. The channels of density 7/8 and 1/8 therefore take a bias spread over sign(P) * [0, 2^27):
            # below the bound channels' (the class stays), inside the clamp at that scale.
            spread = np.isin(_density(np.arange(C)), (7 / 8, 1 / 8))
            bias[spread] = (1 if P > 0 else -1) * rng.integers(0, 2 ** 27, size=int(spread.sum()))
    return _strided(x.reshape(-1, C), case.in_stride, rng), w, bias


def _threads():
    return max(1, min(16, os.cpu_count() or 1))


def accumulators(case, inp, kernel, bias):
    """([rows, channels] int32 oracle accumulators, output height and width or None); `case` carries the zero points"""
    o1.set_threads(_threads())
    try:
        if isinstance(case, FcCase):
            a = strided_view(inp, case.batch, case.input_channels, case.in_stride)
            return o1.gemm_acc(a, kernel, bias, case.izp, case.kzp), None
        H, W = case.input_size
        shape = o1.conv_shape(case.batch, H, W, case.padding, case.kernel_size, case.subsampling, case.dilation,
                              case.groups, case.gic, case.goc, case.in_stride)
        if isinstance(case, DeconvCase):
            acc, hw = o1.deconv2d_acc(shape, case.adjustment, inp, kernel, bias, case.izp, case.kzp), o1.deconv_output_hw(shape, case.adjustment)
        else:
            acc, hw = o1.conv2d_acc(shape, inp, kernel, bias, case.izp, case.kzp), o1.conv_output_hw(shape)
        return acc.reshape(-1, case.groups * case.goc), hw
    finally:
        o1.set_threads(1)


def _finish(case, corner, inp, kernel, bias):
    assert np.abs(bias).max() < 2 ** 31
    bias = bias.astype(np.int32)
    case = dataclasses.replace(case, izp=corner[0], kzp=corner[1], qmin=0, qmax=255)
    acc, hw = accumulators(case, inp, kernel, bias)
    for arr in (inp, kernel, bias, acc):
        arr.setflags(write=False)
    return Operands(case, inp, kernel, bias, acc, hw, corner_values(corner)[2])


@functools.lru_cache(maxsize=48)
def operands(case, corner, regime) -> Operands:
    """Operands of `case` at `corner` in `regime` with the oracle's accumulators: one oracle pass for every forced code,
    scale, zero point and clamp. The case returned carries the corner's zero points. Read-only: shared between tests."""
    assert has_regime(case, regime), (case.name, regime)
    rng = np.random.default_rng(seed_for(f"{case.name}/{corner[0]}/{corner[1]}/{regime[0]}"))
    if isinstance(case, FcCase):
        build = _build_fc
    else:
        build = _build_depthwise if is_depthwise(case) else _build_conv
    inp, kernel, bias = build(case, corner, regime, rng)
    if regime == "A31":       # the same draws as "A30": share its tensors, only the bias differs
        base = operands(case, corner, "A30")
        assert np.array_equal(inp, base.input) and np.array_equal(kernel, base.kernel)
        inp, kernel = base.input, base.kernel
    return _finish(case, corner, inp, kernel, bias)


# the bytes whose distance from kzp is one of -255, -128, -127, 127, 128, 255, by kernel zero point
WEIGHT_RANGE_BYTES = {0: (127, 128, 255), 255: (0, 127, 128), 127: (0, 254, 255), 128: (0, 1, 255)}


@functools.lru_cache(maxsize=16)
def weight_range_operands(case, corner) -> Operands:
    """depthwise, every tap of a channel at one of the three reachable ends of the weight-range classes (blocks of eight
    channels take them in turn), every activation at the extreme but for regime B's lattice, regime B's bias"""
    rng = np.random.default_rng(seed_for(f"{case.name}/{corner[0]}/{corner[1]}/W"))
    values = np.asarray(WEIGHT_RANGE_BYTES[corner[1]])[(np.arange(case.groups) // 8) % 3]
    return _finish(case, corner, *_build_depthwise(case, corner, "B", rng, weight_values=values))


def _dense_bytes(ops: Operands, run: Run) -> np.ndarray:
    return o1.requantize_rows(ops.acc, run.scale, run.zero_point, run.qmin, run.qmax)


def expected_bytes(ops: Operands, run: Run, dense=None) -> np.ndarray:
    """the oracle's output buffer (flat, strided, gaps FILL) for one run"""
    dense = _dense_bytes(ops, run) if dense is None else dense
    rows, cout = dense.shape
    stride = ops.case.out_stride
    if stride == cout:
        return dense.reshape(-1)
    out = np.full((rows - 1) * stride + cout, FILL, np.uint8)
    np.lib.stride_tricks.as_strided(out, shape=(rows, cout), strides=(stride, 1))[:] = dense
    return out


def inside_share(ops: Operands, run: Run, dense=None):
    """(share, count) of the oracle's bytes strictly inside (0, 255)"""
    dense = _dense_bytes(ops, run) if dense is None else dense
    inside = (dense > 0) & (dense < 255)
    return float(inside.mean()), int(inside.sum())


def assert_not_vacuous(ops: Operands, regime: str, run: Run, dense=None):
    """The conditions on the reference alone (measured shares: tests/test_worstcase_host.py). Regime B at zero point
    127: dense, pointwise and fully-connected >= 5 % at every scale; depthwise >= 3 % at scales <= 0.05 and >= 8 bytes
    at the two larger ones. Regime A at 1.5 * 2^-20 with the sign-matched zero point: >= 10 %."""
    share, count = inside_share(ops, run, dense)
    what = f"{ops.case.name} izp {ops.case.izp} kzp {ops.case.kzp} regime {regime} scale {float(run.scale):.3e}: {share:.4f} ({count} bytes) inside the clamp"
    if regime == "B" and run.zero_point == 127:
        if not is_depthwise(ops.case):
            assert share >= 0.05, what
        elif float(run.scale) <= 0.0501:
            assert share >= 0.03, what
        else:
            assert count >= 8, what
    if regime in BOUNDS and run.index == SCALE_AT_BOUND and run.zero_point == (0 if ops.product > 0 else 255):
        assert share >= 0.10, what
    return share, count


def reference(ops: Operands, regime: str, run: Run) -> np.ndarray:
    """expected_bytes after assert_not_vacuous, from one requantization pass"""
    dense = _dense_bytes(ops, run)
    assert_not_vacuous(ops, regime, run, dense)
    return expected_bytes(ops, run, dense)
