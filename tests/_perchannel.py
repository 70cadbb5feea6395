"""Per-channel weight scales (include/qnnpack_gfx950_perchannel.h): problems, their expected bytes and the runs.

Expected bytes: o1.conv2d_acc / o1.gemm_acc, then PER CHANNEL o1.q31_requantize(acc[..., c],
f32(f32(input_scale) * f32(kernel_scales[c])) / f32(output_scale), zero point, min, max).

Scales: adjacent channels differ in exponent AND mantissa (channel_scales). Before any GPU run `Problem.check` asserts two
conditions on the ORACLE's output -- conditions on the inputs, not measurements:
  (i)  in every channel at least a quarter of the outputs lie strictly between output_min and output_max;
  (ii) for every channel c, requantizing its accumulators with the scale of channel c +- 1, 4, 8, 16 (where that channel
       exists) changes at least one byte.
They make a transposed lane map or an off-by-one table index fail. A problem is built for its LARGEST row count; the runs
at fewer rows take a prefix of its rows (one row cannot hold either condition), so both are stated on the full problem.
To meet them with scales that span 2^9, a channel's weights are drawn the narrower the larger its scale, and its bias
places the channel's mean output at its own spot of the range, 20 ... 64 steps off the middle.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from _cases import seed_for
from oracle import o1

FILL = 0xA5
f32 = np.float32


def channel_scales(n: int, factor: float = 1.0) -> np.ndarray:
    """ks[c] = 2^-(6 + c % 9) * (1 + ((37 c) % 64) / 64), times `factor`"""
    c = np.arange(n)
    return (f32(factor) * (2.0 ** -(6 + c % 9)) * (1.0 + ((37 * c) % 64) / 64.0)).astype(np.float32)


def requant_scale(input_scale, kernel_scale, output_scale) -> np.float32:
    """scale_c: float32, each operation rounded once, this order"""
    return f32(f32(f32(input_scale) * f32(kernel_scale)) / f32(output_scale))


def requantize_per_channel(acc: np.ndarray, input_scale, kernel_scales, output_scale, ozp, omin, omax) -> np.ndarray:
    """acc [..., C] int32 -> uint8 of the same shape, channel by channel through the oracle"""
    out = np.empty(acc.shape, np.uint8)
    for c in range(acc.shape[-1]):
        out[..., c] = o1.q31_requantize(np.ascontiguousarray(acc[..., c]),
                                        requant_scale(input_scale, kernel_scales[c], output_scale), ozp, omin, omax)
    return out


def check_conditions(acc: np.ndarray, input_scale, kernel_scales, output_scale, ozp, omin, omax, what: str) -> None:
    """conditions (i) and (ii) of the module docstring on acc [rows, C]"""
    rows, channels = acc.shape
    out = requantize_per_channel(acc, input_scale, kernel_scales, output_scale, ozp, omin, omax)
    for c in range(channels):
        inside = np.count_nonzero((out[:, c] > omin) & (out[:, c] < omax))
        assert 4 * inside >= rows, f"{what}: condition (i) fails in channel {c}: {inside} of {rows} outputs inside the range"
        for d in (-16, -8, -4, -1, 1, 4, 8, 16):
            if 0 <= c + d < channels:
                other = o1.q31_requantize(np.ascontiguousarray(acc[:, c]),
                                          requant_scale(input_scale, kernel_scales[c + d], output_scale), ozp, omin, omax)
                assert np.any(other != out[:, c]), f"{what}: condition (ii) fails for channel {c} with the scale of {c + d}"


@dataclass
class Problem:
    """One operator with per-channel scales, its tensors and its accumulators. kind: "fc" or "conv"."""
    name: str
    kind: str
    inp: np.ndarray            # flat strided input
    kernel: np.ndarray
    bias: np.ndarray
    kernel_scales: np.ndarray
    acc: np.ndarray            # [rows, C]
    input_scale: float
    output_scale: float
    izp: int
    kzp: int
    ozp: int
    omin: int
    omax: int
    in_stride: int
    # conv only
    batch: int = 1
    input_size: tuple = (1, 1)
    kernel_size: tuple = (1, 1)
    padding: tuple = (0, 0, 0, 0)
    subsampling: tuple = (1, 1)
    dilation: tuple = (1, 1)
    groups: int = 1
    gic: int = 1
    goc: int = 1
    out_hw: tuple = (1, 1)

    @property
    def channels(self):
        return self.acc.shape[1]

    def check(self):
        check_conditions(self.acc, self.input_scale, self.kernel_scales, self.output_scale, self.ozp, self.omin, self.omax,
                         self.name)
        return self

    def expected(self, out_stride: int, rows: int = None, kernel_scales=None) -> np.ndarray:
        """the flat strided output of the first `rows` rows, FILL between them"""
        rows = self.acc.shape[0] if rows is None else rows
        ks = self.kernel_scales if kernel_scales is None else kernel_scales
        q = requantize_per_channel(self.acc[:rows], self.input_scale, ks, self.output_scale, self.ozp, self.omin, self.omax)
        out = np.full((rows - 1) * out_stride + self.channels, FILL, np.uint8)
        for r in range(rows):
            out[r * out_stride:r * out_stride + self.channels] = q[r]
        return out

    def create(self, lib, kernel_scales=None, per_tensor_scale=None):
        """the per-channel operator, or with per_tensor_scale the per-tensor one with that kernel scale"""
        ks = self.kernel_scales if kernel_scales is None else kernel_scales
        tail = (self.kernel, self.bias, self.ozp, float(self.output_scale), self.omin, self.omax, 0)
        if self.kind == "fc":
            head = (self.kernel.shape[1], self.kernel.shape[0], self.izp, float(self.input_scale), self.kzp)
            if per_tensor_scale is not None:
                return lib.create_fully_connected_nc_q8(*head, float(per_tensor_scale), *tail)
            return lib.create_fully_connected_nc_q8_per_channel(*head, ks, *tail)
        head = (*self.padding, *self.kernel_size, *self.subsampling, *self.dilation, self.groups, self.gic, self.goc,
                self.izp, float(self.input_scale), self.kzp)
        if per_tensor_scale is not None:
            return lib.create_convolution2d_nhwc_q8(*head, float(per_tensor_scale), *tail)
        return lib.create_convolution2d_nhwc_q8_per_channel(*head, ks, *tail)

    def setup(self, lib, op, d_in, d_out, out_stride: int, rows: int = None):
        if self.kind == "fc":
            lib.setup_fully_connected_nc_q8(op, self.acc.shape[0] if rows is None else rows, d_in, self.in_stride, d_out, out_stride)
        else:
            assert rows is None
            lib.setup_convolution2d_nhwc_q8(op, self.batch, self.input_size[0], self.input_size[1], d_in, self.in_stride,
                                            d_out, out_stride)

    def input_prefix(self, rows: int = None) -> np.ndarray:
        if rows is None or self.kind != "fc":
            return self.inp
        return self.inp[:(rows - 1) * self.in_stride + self.kernel.shape[1]]


def _tuned(name, acc_of, kernel_shape, channel_axis, reduction, channels, izp, kzp, ozp, omin, omax, input_scale):
    """Kernel, bias, kernel scales and output scale for which the two conditions can hold: see the module docstring.
    acc_of(kernel, bias) -> [rows, C]."""
    rng = np.random.default_rng(seed_for(name) ^ 0x5CA1E)
    ks = channel_scales(channels)
    # the largest scale_c: a channel of +-1 weights spreads over some tens of output steps, and stays below 1
    s_max = min(0.9, 40.0 / (0.6 * 74.0 * np.sqrt(reduction)))
    output_scale = f32(float(f32(input_scale) * ks.max()) / s_max)
    scale = np.array([requant_scale(input_scale, k, output_scale) for k in ks], np.float64)
    sigma_w = np.clip(30.0 / (scale * 74.0 * np.sqrt(reduction)), 0.6, 73.0)
    shape = [1] * len(kernel_shape)
    shape[channel_axis] = channels
    kernel = np.clip(np.rint(kzp + rng.normal(0.0, 1.0, kernel_shape) * sigma_w.reshape(shape)), 0, 255).astype(np.uint8)
    acc0 = acc_of(kernel, np.zeros(channels, np.int32))
    # the channel's mean output at its own spot of the range, a quarter of the range around the zero point
    # (and not at the zero point itself: a channel of constant accumulators -- K = 1 with a weight at its zero point -- then
    #  still answers the scale of a neighbour, which differs by a fifth or more, with another byte)
    spot = rng.uniform(0.08, 0.25, channels) * rng.choice([-1.0, 1.0], channels) * (omax - omin) + (0.5 * (omin + omax) - ozp)
    bias = np.rint(spot / scale - acc0.reshape(-1, channels).mean(axis=0)).astype(np.int64)
    bias = np.clip(bias, -2 ** 30, 2 ** 30).astype(np.int32)
    return kernel, bias, ks, output_scale


def fc_problem(name, rows, k, n, in_stride=None, izp=127, kzp=128, ozp=120, omin=0, omax=255, input_scale=0.75) -> Problem:
    in_stride = in_stride or k
    rng = np.random.default_rng(seed_for(name))
    inp = rng.integers(0, 256, (rows - 1) * in_stride + k, dtype=np.uint8)
    a = np.lib.stride_tricks.as_strided(inp, shape=(rows, k), strides=(in_stride, 1), writeable=False)
    acc_of = lambda kernel, bias: o1.gemm_acc(a, kernel, bias, izp, kzp)
    kernel, bias, ks, output_scale = _tuned(name, acc_of, (n, k), 0, k, n, izp, kzp, ozp, omin, omax, input_scale)
    return Problem(name, "fc", inp, kernel, bias, ks, acc_of(kernel, bias), input_scale, output_scale, izp, kzp, ozp, omin,
                   omax, in_stride)


def conv_problem(name, batch, input_size, kernel_size=(1, 1), padding=(0, 0, 0, 0), subsampling=(1, 1), dilation=(1, 1),
                 groups=1, gic=1, goc=1, in_stride=None, izp=127, kzp=128, ozp=120, omin=0, omax=255,
                 input_scale=0.75) -> Problem:
    in_stride = in_stride or groups * gic
    rng = np.random.default_rng(seed_for(name))
    H, W = input_size
    inp = rng.integers(0, 256, (batch * H * W - 1) * in_stride + groups * gic, dtype=np.uint8)
    shape = o1.conv_shape(batch, H, W, padding, kernel_size, subsampling, dilation, groups, gic, goc, in_stride)
    out_hw = o1.conv_output_hw(shape)
    channels = groups * goc
    acc_of = lambda kernel, bias: o1.conv2d_acc(shape, inp, kernel, bias, izp, kzp).reshape(-1, channels)
    kshape = (groups, goc, kernel_size[0], kernel_size[1], gic)
    # (the channel axis of the [g][oc] pair: tune on a [channels, ...] view)
    kernel, bias, ks, output_scale = _tuned(
        name, lambda kern, b: acc_of(kern.reshape(kshape), b), (channels, kernel_size[0], kernel_size[1], gic), 0,
        kernel_size[0] * kernel_size[1] * gic, channels, izp, kzp, ozp, omin, omax, input_scale)
    kernel = kernel.reshape(kshape)
    return Problem(name, "conv", inp, kernel, bias, ks, acc_of(kernel, bias), input_scale, output_scale, izp, kzp, ozp, omin,
                   omax, in_stride, batch, input_size, kernel_size, padding, subsampling, dilation, groups, gic, goc, out_hw)


def run_placed(lib, problem: Problem, out_stride: int, in_offset: int = 0, out_offset: int = 0, rows: int = None,
               op=None, expected=None):
    """Create (unless `op` is given), set up and run on guarded device buffers at the given byte offsets; compare the whole
    output buffer -- the bytes between strided pixels included -- with the expected bytes; the guards and the input must
    come back unchanged. Returns the kernel name."""
    from _runner import assert_bytes_equal, placed_run
    expected = problem.expected(out_stride, rows) if expected is None else expected
    out = np.full(expected.size, FILL, np.uint8)
    own = op is None
    if own:
        op = problem.create(lib)
    try:
        got = placed_run(lib, op, problem.input_prefix(rows), out, in_offset, out_offset, problem.name,
                         lambda d_in, d_out: problem.setup(lib, op, d_in, d_out, out_stride, rows))
        name = lib.operator_kernel(op)
    finally:
        if own:
            lib.delete_operator(op)
    assert_bytes_equal(got, expected, f"{problem.name} rows={rows} out_stride={out_stride} offsets=({in_offset}, {out_offset}) [{name}]")
    return name
