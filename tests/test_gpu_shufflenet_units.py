"""GPU tier: one ShuffleNet v1 unit and one ShuffleNet v2 unit through the C ABI, on device buffers, run operator by
operator and then captured as ONE hipGraph and replayed. Every intermediate tensor is checked against a chain of oracle
(O1: convolution accumulators, requantization, add) and numpy (channel shuffle, clamp) results, as
tests/test_gpu_network.py does for MobileNetV2. Quantization parameters come from the oracle's accumulators layer by
layer (tests/_cases.py output_quantization), so every tensor spans its 0..255 range.

 * v1, groups 2, stride 1, 28 x 28, 200 channels: grouped 1x1 (g2, 100 -> 25) -> channel shuffle (2, 25) -> depthwise
   3x3 (50) -> grouped 1x1 (g2, 25 -> 100) -> add with the unit input -> clamp (ReLU at the sum's zero point).
 * v2 x1.0, stride 1, 28 x 28, 116 channels, no copies: buffer A holds [x1 | x2] at pixel stride 116. The first 1x1
   reads A + 58 at stride 116; the depthwise 3x3 and the second 1x1 follow, and the second 1x1 writes back into A + 58
   at stride 116 (x2 has been consumed by then); the channel shuffle (2, 58) reads A and writes the unit output.
"""
import numpy as np
import pytest
import torch

import _x8 as x8
from _cases import output_quantization
from _gpu import from_device, to_device
from oracle import o1

pytestmark = pytest.mark.gpu

BATCH, H, W = 2, 28, 28
KZP = 127


def _oracle_conv(rng, x, izp, k, groups, gic, goc, in_stride=None):
    """(kernel, bias, output bytes, output scale, output zero point) of a stride-1 'same' convolution"""
    kernel = rng.integers(0, 256, size=(groups * goc, k, k, gic), dtype=np.uint8)
    bias = rng.integers(-2000, 2000, size=groups * goc, dtype=np.int32)
    pad = k // 2
    shape = o1.conv_shape(BATCH, H, W, (pad,) * 4, (k, k), (1, 1), (1, 1), groups, gic, goc, input_pixel_stride=in_stride)
    acc = o1.conv2d_acc(shape, x, kernel, bias, izp, KZP)
    oscale, ozp = output_quantization(acc)
    out = o1.requantize_rows(acc.reshape(-1, groups * goc), np.float32(1.0) / oscale, ozp, 0, 255).reshape(-1)
    return kernel, bias, out, float(oscale), ozp


def _conv_op(qnnp, k, groups, gic, goc, izp, conv):
    kernel, bias, _, oscale, ozp = conv
    pad = k // 2
    return qnnp.create_convolution2d_nhwc_q8(pad, pad, pad, pad, k, k, 1, 1, 1, 1, groups, gic, goc, izp, 1.0, KZP, 1.0,
                                             kernel, bias, ozp, oscale, 0, 255, 0)


class Unit:
    """operators in launch order and the (name, device buffer, expected bytes) of every tensor they write"""

    def __init__(self, qnnp):
        self.qnnp, self.ops, self.checks = qnnp, [], []

    def run(self):
        for op in self.ops:
            self.qnnp.run_operator(op)

    def verify(self, what):
        torch.cuda.synchronize()
        for name, buf, want in self.checks:
            got = from_device(buf)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"{what}: {name} ({bad.size} of {got.size} bytes differ, first at {bad[:4]})"

    def replay_graph(self, reset):
        """capture the unit as one hipGraph; replay it twice, each time after wiping every written tensor and
        restoring the input with reset()"""
        self.qnnp.graph_begin()
        try:
            self.run()
        finally:
            graph = self.qnnp.graph_end()
        try:
            for _ in range(2):
                for _name, buf, _want in self.checks:
                    buf.fill_(x8.FILL)
                reset()
                torch.cuda.synchronize()
                self.qnnp.graph_launch(graph)
                self.qnnp.graph_synchronize(graph)
                self.verify("graph replay")
        finally:
            self.qnnp.graph_destroy(graph)

    def close(self):
        for op in self.ops:
            self.qnnp.delete_operator(op)


def test_shufflenet_v1_g2_unit(qnnp):
    rng = np.random.default_rng(0x51F1)
    c, g, mid = 200, 2, 50
    x = rng.integers(0, 256, size=BATCH * H * W * c, dtype=np.uint8)
    xzp = 127
    conv1 = _oracle_conv(rng, x, xzp, 1, g, c // g, mid // g)                      # grouped 1x1 200 -> 50
    t1, zp1 = conv1[2], conv1[4]
    t2 = x8.channel_shuffle(t1, BATCH * H * W, g, mid // g).reshape(-1)             # channel shuffle (2, 25)
    conv3 = _oracle_conv(rng, t2, zp1, 3, mid, 1, 1)                                # depthwise 3x3
    t3, zp3 = conv3[2], conv3[4]
    conv4 = _oracle_conv(rng, t3, zp3, 1, g, mid // g, c // g)                      # grouped 1x1 50 -> 200
    t4, zp4 = conv4[2], conv4[4]
    t5 = np.empty_like(x)
    o1.add_q8(BATCH * H * W, c, xzp, 1.0, zp4, 1.0, 128, 2.0, 0, 255, x, c, t4, c, t5, c)
    t6 = np.maximum(t5, np.uint8(128))                                              # clamp [128, 255]

    unit = Unit(qnnp)
    d_x = to_device(x)
    d = [to_device(np.zeros(t.size, np.uint8)) for t in (t1, t2, t3, t4, t5, t6)]
    try:
        unit.ops.append(_conv_op(qnnp, 1, g, c // g, mid // g, xzp, conv1))
        qnnp.setup_convolution2d_nhwc_q8(unit.ops[-1], BATCH, H, W, d_x, c, d[0], mid)
        unit.ops.append(qnnp.create_channel_shuffle_nc_x8(g, mid // g))
        qnnp.setup_channel_shuffle_nc_x8(unit.ops[-1], BATCH * H * W, d[0], mid, d[1], mid)
        unit.ops.append(_conv_op(qnnp, 3, mid, 1, 1, zp1, conv3))
        qnnp.setup_convolution2d_nhwc_q8(unit.ops[-1], BATCH, H, W, d[1], mid, d[2], mid)
        unit.ops.append(_conv_op(qnnp, 1, g, mid // g, c // g, zp3, conv4))
        qnnp.setup_convolution2d_nhwc_q8(unit.ops[-1], BATCH, H, W, d[2], mid, d[3], c)
        unit.ops.append(qnnp.create_add_nc_q8(c, xzp, 1.0, zp4, 1.0, 128, 2.0, 0, 255))
        qnnp.setup_add_nc_q8(unit.ops[-1], BATCH * H * W, d_x, c, d[3], c, d[4], c)
        unit.ops.append(qnnp.create_clamp_nc_u8(c, 128, 255))
        qnnp.setup_clamp_nc_u8(unit.ops[-1], BATCH * H * W, d[4], c, d[5], c)
        names = ("grouped 1x1", "channel shuffle", "depthwise 3x3", "grouped 1x1 (2)", "add", "clamp")
        unit.checks = list(zip(names, d, (t1, t2, t3, t4, t5, t6)))
        unit.run()
        unit.verify("operator by operator")
        assert qnnp.operator_kernel(unit.ops[1]) == "x8_shuffle_lds"
        assert qnnp.operator_kernel(unit.ops[5]) == "u8_clamp_flat_x16"
        unit.replay_graph(lambda: None)
    finally:
        unit.close()


def test_shufflenet_v2_unit_without_copies(qnnp):
    rng = np.random.default_rng(0x51F2)
    c, b = 116, 58
    a = rng.integers(0, 256, size=BATCH * H * W * c, dtype=np.uint8)               # [x1 | x2], pixel stride 116
    azp = 127
    conv1 = _oracle_conv(rng, a[b:], azp, 1, 1, b, b, in_stride=c)                  # 1x1 on x2 = A + 58, stride 116
    t1, zp1 = conv1[2], conv1[4]
    conv2 = _oracle_conv(rng, t1, zp1, 3, b, 1, 1)                                  # depthwise 3x3
    t2, zp2 = conv2[2], conv2[4]
    conv3 = _oracle_conv(rng, t2, zp2, 1, 1, b, b)                                  # 1x1, written back over x2
    a_after = a.copy().reshape(-1, c)
    a_after[:, b:] = conv3[2].reshape(-1, b)
    a_after = a_after.reshape(-1)
    out = x8.channel_shuffle(a_after, BATCH * H * W, 2, b).reshape(-1)              # channel shuffle (2, 58)
    assert np.array_equal(out.reshape(-1, c)[:, 0::2], a.reshape(-1, c)[:, :b])     # x1 passes through

    unit = Unit(qnnp)
    d_a = to_device(a)
    a_saved = d_a.clone()
    d_t1, d_t2 = to_device(np.zeros(t1.size, np.uint8)), to_device(np.zeros(t2.size, np.uint8))
    d_out = to_device(np.zeros(out.size, np.uint8))
    x2 = d_a.data_ptr() + b
    try:
        unit.ops.append(_conv_op(qnnp, 1, 1, b, b, azp, conv1))
        qnnp.setup_convolution2d_nhwc_q8(unit.ops[-1], BATCH, H, W, x2, c, d_t1, b)
        unit.ops.append(_conv_op(qnnp, 3, b, 1, 1, zp1, conv2))
        qnnp.setup_convolution2d_nhwc_q8(unit.ops[-1], BATCH, H, W, d_t1, b, d_t2, b)
        unit.ops.append(_conv_op(qnnp, 1, 1, b, b, zp2, conv3))
        qnnp.setup_convolution2d_nhwc_q8(unit.ops[-1], BATCH, H, W, d_t2, b, x2, c)
        unit.ops.append(qnnp.create_channel_shuffle_nc_x8(2, b))
        qnnp.setup_channel_shuffle_nc_x8(unit.ops[-1], BATCH * H * W, d_a, c, d_out, c)
        unit.checks = [("1x1 on x2", d_t1, t1), ("depthwise 3x3", d_t2, t2), ("A after the 1x1 wrote x2", d_a, a_after),
                       ("channel shuffle", d_out, out)]
        unit.run()
        unit.verify("operator by operator")
        assert qnnp.operator_kernel(unit.ops[3]) == "x8_shuffle_lds"
        unit.replay_graph(lambda: d_a.copy_(a_saved))      # the unit overwrites x2: each replay starts from the input
    finally:
        unit.close()
