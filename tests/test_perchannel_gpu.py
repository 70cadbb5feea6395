"""GPU tier of the per-channel convolution and fully connected operators (include/qnnpack_gfx950_perchannel.h): every
case bit-exact against the oracle applied channel by channel (tests/_perchannel.py), guard bytes between strided pixels
and around the tensors included, inputs unchanged. The shapes are the smallest at which each kernel can still go wrong."""
import functools

import numpy as np
import pytest

import _perchannel as pc
from _gpu import from_device, to_device
from _runner import assert_bytes_equal
from oracle import o1
from qnnpack_amd import QnnpackError, Status

pytestmark = pytest.mark.gpu

ROWS = 129      # a second persistent row tile of the 128-row kernels; the runs at 1 and 31 rows take a prefix


@functools.lru_cache(maxsize=None)
def fc(k, n, in_stride=None, omin=0, omax=255):
    return pc.fc_problem(f"pc_fc_k{k}_n{n}_s{in_stride}_{omin}_{omax}", ROWS, k, n, in_stride, omin=omin, omax=omax).check()


@functools.lru_cache(maxsize=None)
def conv(name, batch, size, kernel=(1, 1), pad=(0, 0, 0, 0), stride=(1, 1), dilation=(1, 1), groups=1, gic=1, goc=1,
         in_stride=None, omin=0, omax=255):
    return pc.conv_problem("pc_" + name, batch, size, kernel, pad, stride, dilation, groups, gic, goc, in_stride,
                           omin=omin, omax=omax).check()


def tile_name(n, c3=False):
    n_pad = (n + 31) // 32 * 32
    return "q8_igemm_pc_mfma_" + ("128x32" if n_pad <= 32 else "128x64" if n_pad <= 64 else "128x128") + ("_c3" if c3 else "")


# ---- fully connected and 1x1: q8_igemm_pc_* ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 33, 72, 132])
@pytest.mark.parametrize("k", [1, 63, 64, 130])
def test_fully_connected_every_tile_width_and_k(qnnp, k, n):
    """output channels: every tile width, a partial channel block, a second n tile; K: one byte, below / at / above a
    K step. Rows 1, 31, 129. Dense rows at offset 0 (store_mode 2 where n % 16 == 0) and strided rows at odd offsets."""
    p = fc(k, n)
    for rows in (1, 31, ROWS):
        assert pc.run_placed(qnnp, p, n, rows=rows) == tile_name(n)
    assert pc.run_placed(qnnp, p, n + 3, 1, 1) == tile_name(n)


@pytest.mark.parametrize("n,out_stride,out_offset", [
    (32, 32, 0), (32, 48, 16), (32, 48, 4), (32, 36, 4), (32, 33, 1), (72, 72, 0), (72, 76, 4), (72, 80, 16), (72, 80, 1),
    (132, 132, 0), (132, 132, 16), (132, 136, 4), (132, 133, 1), (48, 64, 0), (160, 160, 16)])
def test_fully_connected_every_store_mode(qnnp, n, out_stride, out_offset):
    """store_mode 2 (LDS-staged 16-byte stores: n % 16 == 0, stride % 16 == 0, base % 16 == 0), 1 (dword stores) and 0
    (bytes), by channel count, output stride and base offset"""
    p = fc(64, n)
    for rows in (31, ROWS):
        assert pc.run_placed(qnnp, p, out_stride, 0, out_offset, rows=rows) == tile_name(n)


@pytest.mark.parametrize("k,in_stride,in_offset", [(64, 64, 0), (64, 64, 16), (72, 72, 8), (72, 80, 0), (68, 68, 4),
                                                    (68, 72, 12), (63, 63, 0), (64, 64, 1), (64, 65, 0), (130, 130, 2)])
def test_fully_connected_every_activation_load_width(qnnp, k, in_stride, in_offset):
    """16 / 8 / 4 / 1-byte activation loads, picked from K, the input stride and the input's base address"""
    p = fc(k, 40, in_stride)
    assert pc.run_placed(qnnp, p, 40, in_offset, 0) == tile_name(40)
    assert pc.run_placed(qnnp, p, 41, in_offset, 1, rows=31) == tile_name(40)


def test_pointwise_convolution_with_a_clamp(qnnp):
    p = conv("1x1_c24_n40", 2, (9, 9), gic=24, goc=40, omin=10, omax=240)
    assert pc.run_placed(qnnp, p, 40) == tile_name(40)
    assert pc.run_placed(qnnp, p, 44, 0, 4) == tile_name(40)


# ---- grouped: the channel index crosses groups, g * n is no multiple of 4 ---------------------------------------------
@pytest.mark.parametrize("kernel,pad", [((1, 1), (0, 0, 0, 0)), ((3, 3), (1, 1, 1, 1))])
@pytest.mark.parametrize("groups,gic,goc", [(2, 5, 5), (3, 8, 20)])
def test_grouped(qnnp, groups, gic, goc, kernel, pad):
    p = conv(f"grouped_{groups}x{gic}x{goc}_{kernel[0]}", 2, (9, 9), kernel, pad, groups=groups, gic=gic, goc=goc)
    n = groups * goc
    assert pc.run_placed(qnnp, p, n) == tile_name(goc)
    assert pc.run_placed(qnnp, p, n + 4, 0, 0) == tile_name(goc)
    assert pc.run_placed(qnnp, p, n + 1, 1, 3) == tile_name(goc)


# ---- KxK: batch 2, 9x9 pixels, 8 -> 16 and 3 -> 24 (the _c3 slot mode) ------------------------------------------------
@pytest.mark.parametrize("kernel,pad,stride,dilation", [
    ((3, 3), (1, 1, 1, 1), (1, 1), (1, 1)), ((3, 3), (1, 1, 1, 1), (2, 2), (1, 1)),
    ((5, 5), (4, 4, 4, 4), (1, 1), (2, 2)), ((1, 7), (0, 3, 0, 3), (1, 1), (1, 1))])
@pytest.mark.parametrize("gic,goc", [(8, 16), (3, 24)])
def test_kxk(qnnp, gic, goc, kernel, pad, stride, dilation):
    p = conv(f"k{kernel[0]}x{kernel[1]}_s{stride[0]}_d{dilation[0]}_{gic}_{goc}", 2, (9, 9), kernel, pad, stride, dilation,
             gic=gic, goc=goc)
    want = tile_name(goc, c3=gic == 3)
    assert pc.run_placed(qnnp, p, goc) == want            # 16: staged stores; 24: dword stores
    assert pc.run_placed(qnnp, p, goc + 16, 0, 16) == want
    assert pc.run_placed(qnnp, p, goc + 5, 3, 1) == want  # byte stores, odd input base


# ---- depthwise: q8_dwconv_pc_* ----------------------------------------------------------------------------------------
DW_WINDOWS = [("3x3s1", (3, 3), (1, 1, 1, 1), (1, 1), (1, 1), "q8_dwconv_pc_w3s1"),
              ("3x3s2", (3, 3), (1, 1, 1, 1), (2, 2), (1, 1), "q8_dwconv_pc_w3s2"),
              ("5x5", (5, 5), (2, 2, 2, 2), (1, 1), (1, 1), "q8_dwconv_pc_w5s1"),
              ("5x5s2", (5, 5), (2, 2, 2, 2), (2, 2), (1, 1), "q8_dwconv_pc_w5s2"),
              ("3x3d2", (3, 3), (2, 2, 2, 2), (1, 1), (2, 2), "q8_dwconv_pc_any"),
              ("3x1", (3, 1), (1, 0, 1, 0), (1, 1), (1, 1), "q8_dwconv_pc_any")]


@pytest.mark.parametrize("window", DW_WINDOWS, ids=[w[0] for w in DW_WINDOWS])
@pytest.mark.parametrize("channels", [1, 4, 6, 20, 64])
def test_depthwise(qnnp, channels, window):
    """7x7 and 10x13 images (a row longer than one thread's walk of four pixels, and one that is no multiple of it), batch 2;
    dense pixels, and an output stride above C at odd base offsets on both sides. One channel is one group of one input and
    one output channel, which the library takes as a dense convolution (depthwise begins at two groups): it runs on the
    GEMM flavour."""
    tag, kernel, pad, stride, dilation, want = window
    if channels == 1:
        want = tile_name(1)
    for size in ((7, 7), (10, 13)):
        p = conv(f"dw_{tag}_c{channels}_{size[1]}", 2, size, kernel, pad, stride, dilation, groups=channels)
        assert pc.run_placed(qnnp, p, channels) == want
        assert pc.run_placed(qnnp, p, channels + 3, 1, 3) == want
    p = conv(f"dw_{tag}_c{channels}_strided", 2, (7, 7), kernel, pad, stride, dilation, groups=channels,
             in_stride=channels + 5, omin=3, omax=250)
    assert pc.run_placed(qnnp, p, channels + 2, 5, 2) == want


# ---- corner scales ----------------------------------------------------------------------------------------------------
CORNER_BIASES = np.array([-2 ** 31, -2 ** 31 + 1, -2 ** 30, -1, 0, 1, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1], np.int64).astype(np.int32)
# scale_c with input and output scale 1: shift 0 (smallest and largest mantissa), shift 1, shift 31 (2^-32, and its largest mantissa)
CORNER_SCALES = np.array([0.5, 1.0 - 2.0 ** -24, 0.25, 0.25 * (2 - 2.0 ** -23), 2.0 ** -32, 2.0 ** -32 * (2 - 2.0 ** -23),
                          2.0 ** -17 * 1.5, 0.75, 2.0 ** -31], np.float32)


def corner_problem(kind, ozp, omin, omax):
    """K = 1 and the input at its zero point: the accumulator IS the bias. One channel per (bias, scale) pair.
    Condition (i) of tests/_perchannel.py is waived here: these accumulators saturate by design."""
    biases = np.repeat(CORNER_BIASES, CORNER_SCALES.size)
    scales = np.tile(CORNER_SCALES, CORNER_BIASES.size)
    n = biases.size
    izp, kzp = 77, 128
    rows = 5
    if kind == "fc":
        inp = np.full(rows, izp, np.uint8)
        kernel = np.arange(n, dtype=np.uint8).reshape(n, 1)
        acc = o1.gemm_acc(inp.reshape(rows, 1), kernel, biases, izp, kzp)
        return pc.Problem(f"pc_corner_fc_{ozp}", "fc", inp, kernel, biases, scales, acc, 1.0, 1.0, izp, kzp, ozp, omin, omax, 1)
    inp = np.full(rows * n, izp, np.uint8)
    kernel = np.arange(n, dtype=np.uint8).reshape(n, 1, 1, 1, 1)
    shape = o1.conv_shape(1, 1, rows, (0, 0, 0, 0), (1, 1), (1, 1), (1, 1), n, 1, 1, n)
    acc = o1.conv2d_acc(shape, inp, kernel, biases, izp, kzp).reshape(-1, n)
    return pc.Problem(f"pc_corner_dw_{ozp}", "conv", inp, kernel, biases, scales, acc, 1.0, 1.0, izp, kzp, ozp, omin, omax, n,
                      1, (1, rows), groups=n, out_hw=(1, rows))


@pytest.mark.parametrize("ozp,omin,omax", [(0, 0, 255), (128, 1, 254), (255, 0, 255), (128, 128, 128)])
@pytest.mark.parametrize("kind", ["fc", "dw"])
def test_corner_scales_and_accumulators(qnnp, kind, ozp, omin, omax):
    p = corner_problem(kind, ozp, omin, omax)
    assert np.array_equal(p.acc[0], p.bias)
    name = pc.run_placed(qnnp, p, p.channels)
    assert name == ("q8_igemm_pc_mfma_128x128" if kind == "fc" else "q8_dwconv_pc_any")
    pc.run_placed(qnnp, p, p.channels + 1, 0, 1)


# ---- uniform scales: the per-tensor operator's bytes ------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fc", "conv3x3", "dw3x3"])
def test_uniform_scales_equal_the_per_tensor_operator(qnnp, which):
    if which == "fc":
        p, stride = fc(64, 72), 72
    elif which == "conv3x3":
        p, stride = conv("k3x3_s1_d1_8_16", 2, (9, 9), (3, 3), (1, 1, 1, 1), gic=8, goc=16), 16
    else:
        p, stride = conv("dw_3x3s1_c20_13", 2, (10, 13), (3, 3), (1, 1, 1, 1), groups=20), 20
    s = np.float32(2.0 ** -8 * 1.375)
    uniform = np.full(p.channels, s, np.float32)
    expected = p.expected(stride, kernel_scales=uniform)
    outs = []
    for op in (p.create(qnnp, kernel_scales=uniform), p.create(qnnp, per_tensor_scale=s)):
        try:
            d_in, d_out = to_device(p.inp), to_device(np.full(expected.size, pc.FILL, np.uint8))
            p.setup(qnnp, op, d_in, d_out, stride)
            qnnp.run_operator(op)
            outs.append((from_device(d_out), qnnp.operator_kernel(op)))
        finally:
            qnnp.delete_operator(op)
    assert "_pc_" in outs[0][1] and "_pc_" not in outs[1][1], (outs[0][1], outs[1][1])
    assert_bytes_equal(outs[0][0], outs[1][0], f"{which}: per-channel with equal scales against the per-tensor operator")
    assert_bytes_equal(outs[0][0], expected, f"{which}: against the oracle")


# ---- refusals and reuse -----------------------------------------------------------------------------------------------
def test_fused_block_and_residual_attach_are_refused(qnnp):
    c = 16
    dw = conv("dw_3x3s1_c16_fused", 1, (8, 8), (3, 3), (1, 1, 1, 1), groups=c)
    pw = conv("1x1_c16_n16_fused", 1, (8, 8), gic=c, goc=c)
    s = float(np.float32(2.0 ** -9))
    ops = {"dw_pc": dw.create(qnnp), "pw_pc": pw.create(qnnp), "dw": dw.create(qnnp, per_tensor_scale=s),
           "pw": pw.create(qnnp, per_tensor_scale=s)}
    add = qnnp.create_add_nc_q8(c, 120, 0.5, 120, 0.5, 120, 1.0, 0, 255)
    try:
        for expand, depthwise, project in ((None, "dw_pc", "pw"), (None, "dw", "pw_pc"), ("pw_pc", "dw", "pw")):
            st, handle = qnnp.create_fused_block_status(ops[expand] if expand else None, ops[depthwise], ops[project])
            assert st == Status.unsupported_parameter and not handle, (expand, depthwise, project, st)
        st, handle = qnnp.create_fused_block_status(None, ops["dw"], ops["pw"])
        assert st == Status.success
        qnnp.delete_operator(handle)
        d_in = to_device(pw.inp)
        d_out, d_res = to_device(np.zeros(64 * c, np.uint8)), to_device(np.zeros(64 * c, np.uint8))
        qnnp.setup_convolution2d_nhwc_q8(ops["pw_pc"], 1, 8, 8, d_in, c, d_out, c)
        assert qnnp.attach_residual_add_status(ops["pw_pc"], add, d_res, c) == Status.unsupported_parameter
        qnnp.run_operator(ops["pw_pc"])                  # and the operator runs on, without an add
        assert qnnp.operator_residual_folded(ops["pw_pc"]) == -1
        assert_bytes_equal(from_device(d_out), pw.expected(c), "per-channel 1x1 after a refused attach")
        qnnp.setup_convolution2d_nhwc_q8(ops["pw"], 1, 8, 8, d_in, c, d_out, c)
        assert qnnp.attach_residual_add_status(ops["pw"], add, d_res, c) == Status.success
    finally:
        for op in list(ops.values()) + [add]:
            qnnp.delete_operator(op)


def test_forced_kernels_are_refused_at_run(qnnp):
    p = fc(64, 72)
    dw = conv("dw_3x3s1_c20_13", 2, (10, 13), (3, 3), (1, 1, 1, 1), groups=20)
    try:
        for code in (1, 0):
            qnnp.set_option("gemm_kernel", code)
            assert pc.run_placed(qnnp, p, 72) == "q8_igemm_pc_mfma_128x128"
        for code in (2, 5, 6, 9, 20, 23, 24, 29, 31):
            qnnp.set_option("gemm_kernel", code)
            with pytest.raises(QnnpackError) as e:
                pc.run_placed(qnnp, p, 72)               # (placed_run: a refused run writes nothing)
            assert e.value.status == Status.unsupported_parameter, code
        qnnp.set_option("gemm_kernel", 0)
        for code in (1, 2, 3, 4, 6, 8, 9):
            qnnp.set_option("dwconv_kernel", code)
            with pytest.raises(QnnpackError) as e:
                pc.run_placed(qnnp, dw, 20)
            assert e.value.status == Status.unsupported_parameter, code
        qnnp.set_option("dwconv_kernel", 0)
        assert pc.run_placed(qnnp, dw, 20) == "q8_dwconv_pc_w3s1"
    finally:
        qnnp.set_option("gemm_kernel", 0)
        qnnp.set_option("dwconv_kernel", 0)


def test_second_setup_and_host_pointers(qnnp):
    p = fc(63, 33)
    op = p.create(qnnp)
    try:
        pc.run_placed(qnnp, p, 33, rows=ROWS, op=op)
        pc.run_placed(qnnp, p, 40, 1, 4, rows=31, op=op)       # a second setup at another shape
        out = np.full(30 * 37 + 33, pc.FILL, np.uint8)          # host pointers: staged through the device
        qnnp.setup_fully_connected_nc_q8(op, 31, p.input_prefix(31), p.in_stride, out, 37)
        qnnp.run_operator(op)
        assert_bytes_equal(out, p.expected(37, 31), "per-channel fully connected, host pointers")
    finally:
        qnnp.delete_operator(op)
    dw = conv("dw_3x3s2_c6_13", 2, (10, 13), (3, 3), (1, 1, 1, 1), (2, 2), groups=6)
    op = dw.create(qnnp)
    try:
        out = np.full(dw.expected(9).size, pc.FILL, np.uint8)
        dw.setup(qnnp, op, dw.inp, out, 9)
        qnnp.run_operator(op)
        assert_bytes_equal(out, dw.expected(9), "per-channel depthwise, host pointers")
    finally:
        qnnp.delete_operator(op)


def test_one_graph_from_float_to_float(qnnp):
    """quantize -> per-channel conv -> per-channel depthwise -> per-channel FC -> dequantize in ONE hipGraph, replayed
    twice; each stage's bytes are the oracle's on the bytes of the stage before"""
    c1, c2, hw = 8, 16, 6
    rng = np.random.default_rng(7)
    x = rng.normal(0.0, 40.0, (hw * hw, c1)).astype(np.float32)
    q_scale, q_zp = np.float32(0.75), 127
    x_q = np.clip(np.rint(x * (np.float32(1) / q_scale)).astype(np.int64) + q_zp, 0, 255).astype(np.uint8)
    stage1 = pc.conv_problem("pc_graph_3x3", 1, (hw, hw), (3, 3), (1, 1, 1, 1), gic=c1, goc=c2)
    stage1.inp = x_q.reshape(-1)
    shape1 = o1.conv_shape(1, hw, hw, (1, 1, 1, 1), (3, 3), (1, 1), (1, 1), 1, c1, c2, c1)
    stage1.acc = o1.conv2d_acc(shape1, stage1.inp, stage1.kernel, stage1.bias, stage1.izp, stage1.kzp).reshape(-1, c2)
    y1 = stage1.expected(c2)
    stage2 = pc.conv_problem("pc_graph_dw", 1, (hw, hw), (3, 3), (1, 1, 1, 1), groups=c2)
    stage2.inp = y1
    shape2 = o1.conv_shape(1, hw, hw, (1, 1, 1, 1), (3, 3), (1, 1), (1, 1), c2, 1, 1, c2)
    stage2.acc = o1.conv2d_acc(shape2, y1, stage2.kernel, stage2.bias, stage2.izp, stage2.kzp).reshape(-1, c2)
    y2 = stage2.expected(c2)
    stage3 = pc.fc_problem("pc_graph_fc", hw * hw, c2, 10)
    stage3.inp = y2
    stage3.acc = o1.gemm_acc(y2.reshape(hw * hw, c2), stage3.kernel, stage3.bias, stage3.izp, stage3.kzp)
    y3 = stage3.expected(10)
    want = (y3.astype(np.int32) - stage3.ozp).astype(np.float32) * np.float32(stage3.output_scale)

    import torch
    d_x = torch.from_numpy(x.copy()).cuda()
    d_q, d1, d2, d3 = (to_device(np.zeros(n, np.uint8)) for n in (x_q.size, y1.size, y2.size, y3.size))
    d_y = torch.zeros(hw * hw * 10, dtype=torch.float32, device="cuda")
    quant = qnnp.create_quantize_nc_f32_q8(c1, q_zp, float(q_scale), 0, 255)
    dequant = qnnp.create_dequantize_nc_q8_f32(10, stage3.ozp, float(stage3.output_scale))
    ops = [quant, stage1.create(qnnp), stage2.create(qnnp), stage3.create(qnnp), dequant]
    graph = None
    try:
        qnnp.setup_quantize_nc_f32_q8(quant, hw * hw, d_x, c1, d_q, c1)
        stage1.setup(qnnp, ops[1], d_q, d1, c2)
        stage2.setup(qnnp, ops[2], d1, d2, c2)
        stage3.setup(qnnp, ops[3], d2, d3, 10)
        qnnp.setup_dequantize_nc_q8_f32(dequant, hw * hw, d3, 10, d_y, 10)
        qnnp.graph_begin()
        for op in ops:
            qnnp.run_operator(op)
        graph = qnnp.graph_end()
        for _ in range(2):
            d_y.zero_()
            qnnp.graph_launch(graph)
            qnnp.graph_synchronize(graph)
            assert_bytes_equal(from_device(d_q), x_q.reshape(-1), "graph: quantize")
            assert_bytes_equal(from_device(d1), y1, "graph: per-channel 3x3")
            assert_bytes_equal(from_device(d2), y2, "graph: per-channel depthwise")
            assert_bytes_equal(from_device(d3), y3, "graph: per-channel fully connected")
            assert np.array_equal(d_y.cpu().numpy().view(np.uint32), want.reshape(-1).view(np.uint32))
        names = [qnnp.operator_kernel(op) for op in ops[1:4]]
        assert names == ["q8_igemm_pc_mfma_128x32", "q8_dwconv_pc_w3s1", "q8_igemm_pc_mfma_128x32"], names
    finally:
        if graph is not None:
            qnnp.graph_destroy(graph)
        for op in ops:
            qnnp.delete_operator(op)
