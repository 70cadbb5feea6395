"""GPU tier of the dynamically quantized fully connected operator with 4-bit weights
(qnnp_gfx950_create_fully_connected_nc_f32_qd8_qc4w: hip/qd8f32gemm4.hip behind dynamic-fully-connected.c). The
expectation is tests/_dynamic_fc.expected on the unpacked nibbles; outputs are compared as uint32 bit patterns inside
guard bytes, and the product kernel's name is asserted per case."""
import numpy as np
import pytest

import _dynamic_fc as dfc
from _gpu import Guarded
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

F32 = np.float32
INF, NAN = float("inf"), float("nan")
FILL = 0xA5A5A5A5


def pack(w, spare=0):
    """w [N][K] in [-8, 7] -> [N][(K + 1) / 2] bytes, weight k in bits 4 (k % 2) .. of byte k / 2; `spare` fills the
    unused high nibble of an odd K"""
    n, k = w.shape
    nibbles = np.full((n, k + k % 2), spare, np.uint8)
    nibbles[:, :k] = w.astype(np.int8).view(np.uint8) & 15
    return nibbles[:, 0::2] | (nibbles[:, 1::2] << 4)


def problem(name, batch, k, n):
    x, kernel, scales, bias = dfc.problem(name, batch, k, n)
    return x, kernel >> 4, scales, bias


def kernel_name(batch):
    return "qd8_f32_qc4w_gemv_mfma_16" if batch <= 16 else "qd8_f32_qc4w_gemm_mfma_128x128"


def run(qnnp, op, x, n, in_extra=0, out_extra=0, in_off=0, out_off=0, what=""):
    """one setup and run on fresh guarded buffers (strides above the channel counts by *_extra elements, bases offset by
    *_off bytes): y [batch][N] as bit patterns, after checking the guards, the gaps and the kernel name"""
    batch, k = x.shape
    in_stride, out_stride = k + in_extra, n + out_extra
    x_host = np.full((batch - 1) * in_stride + k, 7.25, F32)
    y_host = np.full((batch - 1) * out_stride + n, FILL, np.uint32)
    for r in range(batch):
        x_host[r * in_stride:r * in_stride + k] = x[r]
    gx, gy = Guarded(x_host, in_off), Guarded(y_host, out_off)
    assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, gx, in_stride, gy, out_stride) == Status.success, what
    qnnp.run_operator(op)
    assert qnnp.operator_kernel(op) == kernel_name(batch), (what, qnnp.operator_kernel(op))
    got = gy.read().view(np.uint32)
    gy.assert_intact(what)
    gx.assert_intact(what + " (input)")
    y = np.stack([got[r * out_stride:r * out_stride + n] for r in range(batch)])
    gaps = np.delete(got, (np.arange(batch)[:, None] * out_stride + np.arange(n)).ravel())
    assert np.all(gaps == FILL), what + ": a gap between output rows was written"
    return y


def same(got, want, what):
    bad = np.argwhere(got != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} differ, first at {bad[:4].tolist()}"


def check(qnnp, name, x, w, scales, bias, lo=-INF, hi=INF, spare=0, **layout):
    want = dfc.expected(x, w.astype(np.int8), scales, bias, lo, hi)
    op = qnnp.create_fully_connected_nc_f32_qd8_qc4w(x.shape[1], w.shape[0], pack(w, spare), scales, bias, lo, hi)
    try:
        same(run(qnnp, op, x, w.shape[0], what=name, **layout), want, name)
    finally:
        qnnp.delete_operator(op)
    return want


# every batch, K and N with at least two values of the other two: GEMV / tile GEMM and one / two row tiles; odd K, one K
# tile, odd and even K-tile counts through both kernels, the GEMV's pass boundary at 64 tiles
SHAPES = [(1, 1, 1), (17, 1, 16), (16, 63, 16), (129, 63, 33), (1, 64, 130), (129, 64, 33), (17, 65, 130), (1, 65, 1),
          (129, 127, 1), (16, 127, 130), (17, 128, 33), (1, 128, 16), (1, 129, 33), (17, 129, 130), (16, 192, 1),
          (129, 192, 16), (16, 1025, 33), (129, 1025, 130), (16, 4096, 130), (17, 4096, 16), (1, 4160, 16), (17, 4160, 1)]


@pytest.mark.parametrize("batch,k,n", SHAPES)
def test_shape_edges_of_each_kernel(qnnp, batch, k, n):
    name = f"shape4/b{batch}_k{k}_n{n}"
    check(qnnp, name, *problem(name, batch, k, n), spare=15)


@pytest.mark.parametrize("batch", [3, 17])
@pytest.mark.parametrize("pattern", ["all_-8", "all_7", "all_-1", "alternating"])
def test_nibble_classes(qnnp, batch, pattern):
    k, n = 130, 33
    x, _, scales, bias = problem("nibbles", batch, k, n)
    row = {"all_-8": np.full(k, -8), "all_7": np.full(k, 7), "all_-1": np.full(k, -1),
           "alternating": np.where(np.arange(k) % 2 == 0, -8, 7)}[pattern]
    check(qnnp, f"nibbles/{pattern}/b{batch}", x, np.tile(row, (n, 1)), scales, bias)


@pytest.mark.parametrize("batch", [3, 17])
def test_spare_nibble_of_an_odd_k_is_ignored(qnnp, batch):
    name = f"spare/b{batch}"
    for spare in (0, 15):
        check(qnnp, name, *problem(name, batch, 129, 33), spare=spare)


@pytest.mark.parametrize("batch", [1, 17])
@pytest.mark.parametrize("pattern", ["all_high", "both_ends", "all_low"])
def test_accumulator_bound(qnnp, batch, pattern):
    """K = 32768, weights at 7 and -8, activations at the ends of their range: the kernels' 16 * sum reaches 2^29"""
    k, n = 32768, 16
    x = {"all_high": np.ones(k, F32), "all_low": -np.ones(k, F32), "both_ends": np.tile(np.array([0.0, 2.0], F32), k // 2)}[pattern]
    x = np.tile(x, (batch, 1))
    w = np.empty((n, k), np.int64)
    w[0::4], w[1::4] = 7, -8
    w[2::4] = np.where(np.arange(k) % 2 == 1, 7, -8)
    w[3::4] = np.where(np.arange(k) % 2 == 1, -8, 7)
    loop = 16 * np.abs((dfc.quantize_rows(x[:1])[0].astype(np.int64) - 128) @ w.T).max()
    assert loop <= 2 ** 29 and (loop == 2 ** 29 or pattern != "all_low")
    want = check(qnnp, f"bound4/{pattern}/b{batch}", x, w, np.full(n, 2.0 ** -9, F32), np.arange(n, dtype=F32))
    assert np.abs(want).max() > 60


@pytest.mark.parametrize("batch", [3, 17])
def test_strided_rows_and_offset_bases(qnnp, batch):
    name = f"layout4/b{batch}"
    check(qnnp, name, *problem(name, batch, 200, 33), in_extra=1, out_extra=1, in_off=12, out_off=8)


@pytest.mark.parametrize("batch", [3, 17])
def test_clamp_cuts_and_null_bias(qnnp, batch):
    x, w, scales, bias = problem("clamp4", batch, 200, 33)
    want = check(qnnp, f"clamp4/b{batch}", x, w, scales, bias, -0.5, 0.75)
    assert (want == F32(-0.5)).any() and (want == F32(0.75)).any() and ((want > -0.5) & (want < 0.75)).any()
    check(qnnp, f"no bias4/b{batch}", x, w, scales, None)


def test_create_refusals_in_their_order(qnnp):
    k, n = 8, 4
    kernel, scales, bias = np.full((n, k // 2), 0x11, np.uint8), np.full(n, 0.01, F32), np.zeros(n, F32)

    def with_(array, value):
        return np.where(np.arange(len(array)) == 2, array.dtype.type(value), array)
    inv, uns = Status.invalid_parameter, Status.unsupported_parameter
    big = 2 ** 24
    table = [
        ((k, n, kernel, scales, bias, -INF, INF), Status.success),
        ((k, n, None, scales, bias, -INF, INF), inv),
        ((k, n, kernel, with_(scales, 0.0), bias, -INF, INF), inv),
        ((k, n, kernel, with_(scales, 1e-40), bias, -INF, INF), inv),
        ((k, n, kernel, with_(scales, NAN), bias, -INF, INF), inv),
        ((32769, n, kernel, with_(scales, 2.0 ** 21), bias, 1.0, 0.5), inv),          # invalid before unsupported
        ((k, n, kernel, with_(scales, 2.0 ** -21), bias, -INF, INF), uns),
        ((k, n, kernel, with_(scales, float(np.nextafter(F32(2.0 ** 20), F32(INF)))), bias, -INF, INF), uns),
        ((32769, 1, np.zeros((1, 16385), np.uint8), scales[:1], bias[:1], -INF, INF), uns),
        ((1, big, np.zeros((big, 1), np.uint8), np.full(big, 0.01, F32), None, -INF, INF), uns),
    ]
    for args, want in table:
        st, op = qnnp.create_fully_connected_nc_f32_qd8_qc4w_status(*args)
        if op:
            qnnp.delete_operator(op)
        assert st == want and bool(op) == (want == Status.success), (args[:2], args[5:], st, want)


@pytest.mark.parametrize("batch", [3, 17])
def test_int8_operator_with_the_same_weights_gives_the_same_bytes(qnnp, batch):
    """both widths set up on the same tensors through the same setup function"""
    import torch
    k, n = 200, 33
    x, w, scales, bias = problem("widths", batch, k, n)
    ops = [qnnp.create_fully_connected_nc_f32_qd8(k, n, w.astype(np.int8), scales, bias, -1.0, INF),
           qnnp.create_fully_connected_nc_f32_qd8_qc4w(k, n, pack(w), scales, bias, -1.0, INF)]
    d_x = torch.from_numpy(x).cuda()
    d_y = torch.zeros(batch * n, dtype=torch.float32, device="cuda")
    try:
        got = []
        for op in ops:
            d_y.fill_(123.0)
            qnnp.setup_fully_connected_nc_f32_qd8(op, batch, d_x, k, d_y, n)
            qnnp.run_operator(op)
            got.append(d_y.cpu().numpy().view(np.uint32).reshape(batch, n))
        assert [qnnp.operator_kernel(op) for op in ops] == [dfc.gemm_kernel(batch), kernel_name(batch)]
        same(got[1], got[0], "4-bit against int8")
    finally:
        for op in ops:
            qnnp.delete_operator(op)


@pytest.mark.parametrize("batch", [4, 40])
def test_graph_capture_follows_the_input(qnnp, batch):
    """one run recorded into the library's capture (two launches), replayed twice with changed input"""
    import torch
    k, n = 200, 33
    x, w, scales, bias = problem("graph4", batch, k, n)
    op = qnnp.create_fully_connected_nc_f32_qd8_qc4w(k, n, pack(w), scales, bias, -2.0, INF)
    d_x = torch.zeros(batch * k, dtype=torch.float32, device="cuda")
    d_y = torch.zeros(batch * n, dtype=torch.float32, device="cuda")
    try:
        qnnp.setup_fully_connected_nc_f32_qd8(op, batch, d_x, k, d_y, n)
        qnnp.graph_begin()
        try:
            qnnp.run_operator(op)
        finally:
            graph = qnnp.graph_end()
        try:
            for rep, factor in enumerate((1.0, -0.37)):
                x_rep = (x * F32(factor)).astype(F32)
                d_x.copy_(torch.from_numpy(x_rep.reshape(-1)))
                d_y.fill_(123.0)
                torch.cuda.synchronize()
                qnnp.graph_launch(graph)
                qnnp.graph_synchronize(graph)
                same(d_y.cpu().numpy().view(np.uint32).reshape(batch, n),
                     dfc.expected(x_rep, w.astype(np.int8), scales, bias, -2.0, INF), f"replay {rep}")
        finally:
            qnnp.graph_destroy(graph)
    finally:
        qnnp.delete_operator(op)
