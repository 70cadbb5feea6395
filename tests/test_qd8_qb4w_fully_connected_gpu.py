"""GPU tier of the dynamically quantized fully connected operator with 4-bit weights and block-wise scales
(qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w: hip/qd8f32gemm4b.hip behind dynamic-fully-connected.c). The
expectation restates the header's definition -- an exact integer sum per block, then a float32 sum over the blocks in
ascending order; outputs are compared as uint32 bit patterns inside guard bytes, and the product kernel's name is asserted
per case."""
import numpy as np
import pytest

import _dynamic_fc as dfc
from _gpu import Guarded
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

F32 = np.float32
INF, NAN = float("inf"), float("nan")
FILL = 0xA5A5A5A5


def terms(x, w, scales, block):
    """t_b [rows][N] float32 for b = 0 .. K / block - 1, and scale_r [rows]"""
    q, scale, zp = dfc.quantize_rows(x)
    d = q.astype(np.int64) - zp[:, None]
    out = []
    for b in range(w.shape[1] // block):
        acc = d[:, b * block:(b + 1) * block] @ w[:, b * block:(b + 1) * block].astype(np.int64).T
        assert np.abs(acc).max() < 2 ** 31, "a block's sum must fit int32 by itself"
        out.append(acc.astype(F32) * scales[:, b].astype(F32)[None, :])
    return out, scale


def finish(ysum, scale, bias, lo, hi):
    y = ysum * scale[:, None]
    y = y + (np.zeros(ysum.shape[1], F32) if bias is None else bias.astype(F32))[None, :]
    y = np.minimum(np.maximum(y, F32(lo)), F32(hi))
    assert y.dtype == np.float32
    return y


def expected(x, w, scales, bias, block, lo=-INF, hi=INF):
    t, scale = terms(x, w, scales, block)
    ysum = np.zeros_like(t[0])
    for t_b in t:                       # the definition's order
        ysum = ysum + t_b
    return finish(ysum, scale, bias, lo, hi)


def pack(w):
    """w [N][K] in [-8, 7], K even -> [N][K / 2] bytes, weight k in bits 4 (k % 2) .. of byte k / 2"""
    nibbles = w.astype(np.int8).view(np.uint8) & 15
    return nibbles[:, 0::2] | (nibbles[:, 1::2] << 4)


def problem(name, batch, k, n, block):
    x, kernel, _, bias = dfc.problem(name, batch, k, n)
    rng = np.random.default_rng(sum(name.encode()) * 131 + block)
    return x, (kernel >> 4).astype(np.int64), rng.uniform(0.002, 0.05, size=(n, k // block)).astype(F32), bias


def kernel_name(batch):
    return "qd8_f32_qb4w_gemv_mfma_16" if batch <= 16 else "qd8_f32_qb4w_gemm_mfma_128x128"


def same(got, want, what):
    bad = np.argwhere(got != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} differ, first at {bad[:4].tolist()}"


def check(qnnp, name, x, w, scales, bias, block, lo=-INF, hi=INF, want=None, in_extra=0, out_extra=0, in_off=0, out_off=0):
    """create, one setup and run on fresh guarded buffers (strides above the channel counts by *_extra elements, bases
    offset by *_off bytes), compare with the definition; returns the expectation"""
    (batch, k), n = x.shape, w.shape[0]
    want = expected(x, w, scales, bias, block, lo, hi) if want is None else want
    in_stride, out_stride = k + in_extra, n + out_extra
    x_host = np.full((batch - 1) * in_stride + k, 7.25, F32)
    for r in range(batch):
        x_host[r * in_stride:r * in_stride + k] = x[r]
    gx, gy = Guarded(x_host, in_off), Guarded(np.full((batch - 1) * out_stride + n, FILL, np.uint32), out_off)
    op = qnnp.create_fully_connected_nc_f32_qd8_qb4w(k, n, block, pack(w), scales, bias, lo, hi)
    try:
        assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, gx, in_stride, gy, out_stride) == Status.success, name
        qnnp.run_operator(op)
        assert qnnp.operator_kernel(op) == kernel_name(batch), (name, qnnp.operator_kernel(op))
        assert qnnp.dynamic_rows_kernel(op).startswith("f32_qd8_rows_"), name
    finally:
        qnnp.delete_operator(op)
    got = gy.read().view(np.uint32)
    gy.assert_intact(name)
    gx.assert_intact(name + " (input)")
    cells = (np.arange(batch)[:, None] * out_stride + np.arange(n)).ravel()
    assert np.all(np.delete(got, cells) == FILL), name + ": a gap between output rows was written"
    same(got[cells].reshape(batch, n), want, name)
    return want


# (batch, K, B, N). One block / one MFMA; an odd tile count (the last pair without its odd half); one block per step and per
# two steps; exactly one GEMV pass, a second pass of one block, of two, of one 256-wide; both kernels for every (K, B)
SHAPES = [(1, 64, 64, 1), (17, 64, 64, 16), (16, 64, 64, 130), (16, 192, 64, 33), (129, 192, 64, 130), (1, 128, 128, 130),
          (129, 128, 128, 1), (16, 256, 256, 16), (17, 256, 256, 33), (1, 512, 256, 33), (129, 512, 256, 16),
          (16, 4096, 128, 130), (17, 4096, 128, 1), (129, 4096, 128, 16), (1, 4160, 64, 16), (17, 4160, 64, 33),
          (16, 4224, 128, 1), (129, 4224, 128, 33), (1, 4352, 256, 130), (17, 4352, 256, 16)]


@pytest.mark.parametrize("batch,k,block,n", SHAPES)
def test_shape_edges_of_each_kernel(qnnp, batch, k, block, n):
    name = f"shapeb/b{batch}_k{k}_B{block}_n{n}"
    check(qnnp, name, *problem(name, batch, k, n, block), block)


@pytest.mark.parametrize("batch", [3, 17])
def test_the_sum_over_blocks_runs_in_ascending_order(qnnp, batch):
    """block scales alternating between about 2^9 and 2^-9: any other order of the same terms rounds differently"""
    k, n, block = 2048, 33, 64
    x, w, scales, bias = problem("order", batch, k, n, block)
    scales = (np.where(np.arange(k // block) % 2 == 0, 2.0 ** 9, 2.0 ** -9) * (scales / F32(0.05) + F32(1))).astype(F32)
    t, scale = terms(x, w, scales, block)
    want = expected(x, w, scales, bias, block)
    backwards = np.zeros_like(t[0])
    for t_b in reversed(t):
        backwards = backwards + t_b
    pairwise = list(t)
    while len(pairwise) > 1:
        pairwise = [pairwise[i] + pairwise[i + 1] for i in range(0, len(pairwise), 2)]
    for other in (backwards, pairwise[0]):
        assert (finish(other, scale, bias, -INF, INF).view(np.uint32) != want.view(np.uint32)).any()
    check(qnnp, f"order/b{batch}", x, w, scales, bias, block, want=want)


@pytest.mark.parametrize("batch", [1, 17])
@pytest.mark.parametrize("block", [64, 256])
def test_many_blocks_at_the_integer_bound(qnnp, batch, block):
    """K = 32768 (512 blocks of 64), weights at 7 and -8, activations at the ends of their range: the kernels' per-block
    integer 16 * acc_b reaches 16 * 255 * 8 * B"""
    k, n = 32768, 16
    w = np.empty((n, k), np.int64)
    w[0::4], w[1::4] = 7, -8
    w[2::4] = np.where(np.arange(k) % 2 == 1, 7, -8)
    w[3::4] = np.where(np.arange(k) % 2 == 1, -8, 7)
    scales = problem("boundb", batch, k, n, block)[2]
    reached = []
    for pattern, row in (("all_high", np.ones(k, F32)), ("all_low", -np.ones(k, F32)),
                         ("both_ends", np.tile(np.array([0.0, 2.0], F32), k // 2))):
        x = np.tile(row, (batch, 1))
        q, _, zp = dfc.quantize_rows(x[:1])
        acc = ((q.astype(np.int64) - zp[:, None]).reshape(-1, block) * w[1].reshape(-1, block)).sum(axis=1)
        reached.append(16 * np.abs(acc).max())
        check(qnnp, f"boundb/{pattern}/b{batch}_B{block}", x, w, scales, np.arange(n, dtype=F32), block)
    assert max(reached) == 16 * 255 * 8 * block < 2 ** 24


@pytest.mark.parametrize("batch", [3, 17])
def test_strided_rows_and_offset_bases(qnnp, batch):
    name = f"layoutb/b{batch}"
    check(qnnp, name, *problem(name, batch, 256, 33, 128), 128, in_extra=1, out_extra=1, in_off=12, out_off=8)


@pytest.mark.parametrize("batch", [3, 17])
def test_clamp_cuts_and_null_bias(qnnp, batch):
    x, w, scales, bias = problem("clampb", batch, 256, 33, 64)
    want = check(qnnp, f"clampb/b{batch}", x, w, scales, bias, 64, -0.5, 0.75)
    assert (want == F32(-0.5)).any() and (want == F32(0.75)).any() and ((want > -0.5) & (want < 0.75)).any()
    check(qnnp, f"no biasb/b{batch}", x, w, scales, None, 64)


@pytest.mark.parametrize("batch", [3, 17])
def test_zero_row_and_non_finite_row(qnnp, batch):
    """both rows take scale_r = 1 through the new epilogue"""
    x, w, scales, bias = problem("specialb", batch, 256, 33, 128)
    x[0] = 0
    x[1, [3, 5, 7]] = NAN, INF, -INF
    assert (dfc.quantize_rows(x)[1][:2] == 1).all()
    check(qnnp, f"specialb/b{batch}", x, w, scales, bias, 128)


def test_create_refusals_in_their_order(qnnp):
    k, n, block = 128, 4, 64
    kernel, scales, bias = np.full((n, k // 2), 0x11, np.uint8), np.full((n, k // block), 0.01, F32), np.zeros(n, F32)

    def with_(value):
        out = scales.copy()
        out[2, 1] = value
        return out
    inv, uns = Status.invalid_parameter, Status.unsupported_parameter
    table = [
        ((k, n, block, kernel, scales, bias, -INF, INF), Status.success),
        ((k, n, 0, kernel, scales, bias, -INF, INF), inv),
        ((k, n, block, kernel, with_(1e-40), bias, -INF, INF), inv),
        ((k, n, 32, kernel, scales, bias, 1.0, 0.5), inv),                            # invalid before unsupported
        ((k, n, block, kernel, with_(2.0 ** -17), np.array([0, NAN, 0, 0], F32), -INF, INF), inv),
        ((k, n, 32, kernel, np.full((n, 4), 0.01, F32), bias, -INF, INF), uns),
        ((k, n, 512, kernel, scales, bias, -INF, INF), uns),
        ((192, n, 128, np.zeros((n, 96), np.uint8), scales, bias, -INF, INF), uns),   # K is no multiple of B
        ((k, n, block, kernel, with_(float(np.nextafter(F32(2.0 ** -16), F32(0)))), bias, -INF, INF), uns),
        ((k, n, block, kernel, with_(float(np.nextafter(F32(2.0 ** 16), F32(INF)))), bias, -INF, INF), uns),
        ((k, n, block, kernel, with_(2.0 ** -16), bias, -INF, INF), Status.success),
        ((k, n, block, kernel, with_(2.0 ** 16), bias, -INF, INF), Status.success),
        ((32768 + 64, 1, 64, np.zeros((1, 16416), np.uint8), np.full((1, 513), 0.01, F32), None, -INF, INF), uns),
    ]
    for args, want in table:
        st, op = qnnp.create_fully_connected_nc_f32_qd8_qb4w_status(*args)
        if op:
            qnnp.delete_operator(op)
        assert st == want and bool(op) == (want == Status.success), (args[:3], args[6:], st, want)


@pytest.mark.parametrize("batch", [4, 40])
def test_graph_capture_follows_the_input(qnnp, batch):
    """one run recorded into the library's capture (two launches), replayed twice with changed input"""
    import torch
    k, n, block = 256, 33, 128
    x, w, scales, bias = problem("graphb", batch, k, n, block)
    op = qnnp.create_fully_connected_nc_f32_qd8_qb4w(k, n, block, pack(w), scales, bias, -2.0, INF)
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
                     expected(x_rep, w, scales, bias, block, -2.0, INF), f"replay {rep}")
        finally:
            qnnp.graph_destroy(graph)
    finally:
        qnnp.delete_operator(op)
