"""GPU tier of the dynamically quantized fully connected operator with unsigned 4-bit weights, block-wise scales and one
zero point per channel and block (qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_zp: hip/qd8f32gemm4z.hip behind
dynamic-fully-connected.c). The expectation restates the header's definition -- an exact int64 sum of (q - zp)(u - z) per
block, cast to float32, then a float32 sum over the blocks in ascending order; outputs are compared as uint32 bit patterns
inside guard bytes, and the product kernel's name is asserted per case."""
import numpy as np
import pytest

import _dynamic_fc as dfc
from _gpu import Guarded
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

F32 = np.float32
INF, NAN = float("inf"), float("nan")
FILL = 0xA5A5A5A5


def terms(x, u, z, scales, block):
    """t_b [rows][N] float32 for b = 0 .. K / block - 1, scale_r [rows], and the largest |acc_b|"""
    q, scale, zp = dfc.quantize_rows(x)
    d = q.astype(np.int64) - zp[:, None]
    out, peak = [], 0
    for b in range(u.shape[1] // block):
        w = u[:, b * block:(b + 1) * block].astype(np.int64) - z[:, b:b + 1].astype(np.int64)
        acc = d[:, b * block:(b + 1) * block] @ w.T
        peak = max(peak, int(np.abs(acc).max()))
        out.append(acc.astype(F32) * scales[:, b].astype(F32)[None, :])
    assert peak < 2 ** 20
    return out, scale, peak


def finish(ysum, scale, bias, lo, hi):
    y = ysum * scale[:, None]
    y = y + (np.zeros(ysum.shape[1], F32) if bias is None else bias.astype(F32))[None, :]
    y = np.minimum(np.maximum(y, F32(lo)), F32(hi))
    assert y.dtype == np.float32
    return y


def expected(x, u, z, scales, bias, block, lo=-INF, hi=INF):
    t, scale, _ = terms(x, u, z, scales, block)
    ysum = np.zeros_like(t[0])
    for t_b in t:                       # the definition's order
        ysum = ysum + t_b
    return finish(ysum, scale, bias, lo, hi)


def pack(v):
    """v [N][K] nibbles (unsigned, or signed in [-8, 7]), K even -> [N][K / 2] bytes, weight k in bits 4 (k % 2) .. of byte k / 2"""
    nibbles = (v & 15).astype(np.uint8)
    return nibbles[:, 0::2] | (nibbles[:, 1::2] << 4)


def problem(name, batch, k, n, block):
    """x, u, z, scales, bias: zero points drawn per (channel, block) over 0 .. 15; 15 is forced to occur, and 0 beside it
    wherever there is more than one entry"""
    x, _, _, bias = dfc.problem(name, batch, k, n)
    rng = np.random.default_rng(sum(name.encode()) * 131 + block)
    u = rng.integers(0, 16, size=(n, k))
    z = rng.integers(0, 16, size=(n, k // block))
    z.flat[0], z.flat[-1] = 0, 15
    return x, u, z, rng.uniform(0.002, 0.05, size=(n, k // block)).astype(F32), bias


def kernel_name(batch):
    return "qd8_f32_qb4w_zp_gemv_mfma_16" if batch <= 16 else "qd8_f32_qb4w_zp_gemm_mfma_128x128"


def same(got, want, what):
    bad = np.argwhere(got != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} differ, first at {bad[:4].tolist()}"


def run(qnnp, name, op, kernel, x, n, in_extra=0, out_extra=0, in_off=0, out_off=0):
    """one setup and run of `op` (deleted here) on fresh guarded buffers, strides above the channel counts by *_extra
    elements, bases offset by *_off bytes; returns the output bits [batch][n]"""
    batch, k = x.shape
    in_stride, out_stride = k + in_extra, n + out_extra
    x_host = np.full((batch - 1) * in_stride + k, 7.25, F32)
    for r in range(batch):
        x_host[r * in_stride:r * in_stride + k] = x[r]
    gx, gy = Guarded(x_host, in_off), Guarded(np.full((batch - 1) * out_stride + n, FILL, np.uint32), out_off)
    try:
        assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, gx, in_stride, gy, out_stride) == Status.success, name
        qnnp.run_operator(op)
        assert qnnp.operator_kernel(op) == kernel, (name, qnnp.operator_kernel(op))
        assert qnnp.dynamic_rows_kernel(op).startswith("f32_qd8_rows_"), name
    finally:
        qnnp.delete_operator(op)
    got = gy.read().view(np.uint32)
    gy.assert_intact(name)
    gx.assert_intact(name + " (input)")
    cells = (np.arange(batch)[:, None] * out_stride + np.arange(n)).ravel()
    assert np.all(np.delete(got, cells) == FILL), name + ": a gap between output rows was written"
    return got[cells].reshape(batch, n)


def check(qnnp, name, x, u, z, scales, bias, block, lo=-INF, hi=INF, want=None, **layout):
    want = expected(x, u, z, scales, bias, block, lo, hi) if want is None else want
    op = qnnp.create_fully_connected_nc_f32_qd8_qb4w_zp(x.shape[1], u.shape[0], block, pack(u), scales, z, bias, lo, hi)
    got = run(qnnp, name, op, kernel_name(x.shape[0]), x, u.shape[0], **layout)
    same(got, want, name)
    return want, got


# (batch, K, B, N). One block / one MFMA; an odd tile count (the last pair without its odd half); one block per step and per
# two steps; a second GEMV pass of one block at each size, and the tile kernel past a pass; both kernels at every block size
SHAPES = [(1, 64, 64, 1), (17, 64, 64, 16), (16, 192, 64, 33), (129, 192, 64, 130), (1, 128, 128, 130), (129, 128, 128, 1),
          (16, 256, 256, 16), (17, 512, 256, 33), (1, 4160, 64, 16), (16, 4224, 128, 1), (1, 4352, 256, 130), (17, 4160, 64, 33)]


@pytest.mark.parametrize("batch,k,block,n", SHAPES)
def test_shape_edges_of_each_kernel(qnnp, batch, k, block, n):
    name = f"shapez/b{batch}_k{k}_B{block}_n{n}"
    check(qnnp, name, *problem(name, batch, k, n, block), block)


@pytest.mark.parametrize("batch", [1, 17])
@pytest.mark.parametrize("block", [64, 256])
def test_blocks_at_the_integer_bound(qnnp, batch, block):
    """u - z at +15 and -15, whole rows and alternating from block to block, activations at the ends of their range:
    |acc_b| reaches 255 * 15 * B"""
    k, n = 512, 16
    odd = (np.arange(k // block) % 2 == 1)[None, :]
    z = np.empty((n, k // block), np.int64)
    z[0::4], z[1::4], z[2::4], z[3::4] = 0, 15, np.where(odd, 15, 0), np.where(odd, 0, 15)
    u = np.repeat(15 - z, block, axis=1)
    scales = problem("boundz", batch, k, n, block)[3]
    reached = []
    for pattern, row in (("all_high", np.ones(k, F32)), ("all_low", -np.ones(k, F32)),
                         ("both_ends", np.tile(np.array([0.0, 2.0], F32), k // 2))):
        x = np.tile(row, (batch, 1))
        reached.append(terms(x, u, z, scales, block)[2])
        check(qnnp, f"boundz/{pattern}/b{batch}_B{block}", x, u, z, scales, np.arange(n, dtype=F32), block)
    assert max(reached) == 255 * 15 * block


@pytest.mark.parametrize("batch", [3, 17])
def test_the_sum_over_blocks_runs_in_ascending_order(qnnp, batch):
    """block scales alternating between about 2^9 and 2^-9: any other order of the same terms rounds differently"""
    k, n, block = 2048, 33, 64
    x, u, z, scales, bias = problem("orderz", batch, k, n, block)
    scales = (np.where(np.arange(k // block) % 2 == 0, 2.0 ** 9, 2.0 ** -9) * (scales / F32(0.05) + F32(1))).astype(F32)
    t, scale, _ = terms(x, u, z, scales, block)
    want = expected(x, u, z, scales, bias, block)
    backwards = np.zeros_like(t[0])
    for t_b in reversed(t):
        backwards = backwards + t_b
    pairwise = list(t)
    while len(pairwise) > 1:
        pairwise = [pairwise[i] + pairwise[i + 1] for i in range(0, len(pairwise), 2)]
    for other in (backwards, pairwise[0]):
        assert (finish(other, scale, bias, -INF, INF).view(np.uint32) != want.view(np.uint32)).any()
    check(qnnp, f"orderz/b{batch}", x, u, z, scales, bias, block, want=want)


@pytest.mark.parametrize("batch", [3, 17])
def test_zero_points_of_eight_equal_the_signed_operator(qnnp, batch):
    """u = w + 8 and z = 8 everywhere: byte-equal to the _qb4w operator on the signed nibbles w and the same scales"""
    k, n, block = 256, 33, 128
    x, u, _, scales, bias = problem("equalz", batch, k, n, block)
    w, z = u - 8, np.full((n, k // block), 8)
    _, got = check(qnnp, f"equalz/b{batch}", x, u, z, scales, bias, block)
    signed = qnnp.create_fully_connected_nc_f32_qd8_qb4w(k, n, block, pack(w), scales, bias, -INF, INF)
    assert (pack(w) ^ 0x88 == pack(u)).all()
    assert (run(qnnp, f"equalz/qb4w/b{batch}", signed, kernel_name(batch).replace("_zp", ""), x, n) == got).all()


@pytest.mark.parametrize("batch", [3, 17])
def test_carried_over_layout_clamp_and_special_rows(qnnp, batch):
    """strided rows and offset bases; a clamp that cuts, and a NULL bias; an all-zero row and a non-finite row (both take
    scale_r = 1)"""
    name = f"layoutz/b{batch}"
    check(qnnp, name, *problem(name, batch, 256, 33, 128), 128, in_extra=1, out_extra=1, in_off=12, out_off=8)
    x, u, z, scales, bias = problem("clampz", batch, 256, 33, 64)
    want, _ = check(qnnp, f"clampz/b{batch}", x, u, z, scales, bias, 64, -0.5, 0.75)
    assert (want == F32(-0.5)).any() and (want == F32(0.75)).any() and ((want > -0.5) & (want < 0.75)).any()
    check(qnnp, f"no biasz/b{batch}", x, u, z, scales, None, 64)
    x[0] = 0
    x[1, [3, 5, 7]] = NAN, INF, -INF
    assert (dfc.quantize_rows(x)[1][:2] == 1).all()
    check(qnnp, f"specialz/b{batch}", x, u, z, scales, bias, 64)


def test_create_refusals_in_their_order(qnnp):
    k, n, block = 128, 4, 64
    kernel, scales, bias = np.full((n, k // 2), 0x1F, np.uint8), np.full((n, k // block), 0.01, F32), np.zeros(n, F32)
    zps = np.full((n, k // block), 3, np.uint8)

    def with_(array, value):
        out = array.copy()
        out[2, 1] = value
        return out
    wide_s, wide_z = np.full((n, 4), 0.01, F32), np.full((n, 4), 3, np.uint8)
    inv, uns = Status.invalid_parameter, Status.unsupported_parameter
    table = [
        ((k, n, block, kernel, scales, zps, bias, -INF, INF), Status.success),
        ((k, n, 0, kernel, scales, zps, bias, -INF, INF), inv),
        ((k, n, block, kernel, scales, None, bias, -INF, INF), inv),
        ((k, n, block, kernel, with_(scales, 1e-40), zps, bias, -INF, INF), inv),
        ((k, n, block, kernel, scales, with_(zps, 16), bias, -INF, INF), inv),
        ((k, n, 32, kernel, wide_s, with_(wide_z, 16), bias, -INF, INF), inv),         # invalid before unsupported
        ((k, n, 32, kernel, wide_s, wide_z, bias, 1.0, 0.5), inv),
        ((k, n, block, kernel, with_(scales, 2.0 ** -17), zps, np.array([0, NAN, 0, 0], F32), -INF, INF), inv),
        ((k, n, 32, kernel, wide_s, wide_z, bias, -INF, INF), uns),                    # block size 32 is still refused
        ((k, n, 512, kernel, scales, zps, bias, -INF, INF), uns),
        ((192, n, 128, np.zeros((n, 96), np.uint8), scales, zps, bias, -INF, INF), uns),   # K is no multiple of B
        ((k, n, block, kernel, with_(scales, float(np.nextafter(F32(2.0 ** -16), F32(0)))), zps, bias, -INF, INF), uns),
        ((k, n, block, kernel, with_(scales, 2.0 ** 16), with_(zps, 15), bias, -INF, INF), Status.success),
        ((32768 + 64, 1, 64, np.zeros((1, 16416), np.uint8), np.full((1, 513), 0.01, F32), np.zeros((1, 513), np.uint8),
          None, -INF, INF), uns),
    ]
    for args, want in table:
        st, op = qnnp.create_fully_connected_nc_f32_qd8_qb4w_zp_status(*args)
        if op:
            qnnp.delete_operator(op)
        assert st == want and bool(op) == (want == Status.success), (args[:3], args[7:], st, want)


@pytest.mark.parametrize("batch", [3, 17])
def test_graph_capture_follows_the_input(qnnp, batch):
    """one run recorded into the library's capture (two launches), replayed twice with changed input"""
    import torch
    k, n, block = 256, 33, 128
    x, u, z, scales, bias = problem("graphz", batch, k, n, block)
    op = qnnp.create_fully_connected_nc_f32_qd8_qb4w_zp(k, n, block, pack(u), scales, z, bias, -2.0, INF)
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
                     expected(x_rep, u, z, scales, bias, block, -2.0, INF), f"replay {rep}")
        finally:
            qnnp.graph_destroy(graph)
    finally:
        qnnp.delete_operator(op)
