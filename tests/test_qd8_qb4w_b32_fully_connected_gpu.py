"""GPU tier of the dynamically quantized fully connected operator with 4-bit weights in blocks of 32, one scale and one zero
point per channel and block (qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_b32: hip/qd8f32gemm4s.hip behind
dynamic-fully-connected.c). The expectation restates the header's definition -- an exact int64 sum of (q - zp)(u - z) per
32-block, cast to float32, then a float32 sum over the blocks in ascending order; outputs are compared as uint32 bit patterns
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
B = 32


def terms(x, d, scales):
    """t_b [rows][N] float32 for b = 0 .. K / 32 - 1 from d = u - z [N][K], scale_r [rows], and the largest |acc_b|"""
    q, scale, zp = dfc.quantize_rows(x)
    a = q.astype(np.int64) - zp[:, None]
    out, peak = [], 0
    for b in range(d.shape[1] // B):
        acc = a[:, b * B:(b + 1) * B] @ d[:, b * B:(b + 1) * B].astype(np.int64).T
        peak = max(peak, int(np.abs(acc).max()))
        out.append(acc.astype(F32) * scales[:, b].astype(F32)[None, :])
    assert peak < 2 ** 17
    return out, scale, peak


def finish(ysum, scale, bias):
    y = ysum * scale[:, None] + bias.astype(F32)[None, :]
    assert y.dtype == np.float32
    return y


def expected(x, d, scales, bias):
    t, scale, _ = terms(x, d, scales)
    ysum = np.zeros_like(t[0])
    for t_b in t:                       # the definition's order
        ysum = ysum + t_b
    return finish(ysum, scale, bias)


def pack(v):
    """v [N][K] nibbles (unsigned, or signed in [-8, 7]) -> [N][K / 2] bytes, weight k in bits 4 (k % 2) .. of byte k / 2"""
    nibbles = (v & 15).astype(np.uint8)
    return nibbles[:, 0::2] | (nibbles[:, 1::2] << 4)


def problem(name, batch, k, n):
    """x, u, z, scales, bias: zero points drawn per (channel, block) over 0 .. 15; 15 is forced to occur, and 0 beside it
    wherever there is more than one entry"""
    x, _, _, bias = dfc.problem(name, batch, k, n)
    rng = np.random.default_rng(sum(name.encode()) * 131 + B)
    u = rng.integers(0, 16, size=(n, k))
    z = rng.integers(0, 16, size=(n, k // B))
    z.flat[0], z.flat[-1] = 0, 15
    return x, u, z, rng.uniform(0.002, 0.05, size=(n, k // B)).astype(F32), bias


def run(qnnp, name, op, x, n, in_extra=0, out_extra=0, in_off=0, out_off=0):
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
        kernel = "qd8_f32_qb4w_b32_gemv_mfma_16" if batch <= 16 else "qd8_f32_qb4w_b32_gemm_mfma_128x128"
        assert qnnp.operator_kernel(op) == kernel, (name, qnnp.operator_kernel(op))
    finally:
        qnnp.delete_operator(op)
    got = gy.read().view(np.uint32)
    gy.assert_intact(name)
    gx.assert_intact(name + " (input)")
    cells = (np.arange(batch)[:, None] * out_stride + np.arange(n)).ravel()
    assert np.all(np.delete(got, cells) == FILL), name + ": a gap between output rows was written"
    return got[cells].reshape(batch, n)


def check(qnnp, name, x, u, z, scales, bias, want=None, **layout):
    """z None: `u` holds signed nibbles and the create gets no zero points"""
    d = u if z is None else u - np.repeat(z, B, axis=1)
    want = expected(x, d, scales, bias) if want is None else want
    k, n = x.shape[1], u.shape[0]
    op = qnnp.create_fully_connected_nc_f32_qd8_qb4w_b32(k, n, pack(u), scales, None if z is None else z.astype(np.uint8),
                                                         bias, -INF, INF)
    got = run(qnnp, name, op, x, n, **layout)
    bad = np.argwhere(got != want.view(np.uint32))
    assert len(bad) == 0, f"{name}: {len(bad)} of {want.size} differ, first at {bad[:4].tolist()}"
    return got


# (batch, K, N). K = 32: one block, half a tile; 64: two blocks in one tile; 96 and 160: an odd block count, the last pair
# without its odd tile at 160; 2080: one block past a GEMV pass of 32 tiles. Both kernels see every K
SHAPES = [(1, 32, 1), (17, 32, 16), (129, 32, 33), (16, 64, 33), (129, 64, 130), (1, 96, 130), (17, 96, 33), (16, 160, 16),
          (129, 160, 1), (1, 160, 130), (1, 2080, 16), (17, 2080, 33)]


@pytest.mark.parametrize("batch,k,n", SHAPES)
def test_shape_edges_of_each_kernel(qnnp, batch, k, n):
    name = f"shape32/b{batch}_k{k}_n{n}"
    check(qnnp, name, *problem(name, batch, k, n))


@pytest.mark.parametrize("batch", [3, 17])
def test_blocks_at_the_integer_bound(qnnp, batch):
    """u - z at +15 and -15, whole rows and alternating from block to block, activations at the ends of their range:
    |acc_b| reaches 255 * 15 * 32"""
    k, n = 128, 16
    odd = (np.arange(k // B) % 2 == 1)[None, :]
    z = np.empty((n, k // B), np.int64)
    z[0::4], z[1::4], z[2::4], z[3::4] = 0, 15, np.where(odd, 15, 0), np.where(odd, 0, 15)
    u = np.repeat(15 - z, B, axis=1)
    scales = problem("bound32", batch, k, n)[3]
    reached = []
    for pattern, row in (("all_high", np.ones(k, F32)), ("all_low", -np.ones(k, F32)),
                         ("both_ends", np.tile(np.array([0.0, 2.0], F32), k // 2))):
        x = np.tile(row, (batch, 1))
        reached.append(terms(x, u - np.repeat(z, B, axis=1), scales)[2])
        check(qnnp, f"bound32/{pattern}/b{batch}", x, u, z, scales, np.arange(n, dtype=F32))
    assert max(reached) == 255 * 15 * 32


@pytest.mark.parametrize("batch", [3, 17])
def test_the_sum_over_blocks_runs_in_ascending_order(qnnp, batch):
    """block scales alternating between about 2^9 and 2^-9: any other order of the same terms rounds differently"""
    k, n = 2048, 33
    x, u, z, scales, bias = problem("order32", batch, k, n)
    scales = (np.where(np.arange(k // B) % 2 == 0, 2.0 ** 9, 2.0 ** -9) * (scales / F32(0.05) + F32(1))).astype(F32)
    t, scale, _ = terms(x, u - np.repeat(z, B, axis=1), scales)
    want = expected(x, u - np.repeat(z, B, axis=1), scales, bias)
    backwards = np.zeros_like(t[0])
    for t_b in reversed(t):
        backwards = backwards + t_b
    pairwise = list(t)
    while len(pairwise) > 1:
        pairwise = [pairwise[i] + pairwise[i + 1] for i in range(0, len(pairwise), 2)]
    for other in (backwards, pairwise[0]):
        assert (finish(other, scale, bias).view(np.uint32) != want.view(np.uint32)).any()
    check(qnnp, f"order32/b{batch}", x, u, z, scales, bias, want=want)


@pytest.mark.parametrize("batch", [3, 17])
def test_signed_nibbles_equal_zero_points_of_eight(qnnp, batch):
    """no zero points on signed nibbles w, and zero point 8 everywhere on w ^ 8: the same bits, and numpy's"""
    k, n = 160, 33
    x, u, _, scales, bias = problem("signed32", batch, k, n)
    w = u - 8
    assert ((w & 15) ^ 8 == u).all()
    signed = check(qnnp, f"signed32/w/b{batch}", x, w, None, scales, bias)
    assert (check(qnnp, f"signed32/u/b{batch}", x, u, np.full((n, k // B), 8), scales, bias) == signed).all()


@pytest.mark.parametrize("batch", [3, 17])
def test_strided_rows_and_offset_bases(qnnp, batch):
    name = f"layout32/b{batch}"
    check(qnnp, name, *problem(name, batch, 160, 33), in_extra=1, out_extra=1, in_off=12, out_off=8)


def _with(array, value):
    out = array.copy()
    out[2, 1] = value
    return out


K, N = 128, 4
KERNEL, SCALES, ZPS = np.full((N, K // 2), 0x1F, np.uint8), np.full((N, K // B), 0.01, F32), np.full((N, K // B), 3, np.uint8)
BIAS, K48 = np.zeros(N, F32), (48, N, np.zeros((N, 24), np.uint8), SCALES[:, :1])
INV, UNS = Status.invalid_parameter, Status.unsupported_parameter
BELOW = float(np.nextafter(F32(2.0 ** -16), F32(0)))


@pytest.mark.parametrize("args,want", [
    ((K, N, KERNEL, SCALES, ZPS, BIAS, -INF, INF), Status.success),
    ((K, N, KERNEL, SCALES, None, BIAS, -INF, INF), Status.success),                      # signed nibbles
    ((0, N, KERNEL, SCALES, ZPS, BIAS, -INF, INF), INV),
    ((K, N, None, SCALES, ZPS, BIAS, -INF, INF), INV),
    ((K, N, KERNEL, None, ZPS, BIAS, -INF, INF), INV),
    ((K, N, KERNEL, _with(SCALES, 1e-40), ZPS, BIAS, -INF, INF), INV),
    ((K, N, KERNEL, SCALES, _with(ZPS, 16), BIAS, -INF, INF), INV),
    ((K, N, KERNEL, _with(SCALES, BELOW), ZPS, np.array([0, NAN, 0, 0], F32), -INF, INF), INV),
    ((K, N, KERNEL, SCALES, ZPS, BIAS, 1.0, 0.5), INV),
    (K48 + (ZPS[:, :1], BIAS, 1.0, 0.5), INV),                                            # invalid before unsupported
    (K48 + (np.full((N, 1), 16, np.uint8), BIAS, -INF, INF), INV),
    (K48 + (ZPS[:, :1], BIAS, -INF, INF), UNS),                                           # K is no multiple of 32
    ((K, N, KERNEL, _with(SCALES, BELOW), ZPS, BIAS, -INF, INF), UNS),
    ((K, N, KERNEL, _with(SCALES, 2.0 ** 16), _with(ZPS, 15), BIAS, -INF, INF), Status.success),
    ((32768 + 32, 1, np.zeros((1, 16400), np.uint8), np.full((1, 1025), 0.01, F32), np.zeros((1, 1025), np.uint8), None,
      -INF, INF), UNS),
])
def test_create_refusals_in_their_order(qnnp, args, want):
    st, op = qnnp.create_fully_connected_nc_f32_qd8_qb4w_b32_status(*args)
    if op:
        qnnp.delete_operator(op)
    assert st == want and bool(op) == (want == Status.success), (args[:2], args[5:], st, want)
