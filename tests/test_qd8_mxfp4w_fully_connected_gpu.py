"""GPU tier of the dynamically quantized fully connected operator with MXFP4 weights: E2M1 codes and one E8M0 scale per
channel and block of 32 (qnnp_gfx950_create_fully_connected_nc_f32_qd8_mxfp4w: hip/qd8f32gemm4m.hip behind
dynamic-fully-connected.c). The expectation restates the header's definition -- an exact int64 sum of (q - zp) w2 per block
through a 16-entry table of twice the E2M1 values, np.ldexp in float32, then a float32 sum over the blocks in ascending
order; outputs are compared as uint32 bit patterns inside guard bytes, and the product kernel's name is asserted per case."""
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
W2 = np.array([0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12], np.int64)     # twice the value of code 0 .. 15


def terms(x, codes, e):
    """t_b [rows][N] float32 for b = 0 .. K / 32 - 1 from codes [N][K] and E8M0 bytes e [N][K / 32], scale_r [rows], and
    the largest |acc_b|"""
    q, scale, zp = dfc.quantize_rows(x)
    a, w2 = q.astype(np.int64) - zp[:, None], W2[codes]
    out, peak = [], 0
    for b in range(codes.shape[1] // B):
        acc = a[:, b * B:(b + 1) * B] @ w2[:, b * B:(b + 1) * B].T
        peak = max(peak, int(np.abs(acc).max()))
        out.append(np.ldexp(acc.astype(F32), e[None, :, b].astype(np.int32) - 128))
    assert peak <= 97920 and all(t.dtype == np.float32 for t in out)
    return out, scale, peak


def finish(ysum, scale, bias):
    y = ysum * scale[:, None] + bias.astype(F32)[None, :]
    assert y.dtype == np.float32
    return y


def expected(x, codes, e, bias):
    t, scale, _ = terms(x, codes, e)
    ysum = np.zeros_like(t[0])
    for t_b in t:                       # the definition's order
        ysum = ysum + t_b
    return finish(ysum, scale, bias)


def pack(v):
    """v [N][K] codes or nibbles -> [N][K / 2] bytes, weight k in bits 4 (k % 2) .. of byte k / 2"""
    nibbles = (v & 15).astype(np.uint8)
    return nibbles[:, 0::2] | (nibbles[:, 1::2] << 4)


def problem(name, batch, k, n):
    """x, codes, e, bias: codes uniform over 0 .. 15, exponents over a few values around 120"""
    x, _, _, bias = dfc.problem(name, batch, k, n)
    rng = np.random.default_rng(sum(name.encode()) * 131 + B)
    return x, rng.integers(0, 16, size=(n, k)), rng.integers(117, 124, size=(n, k // B)).astype(np.uint8), bias


def run(qnnp, name, op, x, n, kernel="mxfp4w", in_extra=0, out_extra=0, in_off=0, out_off=0):
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
        want = f"qd8_f32_{kernel}_gemv_mfma_16" if batch <= 16 else f"qd8_f32_{kernel}_gemm_mfma_128x128"
        assert qnnp.operator_kernel(op) == want, (name, qnnp.operator_kernel(op))
    finally:
        qnnp.delete_operator(op)
    got = gy.read().view(np.uint32)
    gy.assert_intact(name)
    gx.assert_intact(name + " (input)")
    cells = (np.arange(batch)[:, None] * out_stride + np.arange(n)).ravel()
    assert np.all(np.delete(got, cells) == FILL), name + ": a gap between output rows was written"
    return got[cells].reshape(batch, n)


def check(qnnp, name, x, codes, e, bias, want=None, **layout):
    want = expected(x, codes, e, bias) if want is None else want
    k, n = x.shape[1], codes.shape[0]
    op = qnnp.create_fully_connected_nc_f32_qd8_mxfp4w(k, n, pack(codes), e, bias, -INF, INF)
    got = run(qnnp, name, op, x, n, **layout)
    bad = np.argwhere(got != want.view(np.uint32))
    assert len(bad) == 0, f"{name}: {len(bad)} of {want.size} differ, first at {bad[:4].tolist()}"
    return got


def edge_rows(batch, k):
    """rows of ones, of minus ones and of alternating 0 / 2 in turn: zero point 0 or 255, q - zp_r reaching +-255"""
    patterns = np.stack([np.ones(k, F32), -np.ones(k, F32), np.tile(np.array([0.0, 2.0], F32), k // 2)])
    return patterns[np.arange(batch) % 3]


# (batch, K, N). K = 32: one block, half a tile; 64: two blocks in one tile; 96 and 160: an odd block count, the last pair
# without its odd tile at 160; 2080: one block past a GEMV pass of 32 tiles. Both kernels see every K
SHAPES = [(1, 32, 1), (17, 32, 16), (129, 32, 33), (16, 64, 33), (129, 64, 130), (1, 96, 130), (17, 96, 33), (16, 160, 16),
          (129, 160, 1), (1, 160, 130), (1, 2080, 16), (17, 2080, 33)]


@pytest.mark.parametrize("batch,k,n", SHAPES)
def test_shape_edges_of_each_kernel(qnnp, batch, k, n):
    name = f"shapemx/b{batch}_k{k}_n{n}"
    check(qnnp, name, *problem(name, batch, k, n))


@pytest.mark.parametrize("batch", [3, 17])
def test_every_code(qnnp, batch):
    """channel c carries code c in all 32 positions, -0 included"""
    codes = np.repeat(np.arange(16)[:, None], B, axis=1)
    check(qnnp, f"codes/b{batch}", edge_rows(batch, B), codes, np.full((16, 1), 127, np.uint8), np.zeros(16, F32))


@pytest.mark.parametrize("batch", [3, 17])
def test_blocks_at_the_integer_bound(qnnp, batch):
    """codes +6 and -6, whole rows and alternating from block to block, activations at the ends of their range:
    |acc_b| reaches 255 * 12 * 32"""
    k, n = 128, 16
    odd = (np.arange(k // B) % 2 == 1)[None, :]
    per_block = np.empty((n, k // B), np.int64)
    per_block[0::4], per_block[1::4], per_block[2::4], per_block[3::4] = 7, 15, np.where(odd, 15, 7), np.where(odd, 7, 15)
    codes, e = np.repeat(per_block, B, axis=1), problem("boundmx", batch, k, n)[2]
    x = edge_rows(batch, k)
    assert terms(x, codes, e)[2] == 255 * 12 * 32 == 97920
    check(qnnp, f"boundmx/b{batch}", x, codes, e, np.arange(n, dtype=F32))


@pytest.mark.parametrize("batch", [3, 17])
def test_the_sum_over_blocks_runs_in_ascending_order(qnnp, batch):
    """block exponents alternating between about 2^8 and 2^-10: any other order of the same terms rounds differently"""
    k, n = 2048, 33
    x, codes, e, bias = problem("ordermx", batch, k, n)
    e = (np.where(np.arange(k // B) % 2 == 0, 136, 118)[None, :] + (e & 1)).astype(np.uint8)
    t, scale, _ = terms(x, codes, e)
    want = expected(x, codes, e, bias)
    backwards = np.zeros_like(t[0])
    for t_b in reversed(t):
        backwards = backwards + t_b
    pairwise = list(t)
    while len(pairwise) > 1:
        pairwise = [pairwise[i] + pairwise[i + 1] for i in range(0, len(pairwise), 2)]
    for other in (backwards, pairwise[0]):
        assert (finish(other, scale, bias).view(np.uint32) != want.view(np.uint32)).any()
    check(qnnp, f"ordermx/b{batch}", x, codes, e, bias, want=want)


@pytest.mark.parametrize("batch", [3, 17])
def test_equals_qb4w_b32_on_signed_nibbles(qnnp, batch):
    """codes whose w2 fits a signed nibble, e in [112, 143]: _qb4w_b32 on w2 with scales 2^(e - 128) gives the same bits"""
    k, n = 160, 33
    x, codes, e, bias = problem("equalmx", batch, k, n)
    codes = np.array([c for c in range(16) if -8 <= W2[c] <= 7])[codes % 13]
    e = np.array([112, 120, 127, 128, 143], np.uint8)[e % 5]
    got = check(qnnp, f"equalmx/b{batch}", x, codes, e, bias)
    scales = np.ldexp(F32(1), e.astype(np.int32) - 128).astype(F32)
    op = qnnp.create_fully_connected_nc_f32_qd8_qb4w_b32(k, n, pack(W2[codes]), scales, None, bias, -INF, INF)
    assert (run(qnnp, f"equalmx/b32/b{batch}", op, x, n, kernel="qb4w_b32") == got).all()


@pytest.mark.parametrize("batch", [3, 17])
def test_strided_rows_and_offset_bases(qnnp, batch):
    name = f"layoutmx/b{batch}"
    check(qnnp, name, *problem(name, batch, 160, 33), in_extra=1, out_extra=1, in_off=12, out_off=8)


def _with(array, value):
    out = array.copy()
    out[2, 1] = value
    return out


K, N = 128, 4
KERNEL, SCALES, BIAS = np.full((N, K // 2), 0x1F, np.uint8), np.full((N, K // B), 127, np.uint8), np.zeros(N, F32)
K48 = (48, N, np.zeros((N, 24), np.uint8), SCALES[:, :1])
INV, UNS = Status.invalid_parameter, Status.unsupported_parameter


@pytest.mark.parametrize("args,want", [
    ((K, N, KERNEL, SCALES, BIAS, -INF, INF), Status.success),
    ((0, N, KERNEL, SCALES, BIAS, -INF, INF), INV),
    ((K, N, None, SCALES, BIAS, -INF, INF), INV),
    ((K, N, KERNEL, None, BIAS, -INF, INF), INV),
    ((K, N, KERNEL, _with(SCALES, 255), BIAS, -INF, INF), INV),                           # E8M0's NaN
    ((K, N, KERNEL, _with(SCALES, 110), np.array([0, NAN, 0, 0], F32), -INF, INF), INV),  # invalid before unsupported
    ((K, N, KERNEL, SCALES, BIAS, 1.0, 0.5), INV),
    (K48 + (BIAS, 1.0, 0.5), INV),
    (K48 + (BIAS, -INF, INF), UNS),                                                       # K is no multiple of 32
    ((K, N, KERNEL, _with(SCALES, 110), BIAS, -INF, INF), UNS),
    ((K, N, KERNEL, _with(SCALES, 144), BIAS, -INF, INF), UNS),
    ((K, N, KERNEL, _with(SCALES, 111), BIAS, -INF, INF), Status.success),
    ((K, N, KERNEL, _with(SCALES, 143), BIAS, -INF, INF), Status.success),
    ((32768 + 32, 1, np.zeros((1, 16400), np.uint8), np.full((1, 1025), 127, np.uint8), None, -INF, INF), UNS),
])
def test_create_refusals_in_their_order(qnnp, args, want):
    st, op = qnnp.create_fully_connected_nc_f32_qd8_mxfp4w_status(*args)
    if op:
        qnnp.delete_operator(op)
    assert st == want and bool(op) == (want == Status.success), (args[:2], args[4:], st, want)
