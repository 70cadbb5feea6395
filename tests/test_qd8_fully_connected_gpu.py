"""GPU tier of the dynamically quantized fully connected operator (hip/f32qd8rows.hip and hip/qd8f32gemm.hip behind
dynamic-fully-connected.c). No reference operator exists; the definition is bit-exact float32 and every expectation is its
numpy restatement in tests/_dynamic_fc.py. Outputs are compared as uint32 bit patterns, inside guard bytes, the fill
between strided rows included; the kernel names of both launches are asserted per case."""
import numpy as np
import pytest

import _dynamic_fc as dfc
from _gpu import Guarded
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

F32 = np.float32
INF, NAN = float("inf"), float("nan")
FILL = 0xA5A5A5A5


def _run(qnnp, op, x, n, in_extra=0, out_extra=0, in_off=0, out_off=0, what=""):
    """one setup and run of x [batch][K] on fresh guarded buffers: strides above the channel counts by *_extra elements,
    bases offset by *_off bytes. Returns y [batch][N] after checking the guards, the gaps, the input and the kernel names."""
    batch, k = x.shape
    in_stride, out_stride = k + in_extra, n + out_extra
    x_host = np.full((batch - 1) * in_stride + k, 7.25, F32)
    y_host = np.full((batch - 1) * out_stride + n, FILL, np.uint32)
    for r in range(batch):
        x_host[r * in_stride:r * in_stride + k] = x[r]
    gx, gy = Guarded(x_host, in_off), Guarded(y_host, out_off)
    assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, gx, in_stride, gy, out_stride) == Status.success, what
    qnnp.run_operator(op)
    assert qnnp.operator_kernel(op) == dfc.gemm_kernel(batch), (what, qnnp.operator_kernel(op))
    assert qnnp.dynamic_rows_kernel(op) == dfc.rows_kernel(k, batch, gx.data_ptr(), in_stride), (what, qnnp.dynamic_rows_kernel(op))
    got = gy.read().view(np.uint32)
    gy.assert_intact(what)
    gx.assert_intact(what + " (input)")
    assert np.array_equal(gx.read().view(np.uint32), x_host.view(np.uint32)), what + ": input changed"
    y = np.empty((batch, n), np.uint32)
    for r in range(batch):
        y[r] = got[r * out_stride:r * out_stride + n]
        got[r * out_stride:r * out_stride + n] = FILL
    assert np.all(got == FILL), what + ": a gap between output rows was written"
    return y


def _same(got, want, what):
    want = want.view(np.uint32)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} differ, first at {bad[:4].tolist()}: got "
                             f"{got[tuple(bad[0])]:#x}, want {want[tuple(bad[0])]:#x}")


def _check(qnnp, name, x, kernel, scales, bias, lo=-INF, hi=INF, **layout):
    n = kernel.shape[0]
    want = dfc.expected(x, kernel, scales, bias, lo, hi)
    op = qnnp.create_fully_connected_nc_f32_qd8(x.shape[1], n, kernel, scales, bias, lo, hi)
    try:
        _same(_run(qnnp, op, x, n, what=name, **layout), want, name)
    finally:
        qnnp.delete_operator(op)
    return want


# every batch, K and N with at least two values of the other two: GEMV / GEMM and one / two row tiles; the K pad and
# wave -> block; then block -> two-pass
SHAPES = [(1, 1, 1), (1, 64, 130), (3, 63, 16), (3, 1025, 33), (3, 200, 1), (16, 65, 33), (16, 1024, 1), (16, 63, 130),
          (17, 200, 130), (17, 1, 16), (17, 65, 16), (129, 64, 1), (129, 1025, 130), (129, 1024, 33),
          (2, 16384, 16), (2, 16385, 16)]


@pytest.mark.parametrize("batch,k,n", SHAPES)
def test_shape_edges_of_each_kernel(qnnp, batch, k, n):
    name = f"shape/b{batch}_k{k}_n{n}"
    _check(qnnp, name, *dfc.problem(name, batch, k, n))


@pytest.mark.parametrize("batch", [3, 17])
@pytest.mark.parametrize("layout", [dict(in_extra=5, out_extra=3), dict(in_extra=4, out_extra=16), dict(in_off=4),
                                    dict(out_off=4), dict(in_extra=1, out_extra=1, in_off=12, out_off=8)],
                         ids=lambda d: "_".join(f"{key}{value}" for key, value in d.items()))
def test_strides_and_base_alignment(qnnp, batch, layout):
    name = f"layout/b{batch}"
    _check(qnnp, name, *dfc.problem(name, batch, 200, 33), **layout)


@pytest.mark.parametrize("batch", [8, 24])
def test_row_classes(qnnp, batch):
    """all-zero, all-positive, all-negative, one NaN, +inf, denormals, +-3e38 and .5 ties (scale 2: odd values), as rows
    of one tensor; batch 24 repeats them through the tile kernel"""
    k, n = 96, 33
    _, kernel, scales, bias = dfc.problem("classes", 1, k, n)
    rng = np.random.default_rng(5)
    base = rng.standard_normal(k).astype(F32)
    rows = np.zeros((8, k), F32)
    rows[1] = np.abs(base) + F32(0.5)
    rows[2] = -np.abs(base) - F32(0.5)
    rows[3] = base
    rows[3, 17] = NAN
    rows[4] = base
    rows[4, 40] = INF
    rows[5] = (rng.integers(1, 2 ** 23, size=k).astype(np.uint32) | (rng.integers(0, 2, size=k).astype(np.uint32) << 31)).view(F32)
    rows[6] = base
    rows[6, 0], rows[6, 95] = 3e38, -3e38
    rows[7] = (2 * rng.integers(0, 255, size=k) + 1).astype(F32)
    rows[7, 0], rows[7, 1] = 0.0, 510.0
    q, scale, zp = dfc.quantize_rows(rows)
    assert scale[0] == 1 and zp[1] == 0 and zp[2] == 255 and scale[4] == 1 and scale[5] == 1 and scale[6] == 1 and scale[7] == 2
    x = np.resize(rows, (batch, k))
    _check(qnnp, f"classes/b{batch}", x, kernel, scales, bias)


@pytest.mark.parametrize("pattern", ["all_high", "both_ends", "all_low"])
def test_accumulator_bound(qnnp, pattern):
    """K = 32768, weights at 127 and -128, activations at the ends of their range: |acc| reaches 255 * 128 * 32768"""
    k, n = 32768, 16
    x = {"all_high": np.ones((1, k), F32), "all_low": -np.ones((1, k), F32),
         "both_ends": np.tile(np.array([0.0, 2.0], F32), k // 2)[None, :]}[pattern]
    kernel = np.empty((n, k), np.int8)
    kernel[0::4], kernel[1::4] = 127, -128
    kernel[2::4] = np.where(np.arange(k) % 2 == 1, 127, -128)
    kernel[3::4] = np.where(np.arange(k) % 2 == 1, -128, 127)
    scales = np.full(n, 2.0 ** -9, F32)
    want = _check(qnnp, f"bound/{pattern}", x, kernel, scales, np.arange(n, dtype=F32))
    assert np.abs(want).max() > 1000


def test_clamp_cuts_and_null_bias(qnnp):
    for batch in (3, 17):
        x, kernel, scales, bias = dfc.problem("clamp", batch, 200, 33)
        want = _check(qnnp, f"clamp/b{batch}", x, kernel, scales, bias, -0.5, 0.75)
        assert (want == F32(-0.5)).any() and (want == F32(0.75)).any() and ((want > -0.5) & (want < 0.75)).any()
        _check(qnnp, f"no bias/b{batch}", x, kernel, scales, None)


def test_create_refusals_in_their_order(qnnp):
    k, n = 8, 4
    kernel, scales, bias = np.ones((n, k), np.int8), np.full(n, 0.01, F32), np.zeros(n, F32)

    def with_(array, value):
        out = array.copy()
        out[2] = value
        return out
    inv, uns = Status.invalid_parameter, Status.unsupported_parameter
    big = 2 ** 24
    table = [
        ((k, n, kernel, scales, bias, -INF, INF), Status.success),
        ((k, n, kernel, with_(scales, 2.0 ** -20), with_(bias, 2.0 ** -126), -1.0, -1.0), Status.success),
        ((0, n, kernel, scales, bias, -INF, INF), inv),
        ((k, 0, kernel, scales, bias, -INF, INF), inv),
        ((k, n, None, scales, bias, -INF, INF), inv),
        ((k, n, kernel, None, bias, -INF, INF), inv),
        ((k, n, kernel, with_(scales, 0.0), bias, -INF, INF), inv),
        ((k, n, kernel, with_(scales, -0.01), bias, -INF, INF), inv),
        ((k, n, kernel, with_(scales, 1e-40), bias, -INF, INF), inv),
        ((k, n, kernel, with_(scales, INF), bias, -INF, INF), inv),
        ((k, n, kernel, with_(scales, NAN), bias, -INF, INF), inv),
        ((k, n, kernel, scales, with_(bias, NAN), -INF, INF), inv),
        ((k, n, kernel, scales, with_(bias, INF), -INF, INF), inv),
        ((k, n, kernel, scales, with_(bias, 1e-40), -INF, INF), inv),
        ((k, n, kernel, scales, bias, NAN, INF), inv),
        ((k, n, kernel, scales, bias, -INF, NAN), inv),
        ((k, n, kernel, scales, bias, 1.0, 0.5), inv),
        ((32769, n, kernel, with_(scales, 2.0 ** 21), bias, 1.0, 0.5), inv),          # invalid before unsupported
        ((k, n, kernel, with_(scales, 2.0 ** -21), bias, -INF, INF), uns),
        ((k, n, kernel, with_(scales, float(np.nextafter(F32(2.0 ** 20), F32(INF)))), bias, -INF, INF), uns),
        ((32769, 1, np.ones((1, 32769), np.int8), scales[:1], bias[:1], -INF, INF), uns),
        ((1, big, np.ones((big, 1), np.int8), np.full(big, 0.01, F32), None, -INF, INF), uns),
    ]
    for args, want in table:
        st, op = qnnp.create_fully_connected_nc_f32_qd8_status(*args)
        if op:
            qnnp.delete_operator(op)
        assert st == want and bool(op) == (want == Status.success), (args[:2], args[5:], st, want)


def test_setup_refusals_leave_the_previous_setup_runnable(qnnp):
    import torch
    batch, k, n = 5, 40, 24
    x, kernel, scales, bias = dfc.problem("setup", batch, k, n)
    want = dfc.expected(x, kernel, scales, bias)
    op = qnnp.create_fully_connected_nc_f32_qd8(k, n, kernel, scales, bias, -INF, INF)
    clamp = qnnp.create_clamp_nc_u8(k, 0, 255)
    d_x = torch.from_numpy(x).cuda()
    d_y = torch.zeros(batch * n, dtype=torch.float32, device="cuda")
    f, y = d_x.data_ptr(), d_y.data_ptr()
    setup = qnnp.setup_fully_connected_nc_f32_qd8_status
    inv, uns = Status.invalid_parameter, Status.unsupported_parameter
    try:
        assert qnnp.run_operator_status(op) == inv                              # before any setup
        assert setup(op, 0, None, 0, None, 0) == Status.success and qnnp.run_operator_status(op) == Status.success
        assert setup(op, batch, d_x, k, d_y, n) == Status.success
        refused = [((batch, None, k, d_y, n), inv), ((batch, d_x, k, None, n), inv),
                   ((batch, f + 2, k, d_y, n), inv), ((batch, d_x, k, y + 1, n), inv),
                   ((batch, d_x, k - 1, d_y, n), inv), ((batch, d_x, k, d_y, n - 1), inv),
                   ((batch, d_x, k, f + 4 * (batch * k - 1), n), inv), ((batch, d_x, k, d_x, n), inv),
                   ((2 ** 31, d_x, k, d_y, n), uns), ((2 ** 40, d_x, k, d_y, n), uns)]
        for args, status in refused + [(None, None)]:
            if args is not None:
                assert setup(op, *args) == status, args
            d_y.zero_()
            qnnp.run_operator(op)
            _same(d_y.cpu().numpy().view(np.uint32).reshape(batch, n), want, f"after the refused setup {args}")
        assert setup(clamp, batch, d_x, k, d_y, n) == inv and setup(None, batch, d_x, k, d_y, n) == inv
        assert qnnp.setup_clamp_nc_u8_status(op, batch, d_x, k, d_y, k) == inv
        # host tensors are staged through the device, strided output rows keeping what lies between them
        y_host = np.full((batch - 1) * (n + 3) + n, 1.5, F32)
        assert setup(op, batch, x, k, y_host, n + 3) == Status.success
        qnnp.run_operator(op)
        padded = np.pad(y_host, (0, 3)).reshape(batch, n + 3)
        _same(np.ascontiguousarray(padded[:, :n]).view(np.uint32), want, "host tensors")
        assert np.all(padded[:-1, n:] == F32(1.5))
    finally:
        qnnp.delete_operator(op)
        qnnp.delete_operator(clamp)


@pytest.mark.parametrize("batch", [4, 40])
def test_graph_capture_follows_the_input(qnnp, batch):
    """one run recorded into the library's capture (two launches), replayed twice with changed input"""
    import torch
    k, n = 200, 33
    x, kernel, scales, bias = dfc.problem("graph", batch, k, n)
    op = qnnp.create_fully_connected_nc_f32_qd8(k, n, kernel, scales, bias, -2.0, INF)
    d_x = torch.zeros(batch * k, dtype=torch.float32, device="cuda")
    d_y = torch.zeros(batch * n, dtype=torch.float32, device="cuda")
    try:
        qnnp.setup_fully_connected_nc_f32_qd8(op, batch, d_x, k, d_y, n)
        qnnp.graph_begin()
        try:
            qnnp.run_operator(op)
            assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, d_x, k, d_y, n) == Status.invalid_parameter
            assert qnnp.create_fully_connected_nc_f32_qd8_status(k, n, kernel, scales, bias, -INF, INF)[0] == Status.invalid_parameter
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
                _same(d_y.cpu().numpy().view(np.uint32).reshape(batch, n), dfc.expected(x_rep, kernel, scales, bias, -2.0, INF),
                      f"replay {rep}")
        finally:
            qnnp.graph_destroy(graph)
    finally:
        qnnp.delete_operator(op)
