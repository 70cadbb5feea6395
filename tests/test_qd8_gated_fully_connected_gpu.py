"""GPU tier of the gated (SwiGLU) setups of the dynamically quantized fully connected operators
(qnnp_gfx950_setup_[grouped_]fully_connected_nc_f32_qd8_gated: hip/f32qd8gatedrows.hip behind dynamic-fully-connected.c).
A gated run on rows of {gate, up} pairs must equal, in every bit, the same handle's plain run on an uploaded tensor holding
h = act(gate) * up of tests/_gated.py, and for the int8 create also tests/_dynamic_fc.expected(h). Outputs are compared as
uint32 bit patterns inside guard bytes, and each case asserts the row kernel's name."""
import numpy as np
import pytest

import _dynamic_fc as dfc
import test_qd8_mxfp4w_fully_connected_gpu as mx
from _gated import gated
from _gpu import Guarded
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

F32, FILL, INF, NAN = np.float32, 0xA5A5A5A5, float("inf"), float("nan")
SILU, CLAMPED = (1.0, INF, 0.0), (1.702, 7.0, 1.0)
INV, OK = Status.invalid_parameter, Status.success


def pairs(name, batch, k):
    """x [batch][2 K] from normal(0, 4): the clamps at +-7 are hit; a few elements at +-100 reach y = -80"""
    rng = np.random.default_rng(sum(name.encode()) * 977 + batch * 31 + k)
    x = rng.normal(0, 4, (batch, 2 * k)).astype(F32)
    x[:, :4] = np.array([100, -100, -100, 100], F32)[:min(4, 2 * k)]
    return x


def rows_kernel(k, batch, address, stride, gate):
    name = dfc.rows_kernel(k, batch, address, stride)
    return name.replace("f32_qd8_rows", "f32_qd8_gated_rows") if gate else name


def run(qnnp, op, x, k, n, gate, in_extra=0, in_off=0):
    """one gated (gate = the three parameters) or plain (gate = None) setup and run of `op` on x [batch][width]; returns the
    output bits [batch][n] after checking the guards and the row kernel's name"""
    batch, width = x.shape
    stride = width + in_extra
    x_host = np.full((batch - 1) * stride + width, 7.25, F32)
    for r in range(batch):
        x_host[r * stride:r * stride + width] = x[r]
    gx, gy = Guarded(x_host, in_off), Guarded(np.full(batch * n, FILL, np.uint32))
    if gate:
        assert qnnp.setup_fully_connected_nc_f32_qd8_gated_status(op, batch, gx, stride, *gate, gy, n) == OK
    else:
        assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, gx, stride, gy, n) == OK
    qnnp.run_operator(op)
    want = rows_kernel(k, batch, gx.data_ptr(), stride, gate)
    assert qnnp.dynamic_rows_kernel(op) == want, (qnnp.dynamic_rows_kernel(op), want)
    got = gy.read().view(np.uint32).reshape(batch, n)
    gx.assert_intact("input")
    gy.assert_intact("output")
    return got


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} differ, first at {bad[:4].tolist()}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


def check_int8(qnnp, name, x, gate, **layout):
    """the int8 create with N = 17: gated run == expected(h) == plain run on h"""
    k, n = x.shape[1] // 2, 17
    _, kernel, scales, bias = dfc.problem(name, 1, k, n)
    h = gated(x, *gate)
    op = qnnp.create_fully_connected_nc_f32_qd8(k, n, kernel, scales, bias, -INF, INF)
    try:
        got = run(qnnp, op, x, k, n, gate, **layout)
        same(got, dfc.expected(h, kernel, scales, bias).view(np.uint32), name)
        same(got, run(qnnp, op, h, k, n, None), name + " (plain run on h)")
    finally:
        qnnp.delete_operator(op)


# cut piece and pad stores; wave -> block; block -> twopass; the largest K. Five rows leave the wave kernel's last workgroup partly empty
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("k", [1, 15, 16, 17, 63, 64, 1024, 1040, 16384, 16416, 32768])
def test_row_kernel_edges(qnnp, k, batch):
    name = f"gated/k{k}_b{batch}"
    check_int8(qnnp, name, pairs(name, batch, k), CLAMPED)


@pytest.mark.parametrize("k", [80, 1040])
@pytest.mark.parametrize("batch,layout,x4", [(3, dict(in_off=4), True), (3, dict(in_extra=1), True), (1, dict(in_extra=1), False)],
                         ids=["base4", "stride_odd", "one_row_stride_odd"])
def test_alignment(qnnp, k, batch, layout, x4):
    name = f"gatedalign/k{k}_b{batch}"
    check_int8(qnnp, name, pairs(name, batch, k), CLAMPED, **layout)       # run() asserts the name by the plain rule ...
    assert dfc.rows_kernel(k, batch, layout.get("in_off", 0), 2 * k + layout.get("in_extra", 0)).endswith("_x4") == x4     # ... which says this


@pytest.mark.parametrize("gate", [SILU, CLAMPED], ids=["silu", "clamped"])
def test_both_parameter_sets(qnnp, gate):
    x = pairs("gatedsets", 3, 80)
    h = gated(x, *gate)
    assert np.isfinite(h).all() and (x[:, 0::2] > 7).any() and (x[:, 1::2] < -7).any() and (x[:, 1::2] > 7).any()
    check_int8(qnnp, "gatedsets", x, gate)


def test_special_values(qnnp):
    """NaN, +-inf, denormals and +-0 in gate and in up positions of one row"""
    x = pairs("gatedspecial", 1, 80)
    den = F32(2.0 ** -140)
    specials = [NAN, INF, -INF, den, -den, 0.0, -0.0, F32(2.0 ** -125)]      # the last: a = 2^-126 exactly, flushed
    for i, v in enumerate(specials):
        x[0, 2 * (3 + i)] = v                    # as a gate, beside a random up
        x[0, 2 * (20 + i) + 1] = v               # as an up value, beside a random gate
    x[0, 80:84] = [NAN, NAN, -INF, 0.0]          # both NaN; -inf * 0
    for gate in (SILU, CLAMPED):
        h = gated(x, *gate)
        assert np.isnan(h).sum() >= 3 and np.isinf(h).any()
        check_int8(qnnp, "gatedspecial", x, gate)


@pytest.mark.parametrize("batch", [3, 20])
@pytest.mark.parametrize("fmt", ["qb4w_b32", "mxfp4w"])
def test_formats(qnnp, fmt, batch):
    k, n = 96, 32
    _, codes, e, bias = mx.problem("gated" + fmt, batch, k, n)
    if fmt == "mxfp4w":
        op = qnnp.create_fully_connected_nc_f32_qd8_mxfp4w(k, n, mx.pack(codes), e, bias, -INF, INF)
    else:
        scales = np.ldexp(F32(1), e.astype(np.int32) - 127).astype(F32)
        op = qnnp.create_fully_connected_nc_f32_qd8_qb4w_b32(k, n, mx.pack(codes), scales, None, bias, -INF, INF)
    x = pairs("gated" + fmt, batch, k)
    try:
        got = run(qnnp, op, x, k, n, CLAMPED)
        same(got, run(qnnp, op, gated(x, *CLAMPED), k, n, None), fmt)
        assert qnnp.operator_kernel(op).startswith(f"qd8_f32_{fmt}_") and (got != FILL).all()
    finally:
        qnnp.delete_operator(op)


@pytest.mark.parametrize("batch,a", [(10, 1), (5, 2)])
def test_grouped(qnnp, batch, a):
    """the gated grouped run against the plain grouped run on h, skipped rows' fill included; then the ids overwritten on the
    device under a captured graph, two replays"""
    import torch
    groups, k, n, rows = 4, 96, 32, batch * a
    sets = [mx.problem(f"gatedgrp/g{g}", 1, k, n)[1:] for g in range(groups)]
    codes, e, bias = (np.stack([s[i] for s in sets]) for i in range(3))
    x = pairs("gatedgrp", batch, k)
    routings = [np.array([0, 3, -1, 1, groups, 2, 1, 1, 0, 3], np.int32), np.array([2, 2, 0, groups, 1, 3, -1, 0, 1, 2], np.int32)]
    fill = np.full(rows * n, FILL, np.uint32)
    gx, gh, gi, gy = Guarded(x), Guarded(gated(x, *CLAMPED)), Guarded(routings[0]), Guarded(fill)
    op = qnnp.create_grouped_fully_connected_nc_f32_qd8_mxfp4w(groups, k, n, np.stack([mx.pack(c) for c in codes]), e, bias, -INF, INF)
    graph = None

    def output(launch, ids):
        gi.view.copy_(torch.from_numpy(ids.view(np.uint8)))
        gy.view.copy_(torch.from_numpy(fill.view(np.uint8)))
        torch.cuda.synchronize()
        launch()
        return gy.read().view(np.uint32).reshape(rows, n)
    try:
        assert qnnp.setup_grouped_fully_connected_nc_f32_qd8_status(op, batch, a, gh, k, gi, gy, n) == OK
        plain = [output(lambda: qnnp.run_operator(op), ids) for ids in routings]
        assert qnnp.dynamic_rows_kernel(op) == "f32_qd8_rows_wave"
        assert qnnp.setup_grouped_fully_connected_nc_f32_qd8_gated_status(op, batch, a, gx, 2 * k, *CLAMPED, gi, gy, n) == OK
        same(output(lambda: qnnp.run_operator(op), routings[0]), plain[0], "eager")
        assert qnnp.dynamic_rows_kernel(op) == "f32_qd8_gated_rows_wave"
        qnnp.graph_begin()
        try:
            qnnp.run_operator(op)
        finally:
            graph = qnnp.graph_end()

        def replay():
            qnnp.graph_launch(graph)
            qnnp.graph_synchronize(graph)
        for ids, want in list(zip(routings, plain))[::-1] * 2:
            same(output(replay, ids), want, "replay")
        skipped = (routings[0] < 0) | (routings[0] >= groups)
        assert (plain[0][skipped] == FILL).all() and (plain[0][~skipped] != FILL).all() and (plain[0] != plain[1]).any()
    finally:
        if graph is not None:
            qnnp.graph_destroy(graph)
        qnnp.delete_operator(op)
    for g in (gx, gh, gi, gy):
        g.assert_intact("grouped")


def test_setup_behaviour(qnnp):
    """the refusals of both setups in their order; a refused gated setup leaves the plain one runnable; a plain setup after a
    gated one runs the plain row kernel"""
    batch, k, n, groups = 3, 96, 32, 2
    x = pairs("gatedsetup", batch, k)
    h = gated(x, *SILU)
    _, codes, e, bias = mx.problem("gatedsetup", batch, k, n)
    gx, gh, gy = Guarded(x), Guarded(h), Guarded(np.full(batch * n, FILL, np.uint32))
    gi = Guarded(np.array([0, 1, 0], np.int32))
    op = qnnp.create_fully_connected_nc_f32_qd8_mxfp4w(k, n, mx.pack(codes), e, bias, -INF, INF)
    grouped = qnnp.create_grouped_fully_connected_nc_f32_qd8_mxfp4w(groups, k, n, np.stack([mx.pack(codes)] * groups),
                                                                    np.stack([e] * groups), None, -INF, INF)
    setup, setup_grouped = qnnp.setup_fully_connected_nc_f32_qd8_gated_status, qnnp.setup_grouped_fully_connected_nc_f32_qd8_gated_status
    bad = [(0.0, INF, 0.0), (NAN, INF, 0.0), (2.0 ** -7, INF, 0.0), (128.0, INF, 0.0), (-1.0, INF, 0.0),       # alpha
           (1.0, NAN, 0.0), (1.0, 2.0 ** -7, 0.0), (1.0, 65.0, 0.0), (1.0, -INF, 0.0), (1.0, -7.0, 0.0),         # limit
           (1.0, INF, NAN), (1.0, INF, INF), (1.0, INF, 1e-40), (1.0, INF, -65.0)]                               # up_shift
    try:
        assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, gh, k, gy, n) == OK
        qnnp.run_operator(op)
        want = gy.read().view(np.uint32)
        assert qnnp.setup_grouped_fully_connected_nc_f32_qd8_status(grouped, batch, 1, gh, k, gi, gy, n) == OK
        for gate in bad:
            assert setup(op, batch, gx, 2 * k, *gate, gy, n) == INV, gate
            assert setup_grouped(grouped, batch, 1, gx, 2 * k, *gate, gi, gy, n) == INV, gate
        for gate in [(2.0 ** -6, 2.0 ** -6, -64.0), (64.0, 64.0, 2.0 ** -126)]:                 # the ends of the ranges are inside
            assert setup(op, batch, gx, 2 * k, *gate, gy, n) == OK, gate
        assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, gh, k, gy, n) == OK
        assert setup(op, batch, gx, 2 * k - 1, *SILU, gy, n) == INV and setup_grouped(grouped, batch, 1, gx, 2 * k - 1, *SILU, gi, gy, n) == INV
        last = gx.data_ptr() + 4 * (batch * 2 * k - 1)
        assert setup(op, batch, gx, 2 * k, *SILU, last, n) == INV, "the overlap check sees all 2 K floats of the last row"
        assert setup(grouped, batch, gx, 2 * k, *SILU, gy, n) == INV and setup_grouped(op, batch, 1, gx, 2 * k, *SILU, gi, gy, n) == INV
        gy.view.copy_(gy.view * 0)
        qnnp.run_operator(op)                           # the plain setup before the refusals still stands
        assert qnnp.dynamic_rows_kernel(op) == "f32_qd8_rows_wave"
        same(gy.read().view(np.uint32), want, "after the refusals")
        assert setup(op, batch, gx, 2 * k, *SILU, gy, n) == OK
        qnnp.run_operator(op)
        assert qnnp.dynamic_rows_kernel(op) == "f32_qd8_gated_rows_wave"
        same(gy.read().view(np.uint32), want, "gated")
        assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, gh, k, gy, n) == OK
        qnnp.run_operator(op)
        assert qnnp.dynamic_rows_kernel(op) == "f32_qd8_rows_wave"
        same(gy.read().view(np.uint32), want, "plain after gated")
    finally:
        qnnp.delete_operator(op)
        qnnp.delete_operator(grouped)
