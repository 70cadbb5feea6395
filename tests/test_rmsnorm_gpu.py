"""GPU tier of the normalized (residual add + RMSNorm) setups of the dynamically quantized fully connected operators
(qnnp_gfx950_setup_[grouped_]fully_connected_nc_f32_qd8_rmsnorm: hip/f32qd8rmsnormrows.hip behind dynamic-fully-connected.c).
An rmsnorm run must equal, in every bit, the same handle's plain run on an uploaded tensor holding h of tests/_rmsnorm.py, and
residual_out must hold that restatement's x. Outputs are compared as uint32 bit patterns inside guard bytes, and each case
asserts the row kernel's name."""
import numpy as np
import pytest

import _dynamic_fc as dfc
import test_qd8_mxfp4w_fully_connected_gpu as mx
from _gpu import Guarded
from _rmsnorm import rmsnorm
from qnnpack_amd import Status
from test_rmsnorm_host import fixed_row

pytestmark = pytest.mark.gpu

F32, FILL, INF, NAN, EPS = np.float32, 0xA5A5A5A5, float("inf"), float("nan"), 1e-5
INV, UNS, OK = Status.invalid_parameter, Status.unsupported_parameter, Status.success
FORMS = ("absent", "separate", "in_place", "discarded")         # the residual pair; discarded: residual_out == NULL


def rows_of(name, batch, k):
    """input and residual [batch][K] from normal(0, 3), gamma [K] of both signs with a zero"""
    rng = np.random.default_rng(sum(name.encode()) * 977 + batch * 31 + k)
    x, residual = (rng.normal(0, 3, (batch, k)).astype(F32) for _ in range(2))
    gamma = (rng.uniform(0.5, 2, k) * rng.choice([-1, 1], k)).astype(F32)
    gamma[k // 2] = 0
    return x, residual, gamma


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} differ, first at {bad[:4].tolist()}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


def strided(x, stride):
    batch, k = x.shape
    host = np.full((batch - 1) * stride + k, 7.25, F32)
    for r in range(batch):
        host[r * stride:r * stride + k] = x[r]
    return host


def kernel_name(k, x4):
    return ("f32_qd8_rmsnorm_rows_wave" if k <= 1024 else "f32_qd8_rmsnorm_rows_block") + ("_x4" if x4 else "")


def plain(qnnp, op, h, n):
    """the output bits of the handle's plain run on h"""
    gh, gy = Guarded(h), Guarded(np.full(h.shape[0] * n, FILL, np.uint32))
    assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, h.shape[0], gh, h.shape[1], gy, n) == OK
    qnnp.run_operator(op)
    assert qnnp.dynamic_rows_kernel(op) == dfc.rows_kernel(h.shape[1], h.shape[0], 0, h.shape[1])
    return gy.read().view(np.uint32)


def check(qnnp, op, n, x, residual, gamma, form, off=0, extra=0, epsilon=EPS):
    """one rmsnorm setup and run in the given residual form, bases offset by `off` bytes and strides `extra` above K: the
    output against the plain run on the restatement's h, residual_out against its x, the guards and the kernel's name"""
    batch, k = x.shape
    stride = k + extra
    h, x_sum = rmsnorm(x, gamma, epsilon, None if form == "absent" else residual)
    want = plain(qnnp, op, h, n)
    gx, gg, gy = Guarded(strided(x, stride), off), Guarded(gamma, off), Guarded(np.full(batch * n, FILL, np.uint32))
    gr = None if form == "absent" else Guarded(strided(residual, stride), off)
    go = {"separate": Guarded(np.full((batch - 1) * stride + k, FILL, np.uint32), off), "in_place": gr}.get(form)
    assert qnnp.setup_fully_connected_nc_f32_qd8_rmsnorm_status(op, batch, gx, stride, gg, epsilon, gr, go, stride, gy, n) == OK
    qnnp.run_operator(op)
    x4 = off % 16 != 0 or (batch > 1 and stride % 4 != 0)
    assert qnnp.dynamic_rows_kernel(op) == kernel_name(k, x4), (qnnp.dynamic_rows_kernel(op), form)
    same(gy.read().view(np.uint32), want, f"output, residual {form}")
    if go is not None:          # the rows hold x; what lies between them is what it was
        expect = strided(x_sum, stride).view(np.uint32)
        between = strided(np.zeros_like(x_sum), stride) != 0
        expect[between] = FILL if form == "separate" else strided(residual, stride).view(np.uint32)[between]
        same(go.read().view(np.uint32), expect, f"residual_out, {form}")
    for g in (gx, gg, gy, gr, go):
        if g is not None:
            g.assert_intact(form)


def int8_handle(qnnp, name, k, n=17):
    _, kernel, scales, bias = dfc.problem(name, 1, k, n)
    return qnnp.create_fully_connected_nc_f32_qd8(k, n, kernel, scales, bias, -INF, INF)


# a cut piece with 63 idle lanes; the full wave; the first block shape (65 pieces: the wave-pairing steps meet zeros); the
# flagship width; an odd K (five rows at stride K are the _x4 flavour); four pieces in every lane
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("k", [1, 1024, 1040, 2880, 4097, 16384])
def test_rows_and_widths_in_every_residual_form(qnnp, k, batch):
    name = f"rmsnorm/k{k}_b{batch}"
    op = int8_handle(qnnp, name, k)
    try:
        for form in FORMS:
            check(qnnp, op, 17, *rows_of(name, batch, k), form)
    finally:
        qnnp.delete_operator(op)


@pytest.mark.parametrize("k,layout", [(80, dict(off=4)), (1040, dict(off=4)), (1040, dict(extra=2)), (80, dict(extra=1))])
def test_unaligned_bases_and_strides_take_the_dword_kernels(qnnp, k, layout):
    op = int8_handle(qnnp, "rmsnormalign", k)
    try:
        for form in ("absent", "separate", "in_place"):
            check(qnnp, op, 17, *rows_of("rmsnormalign", 3, k), form, **layout)
    finally:
        qnnp.delete_operator(op)


def test_special_rows_and_the_order_of_the_sum(qnnp):
    """NaN, +-inf, denormals (beside a zero residual: flushed before and behind the add), an all-zero row, a row whose S
    overflows; and the fixed row whose sequential sum differs from the tree's, at an epsilon that lets the difference through"""
    k = 48
    x, residual, gamma = rows_of("rmsnormspecial", 6, k)
    den = F32(2.0 ** -140)
    x[0, 5], x[1, 5], x[1, 6], x[3], x[4] = NAN, INF, -INF, 0, 3e19
    x[2, :6], residual[2, :6] = [den, -den, 2.0 ** -126, -2.0 ** -126, 2.0 ** -127, 1.0], [0, 0, -1.5 * 2.0 ** -126, den, 1.0, -1.0]
    residual[3] = 0
    op = int8_handle(qnnp, "rmsnormspecial", k)
    narrow = int8_handle(qnnp, "rmsnormorder", 32)
    try:
        for form in FORMS:
            check(qnnp, op, 17, x, residual, gamma, form)
        row = np.repeat(fixed_row(), 2, axis=0)
        check(qnnp, narrow, 17, row, np.zeros_like(row), np.linspace(1, 2, 32).astype(F32), "absent", epsilon=2.0 ** -30)
    finally:
        qnnp.delete_operator(op)
        qnnp.delete_operator(narrow)


def nibbles(rng, n, k):
    return rng.integers(0, 256, (n, k // 2), dtype=np.uint8)


@pytest.mark.parametrize("fmt", ["qc4w", "qb4w", "qb4w_zp", "qb4w_b32", "mxfp4w"])
def test_the_other_creates(qnnp, fmt):
    batch, k, n, blk = 3, 2880, 32, 64
    rng = np.random.default_rng(len(fmt))
    bias = rng.standard_normal(n).astype(F32)

    def scales(per):
        return rng.uniform(0.002, 0.05, (n, per)).astype(F32)
    if fmt == "qc4w":
        op = qnnp.create_fully_connected_nc_f32_qd8_qc4w(k, n, nibbles(rng, n, k), scales(1), bias, -INF, INF)
    elif fmt == "qb4w":
        op = qnnp.create_fully_connected_nc_f32_qd8_qb4w(k, n, blk, nibbles(rng, n, k), scales(k // blk), bias, -INF, INF)
    elif fmt == "qb4w_zp":
        op = qnnp.create_fully_connected_nc_f32_qd8_qb4w_zp(k, n, blk, nibbles(rng, n, k), scales(k // blk),
                                                            rng.integers(0, 16, (n, k // blk), dtype=np.uint8), bias, -INF, INF)
    elif fmt == "qb4w_b32":
        op = qnnp.create_fully_connected_nc_f32_qd8_qb4w_b32(k, n, nibbles(rng, n, k), scales(k // 32), None, bias, -INF, INF)
    else:
        op = qnnp.create_fully_connected_nc_f32_qd8_mxfp4w(k, n, nibbles(rng, n, k), rng.integers(117, 124, (n, k // 32)).astype(np.uint8),
                                                           bias, -INF, INF)
    try:
        check(qnnp, op, n, *rows_of("rmsnorm" + fmt, batch, k), "in_place")
        assert qnnp.operator_kernel(op).startswith(f"qd8_f32_{fmt}_")
    finally:
        qnnp.delete_operator(op)


def test_grouped_gamma_overwritten_between_runs_and_replays(qnnp):
    """the grouped handle, two assignments and one skipped id, against its plain run on h; then gamma overwritten on the device
    between two eager runs and between replays of one captured graph"""
    import torch
    groups, batch, a, k, n = 3, 3, 2, 2880, 32
    rng = np.random.default_rng(5)
    x, residual, gamma = rows_of("rmsnormgrouped", batch, k)
    gammas = [gamma, (gamma * F32(-1.75)).astype(F32)]
    ids = np.array([0, 2, -1, 1, 1, 0], np.int32)
    fill = np.full(batch * a * n, FILL, np.uint32)
    op = qnnp.create_grouped_fully_connected_nc_f32_qd8_mxfp4w(
        groups, k, n, rng.integers(0, 256, (groups, n, k // 2), dtype=np.uint8),
        rng.integers(117, 124, (groups, n, k // 32)).astype(np.uint8), None, -INF, INF)
    gx, gr, gg, gi, gy = Guarded(x), Guarded(residual), Guarded(gamma), Guarded(ids), Guarded(fill)
    gro = Guarded(np.zeros(batch * k, np.uint32))
    graph = None

    def output(launch, g):
        gg.view.copy_(torch.from_numpy(g.view(np.uint8)))
        gy.view.copy_(torch.from_numpy(fill.view(np.uint8)))
        torch.cuda.synchronize()
        launch()
        return gy.read().view(np.uint32).reshape(batch * a, n)
    try:
        want = []
        for g in gammas:
            gh = Guarded(rmsnorm(x, g, EPS, residual)[0])
            assert qnnp.setup_grouped_fully_connected_nc_f32_qd8_status(op, batch, a, gh, k, gi, gy, n) == OK
            want.append(output(lambda: qnnp.run_operator(op), g))
        assert (want[0][2] == FILL).all() and (np.delete(want[0], 2, axis=0) != FILL).all() and (want[0] != want[1]).any()
        assert qnnp.setup_grouped_fully_connected_nc_f32_qd8_rmsnorm_status(op, batch, a, gx, k, gg, EPS, gr, gro, k, gi, gy, n) == OK
        for g, w in zip(gammas, want):
            same(output(lambda: qnnp.run_operator(op), g), w, "eager")
        assert qnnp.dynamic_rows_kernel(op) == "f32_qd8_rmsnorm_rows_block"
        same(gro.read().view(np.uint32), rmsnorm(x, gamma, EPS, residual)[1].view(np.uint32).reshape(-1), "residual_out")
        qnnp.graph_begin()
        try:
            qnnp.run_operator(op)
        finally:
            graph = qnnp.graph_end()

        def replay():
            qnnp.graph_launch(graph)
            qnnp.graph_synchronize(graph)
        for g, w in list(zip(gammas, want))[::-1] * 2:
            same(output(replay, g), w, "replay")
    finally:
        if graph is not None:
            qnnp.graph_destroy(graph)
        qnnp.delete_operator(op)
    for g in (gx, gr, gg, gi, gy, gro):
        g.assert_intact("grouped")


def test_statuses_in_their_order_and_what_a_refusal_leaves(qnnp):
    batch, k, n = 3, 96, 32
    x, residual, gamma = rows_of("rmsnormsetup", batch, k)
    h = rmsnorm(x, gamma, EPS, residual)[0]
    _, codes, e, bias = mx.problem("rmsnormsetup", batch, k, n)
    gx, gr, gg, gh, gy = Guarded(x), Guarded(residual), Guarded(gamma), Guarded(h), Guarded(np.full(batch * n, FILL, np.uint32))
    gi, spare = Guarded(np.array([0, 1, 0], np.int32)), Guarded(np.zeros(batch * k, F32))
    op = qnnp.create_fully_connected_nc_f32_qd8_mxfp4w(k, n, mx.pack(codes), e, bias, -INF, INF)
    grouped = qnnp.create_grouped_fully_connected_nc_f32_qd8_mxfp4w(2, k, n, np.stack([mx.pack(codes)] * 2), np.stack([e] * 2), None, -INF, INF)
    wide = int8_handle(qnnp, "rmsnormwide", 16416, 1)
    setup, setup_grouped = qnnp.setup_fully_connected_nc_f32_qd8_rmsnorm_status, qnnp.setup_grouped_fully_connected_nc_f32_qd8_rmsnorm_status

    def both(want, x=gx, stride=k, g=gg, eps=EPS, r=gr, ro=spare, rs=k, y=gy, b=batch):
        assert setup(op, b, x, stride, g, eps, r, ro, rs, y, n) == want
        assert setup_grouped(grouped, b, 1, x, stride, g, eps, r, ro, rs, gi, y, n) == want
    try:
        assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, gh, k, gy, n) == OK
        qnnp.run_operator(op)
        want = gy.read().view(np.uint32)
        assert qnnp.setup_grouped_fully_connected_nc_f32_qd8_status(grouped, batch, 1, gh, k, gi, gy, n) == OK
        assert setup(grouped, batch, gx, k, gg, EPS, gr, spare, k, gy, n) == INV              # each refuses the other's handles
        assert setup_grouped(op, batch, 1, gx, k, gg, EPS, gr, spare, k, gi, gy, n) == INV
        assert setup(wide, batch, None, 0, None, NAN, None, None, 0, None, 0) == UNS          # from the handle alone
        both(INV, g=None)
        both(INV, r=None)                                                                     # a residual_out without a residual
        for name in ("g", "r", "ro"):
            both(INV, **{name: spare.data_ptr() + 2})
        for eps in (0.0, NAN, INF, -EPS, 2.0 ** -41, 1.0 + 2.0 ** -20, 1e-42):
            both(INV, eps=eps)
        both(INV, eps=NAN, b=2 ** 31)                          # epsilon is looked at in front of the strides and the limits
        both(INV, rs=k - 1)
        assert setup(op, 2 ** 31, gx, k, gg, EPS, gr, spare, k, gy, n) == UNS
        both(INV, y=gg), both(INV, y=gr), both(INV, y=spare)                                  # the output shares no byte with another tensor
        both(INV, ro=gx), both(INV, ro=gg), both(INV, ro=gr.data_ptr() + 4)                   # residual_out: in place or disjoint
        assert setup_grouped(grouped, batch, 1, gx, k, gg, EPS, gr, gi, k, gi, gy, n) == INV
        both(INV, g=gamma), both(INV, x=x), both(INV, r=residual)                             # host memory: nothing here is staged
        gy.view.copy_(gy.view * 0)
        qnnp.run_operator(op)                                   # the plain setup before the refusals still stands
        assert qnnp.dynamic_rows_kernel(op) == "f32_qd8_rows_wave"
        same(gy.read().view(np.uint32), want, "after the refusals")
        for eps in (2.0 ** -40, 1.0):                                                         # the ends of the range are inside
            both(OK, eps=eps)
        both(OK, ro=gr, r=gr, x=spare), both(OK, b=0)
        both(OK, ro=None)
        both(INV, eps=0.0)
        qnnp.run_operator(op)
        assert qnnp.dynamic_rows_kernel(op) == "f32_qd8_rmsnorm_rows_wave"
        same(gy.read().view(np.uint32), want, "rmsnorm after plain, and after a refusal")
        assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, gh, k, gy, n) == OK
        qnnp.run_operator(op)
        assert qnnp.dynamic_rows_kernel(op) == "f32_qd8_rows_wave"
        same(gy.read().view(np.uint32), want, "plain after rmsnorm")
    finally:
        for handle in (op, grouped, wide):
            qnnp.delete_operator(handle)
