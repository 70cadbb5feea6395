"""GPU tier of the top-k softmax router and the weighted combine (include/qnnpack_gfx950_moe.h: hip/f32topk.hip and
hip/f32combine.hip behind moe.c) against their numpy restatement (tests/_moe.py). Ids, weights and outputs are compared as
bit patterns inside guard bytes, and the kernel's name is asserted per case from the header's rule."""
import numpy as np
import pytest

import _moe as moe
import test_qd8_grouped_mxfp4w_fully_connected_gpu as grp
from _gpu import Guarded
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

F32, U32, FILL, INF, NAN, DEN = np.float32, np.uint32, grp.FILL, float("inf"), float("nan"), 2.0 ** -140
INV, UNS, OK = Status.invalid_parameter, Status.unsupported_parameter, Status.success
INT32_MIN = -2 ** 31


def same(got, want, name):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{name}: {len(bad)} of {want.size} differ, first at {bad[:4].tolist()}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


def strided(rows, stride, gap=7.25):
    flat = np.full((len(rows) - 1) * stride + rows.shape[1], gap, rows.dtype)
    for r, row in enumerate(rows):
        flat[r * stride:r * stride + len(row)] = row
    return flat


# ---- the router ----
def topk_kernel(e, vec):
    l, v = next((l, v) for bound, l, v in [(32, 8, 4), (64, 16, 4), (128, 32, 4), (256, 64, 4), (512, 64, 8), (1024, 64, 16)] if e <= bound)
    return f"f32_topk_l{l}_v{v}" + ("" if vec else "_x4")


def check_router(qnnp, name, logits, a, first_group=0, extra=0, offset=0):
    tokens, e = logits.shape
    gl = Guarded(strided(logits, e + extra), offset)
    gi, gw = Guarded(np.full(tokens * a, FILL, U32)), Guarded(np.full(tokens * a, FILL, U32))
    op = qnnp.create_topk_router_nc_f32(e, a, first_group)
    try:
        assert qnnp.setup_topk_router_nc_f32_status(op, tokens, gl, e + extra, gi, gw) == OK
        qnnp.run_operator(op)
        vec = offset % 16 == 0 and (tokens == 1 or (e + extra) % 4 == 0)
        assert qnnp.operator_kernel(op) == topk_kernel(e, vec), (name, qnnp.operator_kernel(op))
    finally:
        qnnp.delete_operator(op)
    ids, w = moe.router(logits, a, first_group)
    same(gi.read().view(np.int32).reshape(tokens, a), ids, name + " ids")
    same(gw.read().view(U32).reshape(tokens, a), w.view(U32), name + " weights")
    for g in (gl, gi, gw):
        g.assert_intact(name)
    return ids, w


def logits_for(e, tokens):
    """normal logits; every other row in steps of 1 / 2, so that keys tie"""
    x = np.random.default_rng(100 * e + tokens).normal(0, 3, (tokens, e)).astype(F32)
    x[1::2] = np.rint(x[1::2] * 2) / 2
    return x


@pytest.mark.parametrize("e,a,tokens", [(1, 1, 1), (32, 4, 5), (65, 8, 3), (128, 8, 67), (1024, 8, 2), (8, 8, 9), (200, 3, 6)])
@pytest.mark.parametrize("first_group", [0, 3])
def test_router_shapes(qnnp, e, a, tokens, first_group):
    ids, _ = check_router(qnnp, f"router/e{e}_a{a}_t{tokens}", logits_for(e, tokens), a, first_group)
    assert first_group == 0 or a < e or (ids < 0).any()


def test_router_strided_rows_at_an_offset_base(qnnp):
    check_router(qnnp, "router/layout", logits_for(65, 5), 8, extra=3, offset=12)
    check_router(qnnp, "router/stride", logits_for(300, 3), 2, extra=1)


def test_router_special_rows(qnnp):
    x = np.zeros((5, 32), F32)
    x[0] = 1.25                                                          # all equal: ids 0 .. A - 1, equal weights
    x[1] = np.resize(np.array([NAN, INF, -INF, 0.0, -0.0, DEN, -DEN, 1.0, -1.0], F32), 32)
    x[2] = np.arange(32) * -45.0                                         # l_a - m < -80 from the third on
    x[3] = NAN
    x[4], x[4, 7] = -3e38, 3e38                                          # d overflows to -inf
    ids, w = check_router(qnnp, "router/special", x, 4)
    assert ids[0].tolist() == [0, 1, 2, 3] and (w[0] == F32(0.25)).all()
    assert ids[1].tolist() == [1, 10, 19, 28] and ids[3].tolist() == [0, 1, 2, 3] and ids[4].tolist() == [7, 0, 1, 2]
    assert w[2, 3] == w[2, 2] > 0 and not np.isnan(w).any()
    check_router(qnnp, "router/zeros", np.resize(np.array([-0.0, 0.0, -DEN, DEN], F32), (2, 8)), 8)


def test_router_refusals_in_their_order(qnnp):
    create, setup = qnnp.create_topk_router_nc_f32_status, qnnp.setup_topk_router_nc_f32_status
    for args, want in [((0, 1), INV), ((4, 0), INV), ((4, 5), INV), ((4, 9), INV), ((1025, 1), UNS), ((16, 9), UNS),
                       ((4, 2, 2 ** 31), UNS), ((1024, 8, 2 ** 31 - 1), OK)]:
        st, op = create(*args)
        if op:
            qnnp.delete_operator(op)
        assert st == want and bool(op) == (want == OK), (args, st)
    x = logits_for(32, 3)
    gl, gi, gw = Guarded(x), Guarded(np.full(24, FILL, U32)), Guarded(np.full(12, FILL, U32))
    op, other = qnnp.create_topk_router_nc_f32(32, 4), qnnp.create_weighted_combine_nc_f32(8, 4, 4)
    try:
        assert setup(op, 3, gl, 32, gi, gw) == OK
        i = gi.data_ptr()
        for what, args, want in [
            ("NULL weights", (op, 3, gl, 32, gi, None), INV), ("misaligned ids", (op, 3, gl, 32, i + 2, gw), INV),
            ("stride", (op, 3, gl, 31, gi, gw), INV), ("T A = 2^20", (op, 2 ** 18, gl, 32, gi, gw), UNS),
            ("weights inside the ids", (op, 3, gl, 32, gi, i + 44), INV), ("host logits", (op, 3, x, 32, gi, gw), INV),
            ("a combine handle", (other, 3, gl, 32, gi, gw), INV),
        ]:
            assert setup(*args) == want, what
        qnnp.graph_begin()
        try:
            assert setup(op, 3, gl, 32, gi, gw) == INV, "inside a capture"
        finally:
            qnnp.graph_destroy(qnnp.graph_end())
        qnnp.run_operator(op)                        # the setup before the refusals still stands
        same(gi.read().view(np.int32)[:12].reshape(3, 4), moe.router(x, 4)[0], "after the refusals")
        assert setup(op, 0, None, 0, None, None) == OK
    finally:
        qnnp.delete_operator(op)
        qnnp.delete_operator(other)


# ---- the combine ----
def routing(tokens, a, groups, seed):
    """ids with -1, `groups` and INT32_MIN sprinkled in; every row of token 1 skipped"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, groups, tokens * a).astype(np.int32)
    ids[1::3] = np.array([-1, groups, INT32_MIN, 0], np.int32)[np.arange(len(ids[1::3])) % 4]
    ids[a:2 * a] = -1
    return ids, rng.uniform(0.05, 1, tokens * a).astype(F32)


def check_combine(qnnp, name, x, routings, a, groups, graph=False, in_extra=0, out_extra=0, in_off=0, out_off=0):
    """ONE setup, then one run (or two replays of one captured graph) per (ids, weights), overwritten on the device in between"""
    import torch
    rows, n = x.shape
    tokens = rows // a
    gx = Guarded(strided(x, n + in_extra, NAN), in_off)
    gy, gi, gw = Guarded(np.full((tokens - 1) * (n + out_extra) + n, FILL, U32), out_off), Guarded(routings[0][0]), Guarded(routings[0][1])
    cells = (np.arange(tokens)[:, None] * (n + out_extra) + np.arange(n)).ravel()
    op, handle = qnnp.create_weighted_combine_nc_f32(n, a, groups), None
    try:
        assert qnnp.setup_weighted_combine_nc_f32_status(op, tokens, gx, n + in_extra, gw, gi, gy, n + out_extra) == OK
        if graph:
            qnnp.graph_begin()
            try:
                qnnp.run_operator(op)
            finally:
                handle = qnnp.graph_end()
        for k, (ids, w) in enumerate(routings):
            skipped = np.repeat((ids < 0) | (ids >= groups), n).reshape(rows, n)
            want = moe.combine(np.where(skipped, F32(NAN), x), w, ids, a, groups)
            assert not np.isnan(want).any()
            for _ in range(2 if graph else 1):
                gi.view.copy_(torch.from_numpy(ids.view(np.uint8)))
                gw.view.copy_(torch.from_numpy(w.view(np.uint8)))
                gy.view.fill_(0xA5)
                torch.cuda.synchronize()
                if graph:
                    qnnp.graph_launch(handle)
                    qnnp.graph_synchronize(handle)
                else:
                    qnnp.run_operator(op)
                got = gy.read().view(U32)
                assert np.all(np.delete(got, cells) == 0xA5A5A5A5), name + ": a gap between output rows was written"
                same(got[cells].reshape(tokens, n), want.view(U32), f"{name} [{k}]")
        vec = in_off % 16 == 0 and out_off % 16 == 0 and (rows == 1 or (n + in_extra) % 4 == 0) and (tokens == 1 or (n + out_extra) % 4 == 0)
        assert qnnp.operator_kernel(op) == ("f32_combine_wave" if n <= 256 else "f32_combine_block") + ("" if vec else "_x4")
    finally:
        if handle is not None:
            qnnp.graph_destroy(handle)
        qnnp.delete_operator(op)
    for g in (gx, gy, gi, gw):
        g.assert_intact(name)
    return want


def rows_for(tokens, a, n, ids=None, groups=4):
    """expert rows over a wide range of exponents; the rows that `ids` skips hold NaN patterns"""
    rng = np.random.default_rng(tokens * 1000 + n)
    x = (rng.normal(0, 1, (tokens * a, n)) * 2.0 ** rng.integers(-20, 20, (tokens * a, n))).astype(F32)
    if ids is not None:
        x[(ids < 0) | (ids >= groups)] = np.array([0x7FC00001, 0xFFFFFFFF], U32).view(F32)[np.arange(n) % 2]
    return x


@pytest.mark.parametrize("tokens,a,n", [(1, 1, 1), (5, 2, 33), (3, 8, 260), (70, 4, 130), (4, 4, 128), (2, 3, 1028)])
def test_combine_shapes_and_skipped_rows(qnnp, tokens, a, n):
    ids, w = routing(tokens, a, 4, n) if tokens > 1 else (np.zeros(1, np.int32), np.ones(1, F32))
    want = check_combine(qnnp, f"combine/t{tokens}_a{a}_n{n}", rows_for(tokens, a, n, ids), [(ids, w)], a, 4)
    assert tokens == 1 or (want[1].view(U32) == 0).all()                  # every row skipped: +0


def test_combine_strided_rows_at_offset_bases(qnnp):
    ids, w = routing(5, 2, 4, 1)
    check_combine(qnnp, "combine/layout", rows_for(5, 2, 33, ids), [(ids, w)], 2, 4, in_extra=3, out_extra=1, in_off=12, out_off=8)
    check_combine(qnnp, "combine/stride", rows_for(5, 2, 258, ids), [(ids, w)], 2, 4, in_extra=2, out_extra=2)


def test_combine_order_of_the_chain_and_the_flushes(qnnp):
    tokens, a, n = 3, 8, 64
    x, ids, w = rows_for(tokens, a, n), np.zeros(tokens * a, np.int32), np.ones(tokens * a, F32)
    assert (moe.combine(x, w, ids, a, 1, backwards=True).view(U32) != moe.combine(x, w, ids, a, 1).view(U32)).any()
    check_combine(qnnp, "combine/order", x, [(ids, w)], a, 1)
    # products and sums at and below 2^-126: weights 2^-100, inputs k 2^-27, k integer in [-8, 8]
    tiny = (np.random.default_rng(5).integers(-8, 9, (tokens * a, n)) * 2.0 ** -27).astype(F32)
    small = np.full(tokens * a, 2.0 ** -100, F32)
    want = check_combine(qnnp, "combine/tiny", tiny, [(ids, small)], a, 1)
    products = (small[:, None] * tiny).astype(F32)
    assert (np.abs(products) == moe.TINY).any() and (want != 0).any() and (np.abs(want[want != 0]) > moe.TINY).all()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_combine_rerouting_without_a_setup(qnnp, graph):
    first, second = routing(5, 2, 4, 11), routing(5, 2, 4, 12)
    assert (first[0] != second[0]).any()
    check_combine(qnnp, "combine/reroute", rows_for(5, 2, 33), [first, second], 2, 4, graph=graph)


def test_combine_refusals_in_their_order(qnnp):
    create, setup = qnnp.create_weighted_combine_nc_f32_status, qnnp.setup_weighted_combine_nc_f32_status
    for args, want in [((0, 1, 1), INV), ((8, 0, 1), INV), ((8, 1, 0), INV), ((0, 9, 1), INV), ((8, 9, 1), UNS),
                       ((8, 1, 1025), UNS), ((2 ** 24, 1, 1), UNS), ((2 ** 24 - 1, 8, 1024), OK)]:
        st, op = create(*args)
        if op:
            qnnp.delete_operator(op)
        assert st == want and bool(op) == (want == OK), (args, st)
    ids, w = routing(3, 2, 4, 3)
    x = rows_for(3, 2, 8, ids)
    gx, gi, gw, gy = Guarded(x), Guarded(ids), Guarded(w), Guarded(np.full(48, FILL, U32))
    op, other = create(8, 2, 4)[1], qnnp.create_topk_router_nc_f32(8, 2)
    try:
        assert setup(op, 3, gx, 8, gw, gi, gy, 8) == OK
        y = gy.data_ptr()
        for what, args, want in [
            ("NULL ids", (op, 3, gx, 8, gw, None, gy, 8), INV), ("misaligned weights", (op, 3, gx, 8, gw.data_ptr() + 1, gi, gy, 8), INV),
            ("stride", (op, 3, gx, 8, gw, gi, gy, 7), INV), ("T A = 2^20", (op, 2 ** 19, gx, 8, gw, gi, gy, 8), UNS),
            ("ids inside the output", (op, 3, gx, 8, gw, y + 32, gy, 8), INV), ("weights inside the output", (op, 3, gx, 8, y + 64, gi, gy, 8), INV),
            ("host weights", (op, 3, gx, 8, w, gi, gy, 8), INV), ("a router handle", (other, 3, gx, 8, gw, gi, gy, 8), INV),
        ]:
            assert setup(*args) == want, what
        qnnp.run_operator(op)                        # the setup before the refusals still stands
        same(gy.read().view(U32)[:24].reshape(3, 8), moe.combine(x, w, ids, 2, 4).view(U32), "after the refusals")
    finally:
        qnnp.delete_operator(op)
        qnnp.delete_operator(other)


# ---- the layer ----
def test_router_grouped_operator_and_combine_in_one_graph(qnnp):
    """logits -> ids and weights -> grouped _mxfp4w -> token rows, captured once; the second replay routes new logits, which
    never leave the device"""
    import torch
    groups, a, tokens, k, n = 4, 2, 5, 96, 33
    x, codes, e, bias = grp.problem("moe/layer", groups, tokens, k, n)
    logits = [logits_for(groups, tokens), logits_for(groups, tokens + 1)[1:]]
    gl, gx = Guarded(logits[0]), Guarded(x)
    gi, gw = Guarded(np.full(tokens * a, FILL, U32)), Guarded(np.full(tokens * a, FILL, U32))
    gr, gy = Guarded(np.full(tokens * a * n, FILL, U32)), Guarded(np.full(tokens * n, FILL, U32))
    ops = [qnnp.create_topk_router_nc_f32(groups, a), grp.create(qnnp, codes, e, bias), qnnp.create_weighted_combine_nc_f32(n, a, groups)]
    handle = None
    try:
        qnnp.setup_topk_router_nc_f32(ops[0], tokens, gl, groups, gi, gw)
        qnnp.setup_grouped_fully_connected_nc_f32_qd8(ops[1], tokens, a, gx, k, gi, gr, n)
        qnnp.setup_weighted_combine_nc_f32(ops[2], tokens, gr, n, gw, gi, gy, n)
        qnnp.graph_begin()
        try:
            for op in ops:
                qnnp.run_operator(op)
        finally:
            handle = qnnp.graph_end()
        wants = []
        for given in logits:
            gl.view.copy_(torch.from_numpy(given.view(np.uint8).reshape(-1)))
            torch.cuda.synchronize()
            qnnp.graph_launch(handle)
            qnnp.graph_synchronize(handle)
            ids, w = moe.router(given, a)
            rows = grp.expected(x, a, ids.reshape(-1), codes, e, bias).view(F32)
            wants.append(moe.combine(rows, w.reshape(-1), ids.reshape(-1), a, groups))
            same(gy.read().view(U32).reshape(tokens, n), wants[-1].view(U32), "moe/layer")
        assert (wants[0].view(U32) != wants[1].view(U32)).any()
    finally:
        if handle is not None:
            qnnp.graph_destroy(handle)
        for op in ops:
            qnnp.delete_operator(op)
    for g in (gl, gx, gi, gw, gr, gy):
        g.assert_intact("moe/layer")
