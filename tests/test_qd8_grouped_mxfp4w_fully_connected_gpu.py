"""GPU tier of the GROUPED dynamically quantized fully connected operator with MXFP4 weights
(qnnp_gfx950_create_grouped_fully_connected_nc_f32_qd8_mxfp4w / qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8:
hip/qd8f32gemm4g.hip behind dynamic-fully-connected.c). Output row j is the _mxfp4w definition for input row j / A with the
weights of group ids[j], so the expectation is that test module's numpy restatement, group by group; rows with an id outside
[0, groups) must keep the fill pattern. Outputs are compared as uint32 bit patterns inside guard bytes, and the product
kernel's name is asserted per case from the rule R <= 16 * groups."""
import numpy as np
import pytest

import test_qd8_mxfp4w_fully_connected_gpu as mx
from _gpu import Guarded
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

F32, FILL, INF, B = np.float32, mx.FILL, float("inf"), 32
INT32_MIN = -2 ** 31


def problem(name, groups, batch, k, n):
    """x [batch][K], codes [groups][N][K], e [groups][N][K / 32], bias [groups][N] (distinct per group)"""
    x = mx.problem(name, batch, k, n)[0]
    sets = [mx.problem(f"{name}/g{g}", 1, k, n)[1:] for g in range(groups)]
    return (x,) + tuple(np.stack([s[i] for s in sets]) for i in range(3))


def routing(kind, groups, rows, seed=0):
    rng = np.random.default_rng(1000 * groups + rows + seed)
    if isinstance(kind, list):
        ids = kind
    elif kind == "robin":
        ids = np.arange(rows) % groups
    elif kind == "random":
        ids = rng.integers(0, groups, rows)
    elif kind == "random_but_2":                     # group 2 stays empty
        ids = rng.permutation(np.array([g for g in range(groups) if g != 2])[np.arange(rows) % (groups - 1)])
    elif kind == "129_21":
        ids = rng.permutation(np.repeat([0, 1], [129, 21]))
    else:                                            # ("all", g)
        ids = np.full(rows, kind[1])
    ids = np.asarray(ids, np.int32)
    assert ids.shape == (rows,)
    return ids


def expected(x, a, ids, codes, e, bias):
    """bits [R][N]: FILL where the row is skipped"""
    want = np.full((len(ids), codes.shape[1]), FILL, np.uint32)
    for g in range(codes.shape[0]):
        rows = np.flatnonzero(ids == g)
        if rows.size:
            want[rows] = mx.expected(x[rows // a], codes[g], e[g], bias[g]).view(np.uint32)
    return want


def create(qnnp, codes, e, bias):
    groups, n, k = codes.shape
    return qnnp.create_grouped_fully_connected_nc_f32_qd8_mxfp4w(
        groups, k, n, np.stack([mx.pack(c) for c in codes]), e, bias, -INF, INF)


def run(qnnp, name, op, x, a, routings, groups, n, graph=False, in_extra=0, out_extra=0, in_off=0, out_off=0):
    """ONE setup of `op` (deleted here), then one run per routing, the device ids overwritten in place in between and the
    output refilled; a graph is captured once and replayed twice per routing. Returns the output bits [R][n] per routing."""
    import torch
    batch, k = x.shape
    rows, in_stride, out_stride = batch * a, k + in_extra, n + out_extra
    x_host = np.full((batch - 1) * in_stride + k, 7.25, F32)
    for r in range(batch):
        x_host[r * in_stride:r * in_stride + k] = x[r]
    fill = np.full((rows - 1) * out_stride + n, FILL, np.uint32)
    gx, gy, gi = Guarded(x_host, in_off), Guarded(fill, out_off), Guarded(routings[0])
    cells = (np.arange(rows)[:, None] * out_stride + np.arange(n)).ravel()
    handle, results = None, []
    try:
        assert qnnp.setup_grouped_fully_connected_nc_f32_qd8_status(op, batch, a, gx, in_stride, gi, gy, out_stride) == Status.success
        if graph:
            qnnp.graph_begin()
            try:
                qnnp.run_operator(op)
            finally:
                handle = qnnp.graph_end()
        for ids in routings:
            for _ in range(2 if graph else 1):
                gi.view.copy_(torch.from_numpy(ids.view(np.uint8)))
                gy.view.copy_(torch.from_numpy(fill.view(np.uint8)))
                torch.cuda.synchronize()
                if graph:
                    qnnp.graph_launch(handle)
                    qnnp.graph_synchronize(handle)
                else:
                    qnnp.run_operator(op)
                got = gy.read().view(np.uint32)
                assert np.all(np.delete(got, cells) == FILL), name + ": a gap between output rows was written"
                results.append(got[cells].reshape(rows, n))
        want = "qd8_f32_mxfp4w_grouped_mfma_16" if rows <= 16 * groups else "qd8_f32_mxfp4w_grouped_mfma_128x128"
        assert qnnp.operator_kernel(op) == want, (name, qnnp.operator_kernel(op))
        assert qnnp.dynamic_rows_kernel(op).startswith("f32_qd8_rows_")
    finally:
        if handle is not None:
            qnnp.graph_destroy(handle)
        qnnp.delete_operator(op)
    for g in (gx, gy, gi):
        g.assert_intact(name)
    return results[::2] if graph and same(results[1::2], results[::2], name + " (second replay)") else results


def same(got, want, name):
    for i, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{name} [{i}]: {len(bad)} of {w.size} differ, first at {bad[:4].tolist()}: {g[tuple(bad[0])]:#x} != {w[tuple(bad[0])]:#x}"
    return True


def check(qnnp, name, groups, batch, a, k, n, kinds, prob=None, **how):
    x, codes, e, bias = prob or problem(name, groups, batch, k, n)
    routings = [routing(kind, groups, batch * a, i) if not isinstance(kind, np.ndarray) else kind for i, kind in enumerate(kinds)]
    got = run(qnnp, name, create(qnnp, codes, e, bias), x, a, routings, groups, n, **how)
    same(got, [expected(x, a, ids, codes, e, bias) for ids in routings], name)
    return got, routings, (x, codes, e, bias)


# (groups, batch, A, K, N, routing): the smallest at which each mechanism can go wrong
SMALL = (4, 5, 2, 96, 33, "random_but_2")           # _16: A = 2, an empty group, an odd block count
FULL_AND_4 = (2, 20, 1, 160, 130, ("all", 1))       # _16: a full tile and a tile of 4 in one group
THREE_17 = (3, 17, 3, 64, 33, "robin")              # R = 51 > 48: _128x128, three partial tiles of 17
TWO_TILES = (2, 150, 1, 160, 130, "129_21")         # _128x128: a full tile, a tile of one row, a partial tile; two column tiles
CASES = [
    (1, 1, 1, 32, 1, ("all", 0)),                   # the smallest problem
    (2, 2, 1, 32, 16, [1, 0]),                      # T attained exactly (0 + 2 tiles); perm is not the identity
    SMALL, FULL_AND_4,
    (3, 16, 3, 2080, 16, "robin"),                  # R = 16 * groups exactly: still _16; one block past a pass of 32 tiles
    THREE_17, TWO_TILES,
    (2, 131, 2, 32, 1, "random"),                   # _128x128 with A = 2, one block, N = 1
    (5, 90, 1, 2080, 33, ("all", 3)),               # _128x128, four groups empty, long K
]


def case_id(case):
    return "g{}_b{}_a{}_k{}_n{}".format(*case[:5])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_shapes_and_routings(qnnp, case):
    check(qnnp, "grouped/" + case_id(case), *case[:5], [case[5]])


@pytest.mark.parametrize("case", [FULL_AND_4, TWO_TILES], ids=case_id)
def test_skipped_rows_keep_the_fill_pattern(qnnp, case):
    groups, rows = case[0], case[1] * case[2]
    ids = routing(case[5], groups, rows)
    ids[1::4] = np.array([-1, groups, INT32_MIN], np.int32)[np.arange(len(ids[1::4])) % 3]
    got, _, _ = check(qnnp, "skip/" + case_id(case), *case[:5], [ids])
    assert (got[0][1::4] == FILL).all() and (got[0][0::4] != FILL).any()


@pytest.mark.parametrize("case", [SMALL, THREE_17], ids=case_id)
def test_equals_the_stand_alone_operator(qnnp, case):
    name, a, n = "alone/" + case_id(case), case[2], case[4]
    got, (ids,), (x, codes, e, bias) = check(qnnp, name, *case[:5], [case[5]])
    for g in np.unique(ids):
        rows = np.flatnonzero(ids == g)
        op = qnnp.create_fully_connected_nc_f32_qd8_mxfp4w(case[3], n, mx.pack(codes[g]), e[g], bias[g], -INF, INF)
        assert (mx.run(qnnp, f"{name}/g{g}", op, x[rows // a], n) == got[0][rows]).all(), (name, g)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", [SMALL, THREE_17], ids=case_id)
def test_rerouting_without_a_setup(qnnp, case, graph):
    """the ids are overwritten on the device between two runs (or replays) of one setup"""
    _, (first, second), _ = check(qnnp, "reroute/" + case_id(case), *case[:5], [case[5], "random"], graph=graph)
    assert (first != second).any()


@pytest.mark.parametrize("case", [SMALL, THREE_17], ids=case_id)
def test_strided_rows_and_offset_bases(qnnp, case):
    check(qnnp, "layout/" + case_id(case), *case[:5], [case[5]], in_extra=1, out_extra=1, in_off=12, out_off=8)


@pytest.mark.parametrize("groups,batch", [(3, 4), (3, 52)], ids=["16", "128x128"])
def test_per_group_bias_and_the_order_of_the_chain(qnnp, groups, batch):
    """block exponents alternating between 136 and 118 in every group: any other order of the same terms rounds differently"""
    k, n = 2048, 33
    x, codes, e, bias = problem("ordergrp", groups, batch, k, n)
    e = (np.where(np.arange(k // B) % 2 == 0, 136, 118)[None, None, :] + (e & 1)).astype(np.uint8)
    assert len({b.tobytes() for b in bias}) == groups
    for g in range(groups):
        t, scale, _ = mx.terms(x, codes[g], e[g])
        backwards = np.zeros_like(t[0])
        for t_b in reversed(t):
            backwards = backwards + t_b
        pairwise = list(t)
        while len(pairwise) > 1:
            pairwise = [pairwise[i] + pairwise[i + 1] for i in range(0, len(pairwise), 2)]
        for other in (backwards, pairwise[0]):
            assert (mx.finish(other, scale, bias[g]).view(np.uint32) != mx.expected(x, codes[g], e[g], bias[g]).view(np.uint32)).any()
    check(qnnp, f"ordergrp/b{batch}", groups, batch, 1, k, n, ["robin"], prob=(x, codes, e, bias))


G, K, N = 2, 128, 4
KERNEL, SCALES, BIAS = np.full((G, N, K // 2), 0x1F, np.uint8), np.full((G, N, K // B), 127, np.uint8), np.zeros((G, N), F32)
INV, UNS, OK = Status.invalid_parameter, Status.unsupported_parameter, Status.success


def _with(value, bias_nan=False):
    scales, bias = SCALES.copy(), BIAS.copy()
    scales[G - 1, 2, 1] = value                       # in the last group only
    if bias_nan:
        bias[G - 1, 1] = np.nan
    return scales, bias


def _many(groups):
    return (groups, 32, 1, np.zeros((max(groups, 1), 1, 16), np.uint8), np.full((max(groups, 1), 1, 1), 127, np.uint8), None, -INF, INF)


@pytest.mark.parametrize("args,want", [
    ((G, K, N, KERNEL, SCALES, BIAS, -INF, INF), OK),
    (_many(0), INV),
    (_many(1024), OK),
    (_many(1025), UNS),
    ((G, K, N, KERNEL) + _with(255) + (-INF, INF), INV),
    ((G, K, N, KERNEL) + _with(110) + (-INF, INF), UNS),
    ((G, K, N, KERNEL) + _with(110, bias_nan=True) + (-INF, INF), INV),                 # invalid before unsupported
    ((G, 48, N, np.zeros((G, N, 24), np.uint8), SCALES[:, :, :1], BIAS, -INF, INF), UNS),     # K is no multiple of 32
], ids=["ok", "groups0", "groups1024", "groups1025", "scale255", "scale110", "invalid_first", "k48"])
def test_create_refusals_in_their_order(qnnp, args, want):
    st, op = qnnp.create_grouped_fully_connected_nc_f32_qd8_mxfp4w_status(*args)
    if op:
        qnnp.delete_operator(op)
    assert st == want and bool(op) == (want == OK), (args[:3], st, want)


def test_setup_refusals_in_their_order(qnnp):
    batch, a = 3, 2
    x = mx.problem("setupgrp", batch, K, N)[0]
    ids = np.array([0, 1, 1, 0, 1, 0], np.int32)
    gx, gi = Guarded(x), Guarded(np.concatenate([ids, ids]))
    gy = Guarded(np.full(batch * a * N, FILL, np.uint32))
    op = qnnp.create_grouped_fully_connected_nc_f32_qd8_mxfp4w(G, K, N, KERNEL, SCALES, BIAS, -INF, INF)
    plain = qnnp.create_fully_connected_nc_f32_qd8_mxfp4w(K, N, KERNEL[0], SCALES[0], BIAS[0], -INF, INF)
    setup = qnnp.setup_grouped_fully_connected_nc_f32_qd8_status
    try:
        assert setup(op, batch, a, gx, K, gi, gy, N) == OK
        y, i = gy.data_ptr(), gi.data_ptr()
        for what, args, want in [
            ("NULL ids", (op, batch, a, gx, K, None, gy, N), INV),
            ("misaligned ids", (op, batch, a, gx, K, i + 2, gy, N), INV),
            ("ids inside the output", (op, batch, a, gx, K, y + 4 * N, gy, N), INV),
            ("A = 0", (op, batch, 0, gx, K, gi, gy, N), INV),
            ("A = 9", (op, 1, 9, gx, K, gi, gy, N), UNS),
            ("R = 2^20", (op, 2 ** 19, 2, gx, K, gi, gy, N), UNS),        # answered from the sizes, before any span or access
            ("a plain handle", (plain, batch, a, gx, K, gi, gy, N), INV),
        ]:
            assert setup(*args) == want, what
        assert qnnp.setup_fully_connected_nc_f32_qd8_status(op, batch, gx, K, gy, N) == INV, "a grouped handle, plain setup"
        qnnp.run_operator(op)                        # the setup before the refusals still stands
        got = gy.read().view(np.uint32).reshape(batch * a, N)
        scales4 = np.broadcast_to(SCALES[0], (N, K // B))
        codes = np.tile(np.array([15, 1]), (N, K // 2))
        same([got], [expected(x, a, ids, np.stack([codes] * G), np.stack([scales4] * G), BIAS)], "after the refusals")
    finally:
        qnnp.delete_operator(op)
        qnnp.delete_operator(plain)
