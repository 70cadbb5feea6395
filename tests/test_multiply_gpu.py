"""GPU tier of the multiply operator (hip/q8mul.hip behind multiply.c) and of the hardswish and hardsigmoid tables.

No reference operator exists for any of the three, so every expectation is the oracle's: oracle.o1.q31_requantize on
the int32 products formed in numpy, and the table formulas in numpy float32 (tests/_multiply.py). All comparisons are
byte-exact and include the FILL bytes between strided rows.

 1. every (a, b) byte pair once, for one parameter set per requantization and clamp class;
 2. shapes: channel counts around the piece widths, broadcast factors, strides, base misalignments, the kernel of each
    alignment class, more than one pass of each kernel's loops, the broadcast boundary;
 3. guarded tensors at odd offsets, in place on either operand, the square;
 4. create and setup statuses, host pointers, async mode, re-setup, operator kinds;
 5. the two activation tables over their parameter ranges, and their statuses;
 6. a squeeze-and-excite block -- pooling, two fully connected layers, hardsigmoid, multiply in place -- as one hipGraph.
"""
import numpy as np
import pytest

import _multiply as mul
from _cases import FcCase
from _gpu import Guarded, from_device, to_device
from _runner import fc_expected
from oracle import o1
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu


def _differences(got, want, what):
    if not np.array_equal(got, want):
        assert got.size == want.size, (what, got.size, want.size)
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[:4]}: got {got[bad[:4]]}, want {want[bad[:4]]}")


def _run(qnnp, q, s, name, misalign=(0, 0, 0), op=None):
    """one shape on fresh device buffers at the given base misalignments; returns the kernel name"""
    a, b, y = mul.tensors(name, s)
    want = mul.expected(q, s, a, b, y)
    own = op is None
    if own:
        op = qnnp.create_multiply_nc_q8(s.channels, *q.args())
    try:
        d_a, d_b, d_y = (to_device(t, m) for t, m in zip((a, b, y), misalign))
        assert mul.setup_status(qnnp, op, s, d_a, d_b, d_y) == Status.success, name
        qnnp.run_operator(op)
        kernel = qnnp.operator_kernel(op)
        _differences(from_device(d_y), want, f"{name} ({kernel})")
        _differences(from_device(d_a), a, f"{name} ({kernel}): a changed")
        _differences(from_device(d_b), b, f"{name} ({kernel}): b changed")
        assert kernel == mul.kernel_for(s, d_a.data_ptr(), d_b.data_ptr(), d_y.data_ptr()), (name, kernel)
        return kernel
    finally:
        if own:
            qnnp.delete_operator(op)


# ---- 1. the whole input domain -----------------------------------------------------------------------------------
def _every_pair_of_bytes_in_every_requantization_class(qnnp):
    """a[r][c] = r, b[r][c] = c: 256 x 256 is every (a, b) pair once, element-wise"""
    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1).copy()
    b = np.ascontiguousarray(a.T)
    d_a, d_b = to_device(a), to_device(b)
    d_y = to_device(np.full(65536, mul.FILL, np.uint8))
    for name, q, distinct in mul.EXHAUSTIVE:
        want = mul.product_rows(q, a, b)
        # a kernel that writes a constant cannot pass (tests/_multiply.py says why some sets can only state 1)
        assert np.unique(want).size >= distinct, (name, np.unique(want).size)
        op = qnnp.create_multiply_nc_q8(256, *q.args())
        try:
            d_y.fill_(mul.FILL)
            qnnp.setup_multiply_nc_q8(op, 256, 1, d_a, 256, d_b, 256, d_y, 256)
            qnnp.run_operator(op)
            assert qnnp.operator_kernel(op) == "q8_mul_x16"
            _differences(from_device(d_y), want.reshape(-1), name)
            # the same through the dword and the byte kernels: strides of 260 and 257 bytes
            for stride, kernel in ((260, "q8_mul_x4"), (257, "q8_mul_x1")):
                s = mul.Shape(256, 256, 1, y_stride=stride)
                y = np.full(mul.span(256, stride, 256), mul.FILL, np.uint8)
                d_s = to_device(y)
                assert mul.setup_status(qnnp, op, s, d_a, d_b, d_s) == Status.success
                qnnp.run_operator(op)
                assert qnnp.operator_kernel(op) == kernel
                _differences(from_device(d_s), mul.expected(q, s, a.reshape(-1), b.reshape(-1), y), f"{name}/{kernel}")
        finally:
            qnnp.delete_operator(op)


# ---- 2. shapes ---------------------------------------------------------------------------------------------------
CHANNELS = (1, 3, 4, 15, 16, 17, 31, 32, 33, 58, 64, 100)


def _shapes_dense_and_strided(qnnp):
    for c in CHANNELS:
        op = qnnp.create_multiply_nc_q8(c, *mul.MID.args())
        try:
            for b_rows in (1, 3):
                for per in (1, 2, 49):
                    for strides in ((0, 0, 0), (c + 3, c + 16, c + 7)):
                        s = mul.Shape(c, b_rows, per, *strides)
                        _run(qnnp, mul.MID, s, f"shape/c{c}_b{b_rows}_p{per}_s{strides[0]}", op=op)
        finally:
            qnnp.delete_operator(op)


def _base_misalignments_for_short_rows(qnnp):
    """1 .. 49 bytes per row with the three base addresses misaligned by 0 .. 15 bytes: every head and tail of a row"""
    seen = set()
    for c in range(1, 50):
        op = qnnp.create_multiply_nc_q8(c, *mul.MID.args())
        try:
            for m in range(16):
                s = mul.Shape(c, 2, 3)
                # alike, then each tensor on its own class
                seen.add(_run(qnnp, mul.MID, s, f"misalign/c{c}_m{m}", (m, m, m), op=op))
                if c in (16, 32) and m % 3 == 1:
                    for mis in ((m, 0, 0), (0, m, 0), (0, 0, m)):
                        seen.add(_run(qnnp, mul.MID, s, f"misalign/c{c}_{mis}", mis, op=op))
        finally:
            qnnp.delete_operator(op)
    assert seen == {"q8_mul_x16", "q8_mul_x4", "q8_mul_x1"}


KERNEL_BY_ALIGNMENT = [   # (channels, b rows, a rows per b row, strides of a, b, product, misalignment of a, b, product, kernel)
    (64, 3, 7, 0, 0, 0, 0, 0, 0, "q8_mul_x16"), (16, 1, 1, 0, 0, 0, 0, 0, 0, "q8_mul_x16"),
    (32, 3, 7, 48, 64, 80, 0, 0, 0, "q8_mul_x16"), (32, 3, 7, 48, 64, 80, 16, 32, 48, "q8_mul_x16"),
    (32, 3, 7, 48, 64, 84, 0, 0, 0, "q8_mul_x4"), (32, 3, 7, 48, 36, 80, 0, 0, 0, "q8_mul_x4"),
    (32, 3, 7, 36, 64, 80, 0, 0, 0, "q8_mul_x4"), (32, 3, 7, 0, 0, 0, 0, 0, 4, "q8_mul_x4"),
    (32, 3, 7, 0, 0, 0, 8, 0, 0, "q8_mul_x4"), (32, 3, 7, 0, 0, 0, 0, 12, 0, "q8_mul_x4"),
    (20, 3, 7, 0, 0, 0, 0, 0, 0, "q8_mul_x4"), (4, 3, 7, 0, 0, 0, 0, 0, 0, "q8_mul_x4"),
    (24, 3, 7, 0, 0, 0, 0, 0, 0, "q8_mul_x4"),            # 24 channels: rows are 8 bytes off the 16-byte grid
    (32, 3, 7, 0, 0, 0, 0, 0, 1, "q8_mul_x1"), (32, 3, 7, 0, 0, 0, 2, 0, 0, "q8_mul_x1"),
    (32, 3, 7, 0, 0, 0, 0, 3, 0, "q8_mul_x1"), (32, 3, 7, 33, 32, 32, 0, 0, 0, "q8_mul_x1"),
    (32, 3, 7, 32, 34, 32, 0, 0, 0, "q8_mul_x1"), (32, 3, 7, 32, 32, 35, 0, 0, 0, "q8_mul_x1"),
    (30, 3, 7, 32, 32, 32, 0, 0, 0, "q8_mul_x1"), (17, 3, 7, 0, 0, 0, 0, 0, 0, "q8_mul_x1"),
    # the strides count even where a tensor has one row
    (32, 1, 7, 48, 33, 80, 0, 0, 0, "q8_mul_x1"), (32, 1, 1, 33, 48, 80, 0, 0, 0, "q8_mul_x1")]


def _kernel_follows_alignment(qnnp):
    for c, b_rows, per, sa, sb, sy, ma, mb, my, kernel in KERNEL_BY_ALIGNMENT:
        s = mul.Shape(c, b_rows, per, sa, sb, sy)
        assert _run(qnnp, mul.MID, s, f"path/c{c}_{sa}_{sb}_{sy}_{ma}_{mb}_{my}", (ma, mb, my)) == kernel, (c, sa, sb, sy, ma, mb, my)


def _more_than_one_pass_of_each_loop(qnnp):
    """hip/q8mul.hip launches at most compute units x 16 workgroups; beyond that its grid-stride loops take further
    passes. One case per kernel whose row groups exceed one pass of grid x -- the smallest such tensors: rows of 129
    pieces, the fewest that fill a workgroup alone -- and one row with more 256-piece chunks than one pass of grid y."""
    cap = qnnp.device_info()["compute_units"] * 16
    for s, kernel in ((mul.Shape(16 * 129, 2, cap // 2 + 3), "q8_mul_x16"), (mul.Shape(4 * 129, cap // 49 + 1, 49), "q8_mul_x4"),
                      (mul.Shape(129, 3, cap // 3 + 2), "q8_mul_x1")):
        pieces = s.channels // int(kernel.rsplit("x", 1)[1])
        assert 128 < pieces <= 256 and s.rows > cap, (s, cap)            # one row a workgroup, more workgroups than the cap
        assert _run(qnnp, mul.MID, s, f"sweep/{kernel}_c{s.channels}") == kernel
    # rows longer than a workgroup: 3 chunks of 256 pieces and a partial one; then more chunks than the launch cap
    long_row = cap * 256 + 301
    assert long_row % 4 != 0 and -(-long_row // 256) > cap
    for s, kernel in ((mul.Shape(16 * 800, 2, 3), "q8_mul_x16"), (mul.Shape(4 * 800, 2, 3, 3204, 3200, 3208), "q8_mul_x4"),
                      (mul.Shape(long_row, 1, 2), "q8_mul_x1")):
        assert _run(qnnp, mul.MID, s, f"sweep_long/{kernel}_c{s.channels}") == kernel
    # rows x a_rows_per_b_row at 2^32 or more: the row of b comes from a plain division, not the reciprocal
    for s, kernel in ((mul.Shape(16, 2, 46341), "q8_mul_x16"), (mul.Shape(1, 2, 65536), "q8_mul_x1")):
        assert s.rows * s.per >= 2 ** 32
        assert _run(qnnp, mul.MID, s, f"division/{kernel}") == kernel


def _broadcast_boundary(qnnp):
    """49 rows of a per row of b, three DIFFERENT b rows: an off-by-one in r / a_rows_per_b_row changes rows 48/49 and
    97/98"""
    for c, strides in ((24, (0, 0, 0)), (16, (0, 0, 0)), (7, (9, 8, 11))):
        s = mul.Shape(c, 3, 49, *strides)
        a, b, y = mul.tensors(f"boundary/c{c}", s)
        sa, sb, sy = s.strides
        a_rows = mul.rows_view(a, s.rows, sa, c)
        a_rows[...] = a_rows[0]                             # identical a rows: the product rows differ through b only
        b_rows = mul.rows_view(b, 3, sb, c)
        want = mul.expected(mul.MID, s, a, b, y)
        w = mul.rows_view(want, s.rows, sy, c)
        assert np.array_equal(w[47], w[48]) and not np.array_equal(w[48], w[49]) and np.array_equal(w[49], w[50])
        assert np.array_equal(w[96], w[97]) and not np.array_equal(w[97], w[98]) and not np.array_equal(w[0], w[146])
        assert not np.array_equal(b_rows[0], b_rows[1]) and not np.array_equal(b_rows[1], b_rows[2])
        op = qnnp.create_multiply_nc_q8(c, *mul.MID.args())
        try:
            d_a, d_b, d_y = to_device(a), to_device(b), to_device(y)
            assert mul.setup_status(qnnp, op, s, d_a, d_b, d_y) == Status.success
            qnnp.run_operator(op)
            _differences(from_device(d_y), want, f"boundary/c{c}")
        finally:
            qnnp.delete_operator(op)


# ---- 3. guards and in place --------------------------------------------------------------------------------------
GUARDED = [   # (channels, b rows, a rows per b row, strides of a, b, product, offsets of a, b, product)
    (64, 3, 5, 0, 0, 0, 0, 0, 0), (64, 3, 5, 0, 0, 0, 16, 32, 48), (7, 3, 5, 0, 0, 0, 3, 3, 3), (100, 2, 9, 0, 0, 0, 1, 9, 5),
    (24, 3, 5, 41, 44, 43, 2, 0, 7), (32, 3, 5, 48, 64, 80, 0, 0, 0), (32, 3, 5, 36, 40, 44, 4, 8, 12), (33, 1, 13, 50, 50, 37, 7, 3, 1),
    (16, 13, 1, 0, 0, 0, 0, 0, 0), (1, 5, 3, 0, 0, 0, 15, 14, 13)]


def _nothing_is_written_outside_the_product(qnnp):
    for c, b_rows, per, sa, sb, sy, oa, ob, oy in GUARDED:
        s = mul.Shape(c, b_rows, per, sa, sb, sy)
        name = f"guarded/c{c}_{sa}_{sb}_{sy}_{oa}_{ob}_{oy}"
        a, b, y = mul.tensors(name, s)
        ga, gb, gy = Guarded(a, oa), Guarded(b, ob), Guarded(y, oy)
        op = qnnp.create_multiply_nc_q8(c, *mul.MID.args())
        try:
            assert mul.setup_status(qnnp, op, s, ga, gb, gy) == Status.success
            qnnp.run_operator(op)
            _differences(gy.read(), mul.expected(mul.MID, s, a, b, y), name)
            for g, t, what in ((gy, None, "product"), (ga, a, "a"), (gb, b, "b")):
                g.assert_intact(f"{name} ({what})")
                if t is not None:
                    _differences(g.read(), t, f"{name}: {what} changed")
        finally:
            qnnp.delete_operator(op)


IN_PLACE = [   # (channels, b rows, a rows per b row, stride of the in-place tensor, stride of the other input, offset)
    (64, 3, 5, 0, 0, 0), (64, 3, 1, 0, 0, 16), (7, 3, 5, 0, 0, 3), (24, 3, 5, 41, 0, 1), (100, 2, 9, 116, 104, 4),
    (33, 5, 1, 33, 40, 15), (16, 4, 1, 32, 16, 0), (20, 4, 7, 24, 20, 8)]


def _in_place_and_the_square(qnnp):
    """in place on a (broadcast and element-wise), in place on b (element-wise), and a == b; guarded, at odd offsets"""
    for c, b_rows, per, s_self, s_other, offset in IN_PLACE:
        op = qnnp.create_multiply_nc_q8(c, *mul.MID.args())
        try:
            # product == a
            s = mul.Shape(c, b_rows, per, s_self, s_other, s_self)
            name = f"in_place_a/c{c}_p{per}_s{s_self}"
            a, b, _ = mul.tensors(name, s)
            ga, gb = Guarded(a, offset), Guarded(b, offset)
            assert mul.setup_status(qnnp, op, s, ga, gb, ga) == Status.success, name
            qnnp.run_operator(op)
            _differences(ga.read(), mul.expected(mul.MID, s, a, b, a), f"{name} ({qnnp.operator_kernel(op)})")
            ga.assert_intact(name)
            gb.assert_intact(name + " (b)")
            _differences(gb.read(), b, f"{name}: b changed")
            if per != 1:
                continue
            # product == b, element-wise
            s = mul.Shape(c, b_rows, 1, s_other, s_self, s_self)
            name = f"in_place_b/c{c}_s{s_self}"
            a, b, _ = mul.tensors(name, s)
            ga, gb = Guarded(a, offset), Guarded(b, offset)
            assert mul.setup_status(qnnp, op, s, ga, gb, gb) == Status.success, name
            qnnp.run_operator(op)
            _differences(gb.read(), mul.expected(mul.MID, s, a, b, b), name)
            gb.assert_intact(name)
            _differences(ga.read(), a, f"{name}: a changed")
            # a == b: the square, out of place and in place
            s = mul.Shape(c, b_rows, 1, s_self, s_self, s_other)
            name = f"square/c{c}_s{s_self}"
            a, _, y = mul.tensors(name, s)
            ga, gy = Guarded(a, offset), Guarded(y, offset)
            assert mul.setup_status(qnnp, op, s, ga, ga, gy) == Status.success, name
            qnnp.run_operator(op)
            _differences(gy.read(), mul.expected(mul.MID, s, a, a, y), name)
            gy.assert_intact(name)
            _differences(ga.read(), a, f"{name}: a changed")
            s = mul.Shape(c, b_rows, 1, s_self, s_self, s_self)
            assert mul.setup_status(qnnp, op, s, ga, ga, ga) == Status.success, name
            qnnp.run_operator(op)
            _differences(ga.read(), mul.expected(mul.MID, s, a, a, a), name + " in place")
            ga.assert_intact(name + " in place")
        finally:
            qnnp.delete_operator(op)


# ---- 4. API ------------------------------------------------------------------------------------------------------
INF, NAN = float("inf"), float("nan")
# (channels, a zp, a scale, b zp, b scale, product zp, product scale, min, max) -> status, in the documented order
MULTIPLY_CREATE = [
    ((8, 121, 0.05, 0, 1 / 256, 133, 0.04, 0, 255), Status.success),
    ((1, 255, 2.0 ** -16, 255, 2.0 ** -16, 255, 1.0, 0, 1), Status.success),                # ratio 2^-32
    ((2 ** 31 - 1, 0, mul.BELOW_ONE, 0, 1.0, 0, 1.0, 254, 255), Status.success),            # the largest ratio and size
    ((0, 121, 0.05, 0, 1 / 256, 133, 0.04, 0, 255), Status.invalid_parameter),
    ((0, 121, 0.0, 0, 0.0, 133, 0.0, 9, 1), Status.invalid_parameter),
    ((8, 121, 0.0, 0, 1 / 256, 133, 0.04, 0, 255), Status.invalid_parameter),
    ((8, 121, -0.05, 0, 1 / 256, 133, 0.04, 0, 255), Status.invalid_parameter),
    ((8, 121, 1e-40, 0, 1 / 256, 133, 0.04, 0, 255), Status.invalid_parameter),
    ((8, 121, INF, 0, 1 / 256, 133, 0.04, 0, 255), Status.invalid_parameter),
    ((8, 121, 0.05, 0, 0.0, 133, 0.04, 0, 255), Status.invalid_parameter),
    ((8, 121, 0.05, 0, NAN, 133, 0.04, 0, 255), Status.invalid_parameter),
    ((8, 121, 0.05, 0, 1 / 256, 133, 0.0, 0, 255), Status.invalid_parameter),
    ((8, 121, 0.05, 0, 1 / 256, 133, INF, 0, 255), Status.invalid_parameter),
    ((8, 121, 0.05, 0, 1 / 256, 133, 0.04, 100, 100), Status.invalid_parameter),
    ((8, 121, 0.05, 0, 1 / 256, 133, 0.04, 200, 100), Status.invalid_parameter),
    ((2 ** 31, 121, 0.05, 0, 1 / 256, 133, 0.04, 200, 100), Status.invalid_parameter),      # invalid before unsupported
    ((8, 121, 1.0, 0, 1.0, 133, 1.0, 200, 100), Status.invalid_parameter),
    ((2 ** 31, 121, 0.05, 0, 1 / 256, 133, 0.04, 0, 255), Status.unsupported_parameter),
    ((8, 121, 1.0, 0, 1.0, 133, 1.0, 0, 255), Status.unsupported_parameter),                # ratio 1
    ((8, 121, 2.0, 0, 3.0, 133, 1.0, 0, 255), Status.unsupported_parameter),
    ((8, 121, 2.0 ** -17, 0, 2.0 ** -17, 133, 1.0, 0, 255), Status.unsupported_parameter),  # 2^-34
    ((8, 121, 2.0 ** -16, 0, 2.0 ** -16, 133, 1.0000001, 0, 255), Status.unsupported_parameter),
    ((8, 121, 2.0 ** -80, 0, 2.0 ** -80, 133, 2.0 ** -100, 0, 255), Status.unsupported_parameter),   # a * b underflows
    ((8, 121, 2.0 ** 80, 0, 2.0 ** 80, 133, 2.0 ** 100, 0, 255), Status.unsupported_parameter)]      # a * b overflows


def _create_statuses(qnnp):
    for args, want in MULTIPLY_CREATE:
        st, op = qnnp.create_multiply_nc_q8_status(*args)
        if op:
            qnnp.delete_operator(op)
        assert st == want and bool(op) == (want == Status.success), (args, st)
    # the oracle accepts exactly the ratios create accepts
    for args, want in MULTIPLY_CREATE:
        if want != Status.invalid_parameter and args[0] < 2 ** 31:
            q = mul.Quant(*args[1:])
            accepted = True
            try:
                with np.errstate(over="ignore", under="ignore"):
                    mul.product_rows(q, np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8))
            except ValueError:
                accepted = False
            assert accepted == (want == Status.success), args
    st, op = qnnp.create_multiply_nc_q8_status(8, *mul.MID.args(), flags=0xFFFFFFFF)       # flags: accepted and ignored
    assert st == Status.success
    assert qnnp.run_operator_status(op) == Status.invalid_parameter                         # before any setup
    qnnp.operator_set_streaming_stores(op, 1)
    qnnp.operator_set_streaming_stores(op, 0)
    qnnp.operator_set_streaming_stores(op, -1)
    qnnp.delete_operator(op)


def _setup_statuses_and_overlaps(qnnp):
    c = 16
    op = qnnp.create_multiply_nc_q8(c, *mul.MID.args())
    d = to_device(np.arange(8192, dtype=np.uint32).astype(np.uint8))
    e = to_device(np.zeros(8192, np.uint8))
    base = d.data_ptr()
    setup = qnnp.setup_multiply_nc_q8_status
    try:
        # no rows: success, and run does nothing, whatever the pointers
        assert setup(op, 0, 5, None, 0, None, 0, None, 0) == Status.success
        assert qnnp.run_operator_status(op) == Status.success
        assert setup(op, 5, 0, None, 0, None, 0, None, 0) == Status.success
        assert qnnp.run_operator_status(op) == Status.success
        assert np.all(from_device(e) == 0)
        for a, b, y in ((None, d, e), (d, None, e), (d, e, None)):
            assert setup(op, 3, 5, a, c, b, c, y, c) == Status.invalid_parameter
        for sa, sb, sy in ((c - 1, c, c), (c, c - 1, c), (c, c, c - 1), (0, c, c)):
            assert setup(op, 3, 5, d, sa, e, sb, e.data_ptr() + 1024, sy) == Status.invalid_parameter
        # the row limit, by status alone: each factor, their product, a product that wraps 64 bits
        for b_rows, per in ((2 ** 31, 1), (1, 2 ** 31), (65536, 32768), (2 ** 33, 2 ** 31), (2 ** 64 - 1, 2 ** 64 - 1),
                            (2 ** 32, 2 ** 32)):
            assert setup(op, b_rows, per, d, c, e, c, d, c) == Status.unsupported_parameter, (b_rows, per)
        # permitted: in place on a (always), in place on b (element-wise), a and b overlapping any way
        assert setup(op, 3, 5, d, 24, e, c, d, 24) == Status.success
        assert setup(op, 15, 1, e, c, d, 24, d, 24) == Status.success
        assert setup(op, 15, 1, d, c, d, c, e, c) == Status.success                         # the square
        assert setup(op, 15, 1, d, c, d, c, d, c) == Status.success                         # the square in place
        assert setup(op, 15, 1, d, c, base + 7, c, e, c) == Status.success                  # a and b shifted
        assert setup(op, 3, 5, d, c, base + 16, 32, e, c) == Status.success                 # b inside a
        assert setup(op, 3, 5, d, c, e, c, base + 15 * c, c) == Status.success              # product right behind a
        # refused: the product on a broadcast b; partial overlaps; the same base with another stride
        refused = [(3, 5, e, c, d, c, d, c), (3, 5, d, c, e, c, base + 1, c), (3, 5, d, c, e, c, base + 15 * c - 1, c),
                   (3, 5, d, c, e, c, d, c + 1), (3, 5, d, c + 1, e, c, d, c), (15, 1, e, c, d, c, base + 1, c),
                   (15, 1, e, c, d, c, d, c + 4), (15, 1, e, c, d, c + 4, d, c), (3, 5, base + 64, c, d, c, base + 32, c),
                   (3, 1, e, c, d, c, base + 2 * c, c)]
        d[4096:].zero_()
        assert setup(op, 3, 5, d, c, e, c, base + 4096, c) == Status.success
        qnnp.run_operator(op)
        want = from_device(d)
        for args in refused:
            # a refused setup leaves the last one runnable
            assert setup(op, *args) == Status.invalid_parameter, args
            d[4096:].zero_()
            assert qnnp.run_operator_status(op) == Status.success
            assert np.array_equal(from_device(d), want), args
        # a valid (3, 1) geometry next to those: b's span ends before the product starts
        assert setup(op, 3, 1, e, c, d, c, base + 3 * c, c) == Status.success
        # the setups of other operator kinds refuse a multiply operator, and the multiply setup refuses theirs
        add = qnnp.create_add_nc_q8(c, 0, 1.0, 0, 1.0, 0, 1.0, 0, 255)
        table = qnnp.create_hardsigmoid_nc_q8(c, 121, 0.05, 0, 1 / 256, 0, 255)
        clamp = qnnp.create_clamp_nc_u8(c, 0, 255)
        try:
            for other in (add, table, clamp):
                assert setup(other, 3, 5, d, c, e, c, base + 4096, c) == Status.invalid_parameter
            assert setup(None, 3, 5, d, c, e, c, base + 4096, c) == Status.invalid_parameter
            assert qnnp.setup_add_nc_q8_status(op, 15, d, c, e, c, base + 4096, c) == Status.invalid_parameter
            assert qnnp.setup_lut_nc_x8_status(op, 15, d, c, e, c) == Status.invalid_parameter
            assert qnnp.setup_sigmoid_nc_q8_status(op, 15, d, c, e, c) == Status.invalid_parameter
            assert qnnp.setup_clamp_nc_u8_status(op, 15, d, c, e, c) == Status.invalid_parameter
            # hardsigmoid is a table operator: any table setup takes it
            assert qnnp.setup_lut_nc_x8_status(table, 15, d, c, e, c) == Status.success
            assert qnnp.setup_sigmoid_nc_q8_status(table, 15, d, c, e, c) == Status.success
        finally:
            for other in (add, table, clamp):
                qnnp.delete_operator(other)
    finally:
        qnnp.delete_operator(op)


def _host_pointers_async_mode_and_resetup(qnnp):
    import torch
    # host pointers for all three tensors, dense and strided, and in place
    for strides in ((0, 0, 0), (45, 41, 47)):
        s = mul.Shape(40, 3, 5, *strides)
        a, b, y = mul.tensors(f"host/{strides}", s)
        op = qnnp.create_multiply_nc_q8(s.channels, *mul.MID.args())
        try:
            want = mul.expected(mul.MID, s, a, b, y)
            a0, b0 = a.copy(), b.copy()
            assert mul.setup_status(qnnp, op, s, a, b, y) == Status.success
            qnnp.run_operator(op)
            _differences(y, want, f"host pointers {strides}")
            assert np.array_equal(a, a0) and np.array_equal(b, b0)
            # mixed: b on the device
            y[...] = mul.FILL
            d_b = to_device(b)
            assert mul.setup_status(qnnp, op, s, a, d_b, y) == Status.success
            qnnp.run_operator(op)
            _differences(y, want, f"host a and product, device b {strides}")
            s_in = mul.Shape(40, 3, 5, strides[0], strides[1], strides[0])
            want = mul.expected(mul.MID, s_in, a, b, a)
            assert mul.setup_status(qnnp, op, s_in, a, b, a) == Status.success
            qnnp.run_operator(op)
            _differences(a, want, f"host pointers in place {strides}")
        finally:
            qnnp.delete_operator(op)
    # async mode with three runs, timing, re-setup to a smaller geometry
    s = mul.Shape(96, 4, 28 * 28)
    a, b, y = mul.tensors("async", s)
    want = mul.expected(mul.MID, s, a, b, y)
    op = qnnp.create_multiply_nc_q8(s.channels, *mul.MID.args())
    d_a, d_b, d_y = to_device(a), to_device(b), to_device(y)
    try:
        qnnp.set_async(True)
        assert mul.setup_status(qnnp, op, s, d_a, d_b, d_y) == Status.success
        for streaming in (1, 0, -1):
            qnnp.operator_set_streaming_stores(op, streaming)
            d_y.fill_(mul.FILL)
            for _ in range(3):
                qnnp.run_operator(op)
            qnnp.synchronize()
            torch.cuda.synchronize()
            _differences(from_device(d_y), want, f"async runs, streaming {streaming}")
        qnnp.set_async(False)
        assert qnnp.time_operator(op, 1, 3) > 0.0
        _differences(from_device(d_y), want, "after timing")
        small = mul.Shape(96, 2, 5)
        d_y.fill_(mul.FILL)
        assert mul.setup_status(qnnp, op, small, d_a, d_b, d_y) == Status.success
        qnnp.run_operator(op)
        got = from_device(d_y)
        _differences(got[:960], mul.expected(mul.MID, small, a, b, y)[:960], "re-setup to a smaller geometry")
        assert np.all(got[960:] == mul.FILL)
        # in place on a with the first geometry
        assert mul.setup_status(qnnp, op, mul.Shape(96, 4, 28 * 28), d_a, d_b, d_a) == Status.success
        qnnp.run_operator(op)
        _differences(from_device(d_a), want, "in place after re-setup")
    finally:
        qnnp.set_async(False)
        qnnp.delete_operator(op)


# ---- 5. tables ---------------------------------------------------------------------------------------------------
class _Identity:
    """the identity input on the device and an output to read a product table into (as tests/test_gpu_lut.py)"""

    def __init__(self):
        self.x = to_device(np.arange(256, dtype=np.uint8))
        self.y = to_device(np.zeros(256, np.uint8))

    def table(self, qnnp, create, args):
        st, op = create(256, *args)
        assert st == Status.success, (args, st)
        try:
            self.y.zero_()
            assert qnnp.setup_lut_nc_x8_status(op, 1, self.x, 256, self.y, 256) == Status.success
            qnnp.run_operator(op)
            return from_device(self.y)
        finally:
            qnnp.delete_operator(op)


SCALES = (0.01, 0.1, 1.25, 10.0)
OUTPUTS = ((0, 1.0 / 256), (133, 0.75), (7, 0.02), (255, 3.0), (64, 1.0 / 64))
CLAMPS = ((0, 255), (3, 250), (128, 255), (0, 128))


def _hardswish_and_hardsigmoid_tables(qnnp):
    """input zero points 0 .. 255 at four scales, each with one of the five output quantizations x four clamps in turn
    (hardsigmoid has the one output quantization it supports), so every combination meets its share of the zero points"""
    identity = _Identity()
    for kind, create, formula, outputs in (("hardswish", qnnp.create_hardswish_nc_q8_status, mul.hardswish_table, OUTPUTS),
                                           ("hardsigmoid", qnnp.create_hardsigmoid_nc_q8_status, mul.hardsigmoid_table, OUTPUTS[:1])):
        combos = [(o, c) for o in outputs for c in CLAMPS]
        used = set()
        for izp in range(256):
            for si, scale in enumerate(SCALES):
                (ozp, oscale), clamp = combos[(izp + si) % len(combos)]
                used.add(((ozp, oscale), clamp))
                args = (izp, scale, ozp, oscale) + clamp
                got, want = identity.table(qnnp, create, args), formula(*args)
                if not np.array_equal(got, want):
                    bad = np.flatnonzero(got != want)
                    raise AssertionError(f"{kind} table for {args}: {bad.size} entries differ, first at {bad[:4]}: "
                                         f"got {got[bad[:4]]}, want {want[bad[:4]]}")
        assert len(used) == len(combos)
    # the tables are not trivial: an unsaturated hardsigmoid and a hardswish with its dip below the zero point
    t = mul.hardsigmoid_table(128, 0.02, 0, 1.0 / 256, 0, 255)
    assert np.unique(t).size > 200
    t = mul.hardswish_table(121, 0.05, 133, 0.04, 0, 255)
    assert t.min() < 133 and t.max() == 255 and np.unique(t).size > 100


S = 1.0 / 256
# (channels, input zp, input scale, output zp, output scale, min, max) -> (hardswish, hardsigmoid), in sigmoid.c's order
TABLE_CREATE = [
    ((8, 121, 0.75, 0, S, 0, 255), Status.success, Status.success),
    ((2 ** 31 - 1, 255, 100.0, 0, S, 254, 255), Status.success, Status.success),
    ((0, 121, 0.75, 0, S, 0, 255), Status.invalid_parameter, Status.invalid_parameter),
    ((8, 121, 0.0, 0, S, 0, 255), Status.invalid_parameter, Status.invalid_parameter),
    ((8, 121, -1.0, 0, S, 0, 255), Status.invalid_parameter, Status.invalid_parameter),
    ((8, 121, INF, 0, S, 0, 255), Status.invalid_parameter, Status.invalid_parameter),
    ((8, 121, NAN, 0, S, 0, 255), Status.invalid_parameter, Status.invalid_parameter),
    ((8, 121, 1e-40, 0, S, 0, 255), Status.invalid_parameter, Status.invalid_parameter),
    ((8, 121, 0.75, 0, 0.0, 0, 255), Status.invalid_parameter, Status.invalid_parameter),
    ((8, 121, 0.75, 0, INF, 0, 255), Status.invalid_parameter, Status.invalid_parameter),
    ((8, 121, 0.75, 0, S, 100, 100), Status.invalid_parameter, Status.invalid_parameter),
    ((8, 121, 0.75, 0, S, 200, 100), Status.invalid_parameter, Status.invalid_parameter),
    ((8, 121, 0.75, 7, 0.5, 200, 100), Status.invalid_parameter, Status.invalid_parameter),
    ((2 ** 31, 121, 0.75, 0, S, 200, 100), Status.invalid_parameter, Status.invalid_parameter),
    ((2 ** 31, 121, 0.75, 0, S, 0, 255), Status.unsupported_parameter, Status.unsupported_parameter),
    ((8, 121, 0.75, 0, 0.5, 0, 255), Status.success, Status.unsupported_parameter),
    ((8, 121, 0.75, 0, S * 2, 0, 255), Status.success, Status.unsupported_parameter),
    ((8, 121, 0.75, 1, S, 0, 255), Status.success, Status.unsupported_parameter),
    ((8, 121, 0.75, 255, 0.5, 0, 255), Status.success, Status.unsupported_parameter)]


def _table_create_statuses(qnnp):
    for args, swish, sigmoid in TABLE_CREATE:
        for create, want in ((qnnp.create_hardswish_nc_q8_status, swish), (qnnp.create_hardsigmoid_nc_q8_status, sigmoid)):
            st, op = create(*args)
            if op:
                qnnp.delete_operator(op)
            assert st == want and bool(op) == (want == Status.success), (args, st, want)


# ---- 6. a squeeze-and-excite block as one hipGraph -----------------------------------------------------------------
def _squeeze_and_excite_block_as_one_graph(qnnp):
    """x [3 * 49][24] -> global average pooling -> FC 24 -> 8 with the ReLU as its output_min -> FC 8 -> 24 ->
    hardsigmoid -> x * s in place on x (a_rows_per_b_row = 49), chained on device buffers, captured once, replayed twice"""
    import torch
    batch, pixels, c, squeeze = 3, 49, 24, 8
    rng = np.random.default_rng(mul._seed("se_block"))
    x = rng.integers(0, 256, size=batch * pixels * c, dtype=np.uint8)
    x_zp, x_scale = 121, 0.05
    # expectations, stage by stage
    pooled = np.full(batch * c, mul.FILL, np.uint8)
    pool_zp, pool_scale = 119, 0.04
    o1.global_average_pooling_q8(batch, pixels, c, x_zp, x_scale, pool_zp, pool_scale, 0, 255, x, c, pooled, c)
    k1 = rng.integers(0, 256, size=(squeeze, c), dtype=np.uint8)
    b1 = rng.integers(-2000, 2001, size=squeeze, dtype=np.int32)
    k2 = rng.integers(0, 256, size=(c, squeeze), dtype=np.uint8)
    b2 = rng.integers(-2000, 2001, size=c, dtype=np.int32)
    fc1 = FcCase("se_fc1", batch, c, squeeze, izp=pool_zp)
    _, (scale1, zp1) = fc_expected(fc1, pooled, k1, b1)
    fc1 = FcCase("se_fc1", batch, c, squeeze, izp=pool_zp, qmin=zp1)       # the ReLU: output_min = the zero point
    mid, (scale1, zp1) = fc_expected(fc1, pooled, k1, b1)
    assert fc1.qmin == zp1 and mid.min() == zp1 and np.unique(mid).size > 4
    fc2 = FcCase("se_fc2", batch, squeeze, c, izp=zp1)
    gate_in, (scale2, zp2) = fc_expected(fc2, mid, k2, b2)
    # 0.011 per step keeps x + 3 inside (0, 6) wherever the zero point lies (255 * 0.011 < 3): not saturated
    hs_args = (zp2, 0.011, 0, 1.0 / 256, 0, 255)
    table = mul.hardsigmoid_table(*hs_args)
    gate = table[gate_in]
    assert np.unique(gate).size >= 8 and gate.min() > 0 and gate.max() < 255, np.unique(gate)
    q = mul.Quant(x_zp, x_scale, 0, 1.0 / 256, 133, 0.04)
    s = mul.Shape(c, batch, pixels)
    want = mul.expected(q, s, x, gate, x)
    assert np.unique(want).size > 64

    ops = []
    try:
        gap = qnnp.create_global_average_pooling_nwc_q8(c, x_zp, x_scale, pool_zp, pool_scale, 0, 255, 0)
        ops.append(gap)
        op1 = qnnp.create_fully_connected_nc_q8(c, squeeze, fc1.izp, 1.0, fc1.kzp, 1.0, k1, b1, zp1, float(scale1), fc1.qmin, 255, 0)
        ops.append(op1)
        op2 = qnnp.create_fully_connected_nc_q8(squeeze, c, fc2.izp, 1.0, fc2.kzp, 1.0, k2, b2, zp2, float(scale2), 0, 255, 0)
        ops.append(op2)
        hs = qnnp.create_hardsigmoid_nc_q8(c, *hs_args)
        ops.append(hs)
        m = qnnp.create_multiply_nc_q8(c, *q.args())
        ops.append(m)
        d_x0 = to_device(x)
        d_x = to_device(x)
        d_pool, d_mid, d_fc2, d_gate = (to_device(np.full(n, mul.FILL, np.uint8)) for n in (batch * c, batch * squeeze, batch * c, batch * c))
        qnnp.setup_global_average_pooling_nwc_q8(gap, batch, pixels, d_x, c, d_pool, c)
        qnnp.setup_fully_connected_nc_q8(op1, batch, d_pool, c, d_mid, squeeze)
        qnnp.setup_fully_connected_nc_q8(op2, batch, d_mid, squeeze, d_fc2, c)
        qnnp.setup_lut_nc_x8(hs, batch, d_fc2, c, d_gate, c)
        qnnp.setup_multiply_nc_q8(m, batch, pixels, d_x, c, d_gate, c, d_x, c)
        qnnp.graph_begin()
        try:
            for op in ops:
                qnnp.run_operator(op)
            # neither create nor setup can be recorded
            assert qnnp.create_multiply_nc_q8_status(c, *q.args())[0] == Status.invalid_parameter
            assert qnnp.setup_multiply_nc_q8_status(m, batch, pixels, d_x, c, d_gate, c, d_x, c) == Status.invalid_parameter
        finally:
            graph = qnnp.graph_end()
        assert np.array_equal(from_device(d_x), x), "nothing runs during the capture"
        try:
            for rep in range(2):
                d_x.copy_(d_x0)
                for t in (d_pool, d_mid, d_fc2, d_gate):
                    t.fill_(mul.FILL)
                torch.cuda.synchronize()
                qnnp.graph_launch(graph)
                qnnp.graph_synchronize(graph)
                _differences(from_device(d_pool), pooled, f"replay {rep}: pooling")
                _differences(from_device(d_mid), mid, f"replay {rep}: FC 24 -> 8 with ReLU")
                _differences(from_device(d_fc2), gate_in, f"replay {rep}: FC 8 -> 24")
                _differences(from_device(d_gate), gate, f"replay {rep}: hardsigmoid")
                _differences(from_device(d_x), want, f"replay {rep}: x * s ({qnnp.operator_kernel(m)})")
        finally:
            qnnp.graph_destroy(graph)
    finally:
        for op in ops:
            qnnp.delete_operator(op)


# ---- the one test ------------------------------------------------------------------------------------------------
# All of the above under ONE test id, as tests/test_gpu_softargmax.py groups its checks: the whole file runs in a few
# seconds and the GPU tier's count of test ids grows by one. A failure names the part, and the part names the case, the
# setup and the kernel.
PARTS = [_every_pair_of_bytes_in_every_requantization_class,                                       # 1
         _shapes_dense_and_strided, _base_misalignments_for_short_rows, _kernel_follows_alignment,   # 2
         _more_than_one_pass_of_each_loop, _broadcast_boundary,
         _nothing_is_written_outside_the_product, _in_place_and_the_square,                          # 3
         _create_statuses, _setup_statuses_and_overlaps, _host_pointers_async_mode_and_resetup,      # 4
         _hardswish_and_hardsigmoid_tables, _table_create_statuses,                                  # 5
         _squeeze_and_excite_block_as_one_graph]                                                     # 6


def test_multiply_hardswish_hardsigmoid(qnnp):
    for part in PARTS:
        try:
            part(qnnp)
        except AssertionError as e:
            raise AssertionError(f"{part.__name__.lstrip('_')}: {e}") from e
