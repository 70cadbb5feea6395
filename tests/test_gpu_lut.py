"""GPU tier of sigmoid, leaky ReLU and the byte lookup-table operator (hip/x8lut.hip behind lut.c, sigmoid.c, leaky-relu.c).

Every case of tests/_lut.py -- the restated reference test lists (test/sigmoid.cc, test/leaky-relu.cc), the heads and
tails of every piece width, strided and adjoining rows, more than one sweep of each kernel's loop, in place, host
pointers, re-setup -- runs on the MI355X on device buffers (host buffers where the case says so) and must give the bytes
of the COMPILED REFERENCE (oracle/_ref/libqnnpack_ref.so, on the host), including the FILL bytes between strided pixels.
Then: the tables of both operators over their parameter ranges, two permutation tables alive at once, the kernel each
alignment class takes, no byte written outside the output tensor, the status codes against the reference's, async mode,
re-setup, a hipGraph of a convolution and a sigmoid, and tensors past 2^31 and 2^32 bytes.
"""
import numpy as np
import pytest

import _large as lg
import _lut as lut
from _cases import ConvCase, conv_tensors
from _gpu import Guarded, from_device, to_device
from _runner import conv_expected
from oracle import ref
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

_REF_GROUPS = {}
for _c in lut.reference_sigmoid_cases() + lut.reference_leaky_relu_cases():
    _REF_GROUPS.setdefault(_c.name.rsplit("/", 1)[0], []).append(_c)


@pytest.fixture(scope="module")
def reference():
    if not ref.available():
        pytest.fail("oracle/_ref/libqnnpack_ref.so was not built (build() makes it where the reference tree exists)")
    return ref.lib()


# ---- the case lists against the reference ------------------------------------------------------------------------
# One test per group of checks, looping over its cases: a failure names the case (lut.check and the assertions below carry
# the case name, the setup and the kernel), and the suite's count of test ids stays small.
def test_case_lists_against_the_reference(qnnp, reference):
    """the restated reference test lists, the extra cases, 1 .. 49 bytes at output offsets 0 .. 15 for each piece width
    (every partial first and last piece), and more than one sweep of each kernel's loop"""
    assert len(_REF_GROUPS) == 18 + 13
    for test in sorted(_REF_GROUPS):
        for case in _REF_GROUPS[test]:
            lut.check(qnnp, reference, case, to_device, from_device)
    for case in lut.extra_cases():
        lut.check(qnnp, reference, case, to_device, from_device)
    for width in sorted(lut.DELTAS):
        for case in lut.flat_edge_cases(width):
            assert lut.check(qnnp, reference, case, to_device, from_device) == f"x8_lut_flat_x{width}", case.name
    for case in lut.sweep_cases():
        _more_than_one_sweep_of_the_loop(qnnp, reference, case)


def _more_than_one_sweep_of_the_loop(qnnp, reference, case):
    kernel = lut.check(qnnp, reference, case, to_device, from_device)
    width = int(kernel.rsplit("x", 1)[1])
    assert kernel == case.name.replace("sigmoid/x/sweep", "x8_lut").replace("table/x/sweep", "x8_lut"), kernel
    if "flat" in kernel:
        # the cases are sized for the MI355X's launch cap; a device with more compute units would make them one pass
        pass_pieces = qnnp.device_info()["compute_units"] * 16 * 256
        assert pass_pieces == lut.FLAT_PASS_PIECES and case.batch * case.channels > pass_pieces * width, case.name
    else:
        items = case.channels if width == 1 else (case.channels + 2 * width - 2) // width
        assert case.batch > lut.ROWS_PASS_GROUPS * (256 // items), case.name


# ---- tables ------------------------------------------------------------------------------------------------------
class _Identity:
    """the identity input on the device and an output to read a product table into"""

    def __init__(self):
        self.x = to_device(np.arange(256, dtype=np.uint8))
        self.y = to_device(np.zeros(256, np.uint8))

    def table(self, qnnp, case):
        st, op = lut.create(qnnp, case, channels=256)
        assert st == Status.success, (case, st)
        try:
            self.y.zero_()
            assert getattr(qnnp, lut._SETUP[case.kind])(op, 1, self.x, 256, self.y, 256) == Status.success
            qnnp.run_operator(op)
            return from_device(self.y)
        finally:
            qnnp.delete_operator(op)


def _assert_tables_equal(qnnp, reference, cases):
    identity = _Identity()
    for case in cases:
        got, want = identity.table(qnnp, case), lut.reference_table(reference, case)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{case.kind} table for {case.create_args()}: {bad.size} entries differ, first at "
                                 f"{bad[:4]}: got {got[bad[:4]]}, want {want[bad[:4]]}")


def _distinct(cases):
    seen = {}
    for c in cases:
        seen.setdefault((c.kind,) + c.create_args(), c)
    return list(seen.values())


def test_tables(qnnp, reference):
    """product and reference tables byte-equal on the identity input: the parameter sweeps of the reference's tests,
    sigmoid zero points 0 .. 255 at four scales, leaky ReLU slopes 1e-4 .. 1 against output zero points 0 .. 255 step 51;
    then two permutation tables alive at once"""
    for cases in (lut.reference_sigmoid_cases(), lut.reference_leaky_relu_cases()):
        cases = _distinct(cases)
        assert len(cases) >= 12
        _assert_tables_equal(qnnp, reference, cases)
    for scale in (0.01, 0.1, 1.25, 10.0):
        _assert_tables_equal(qnnp, reference, [lut.LutCase("sigmoid", "sweep", 1, 256, input_scale=scale, input_zero_point=zp)
                                               for zp in range(256)])
    _assert_tables_equal(qnnp, reference, [lut.LutCase("leaky", "sweep", 1, 256, slope=slope, output_zero_point=zp)
                                           for slope in (1e-4, 1e-3, 1e-2, 1e-1, 1.0) for zp in range(0, 256, 51)])
    _two_permutation_tables_alive_at_once(qnnp)


def _two_permutation_tables_alive_at_once(qnnp):
    """every wrong index, and a table taken from the other operator, changes a byte"""
    a = lut.LutCase("table", "table/two/a", 50, 77, in_stride=80, out_stride=96, table_seed=11)
    b = lut.LutCase("table", "table/two/b", 50, 77, in_stride=80, out_stride=96, table_seed=12)
    x = lut.input_tensor(a)
    ops = [lut.create(qnnp, c)[1] for c in (a, b)]
    try:
        d_x = to_device(x)
        outs = [to_device(lut.output_tensor(c)) for c in (a, b)]
        for c, op, d_y in zip((a, b), ops, outs):
            assert lut.setup_status(qnnp, c, op, c.batch, d_x, d_y) == Status.success
        for op in ops + ops[::-1]:
            qnnp.run_operator(op)
        for c, d_y in zip((a, b), outs):
            assert np.array_equal(from_device(d_y), lut.apply_table(c, lut.permutation(c.table_seed), x, c.batch)), c.name
        # the identity input gives each operator's own permutation back
        identity = _Identity()
        for c in (a, b):
            assert np.array_equal(identity.table(qnnp, c), lut.permutation(c.table_seed)), c.name
    finally:
        for op in ops:
            qnnp.delete_operator(op)


# ---- dispatch and guards -----------------------------------------------------------------------------------------
KERNEL_BY_ALIGNMENT = [   # (batch, channels, input stride, output stride, misalign in, out, in place, kernel)
    (9, 64, 0, 0, 0, 0, False, "x8_lut_flat_x16"), (9, 7, 0, 0, 3, 3, False, "x8_lut_flat_x16"),
    (9, 7, 0, 0, 0, 4, False, "x8_lut_flat_x4"), (9, 64, 0, 0, 1, 0, False, "x8_lut_flat_x1"),
    (9, 64, 0, 0, 2, 0, True, "x8_lut_flat_x16"), (9, 24, 40, 56, 0, 0, False, "x8_lut_rows_x16"),
    (9, 24, 40, 44, 0, 0, False, "x8_lut_rows_x4"), (9, 24, 41, 44, 0, 0, False, "x8_lut_rows_x1"),
    (9, 24, 41, 0, 1, 0, True, "x8_lut_rows_x16"), (9, 24, 40, 40, 0, 3, False, "x8_lut_rows_x1"),
    (9, 24, 40, 24, 0, 0, False, "x8_lut_rows_x16"), (9, 24, 28, 24, 0, 0, False, "x8_lut_rows_x4"),
    # one pixel is flat whatever the strides; the stride difference then does not count either
    (1, 24, 4099, 9000, 0, 0, False, "x8_lut_flat_x16"), (1, 24, 4099, 9000, 0, 12, False, "x8_lut_flat_x4"),
    (1, 24, 4099, 9000, 6, 1, False, "x8_lut_flat_x1")]
GUARDED = [   # (channels, input stride, output stride, offset of the input, of the output)
    (64, 0, 0, 0, 0), (7, 0, 0, 3, 3), (100, 0, 0, 1, 9), (100, 0, 0, 5, 1), (24, 41, 44, 2, 0), (24, 40, 56, 5, 5),
    (33, 50, 50, 7, 3), (24, 40, 24, 3, 3), (33, 37, 33, 1, 1), (7, 10, 7, 0, 15)]
GUARDED_IN_PLACE = [(64, 0, 0), (7, 0, 3), (24, 41, 1), (100, 116, 4), (33, 33, 15)]   # (channels, stride, offset)


def test_dispatch_and_guards(qnnp, reference):
    """the kernel of each alignment class; with guarded tensors at odd offsets nothing is written outside the output and
    the input stays intact, in place too"""
    for row in KERNEL_BY_ALIGNMENT:
        _kernel_follows_alignment(qnnp, reference, *row)
    for kind in ("table", "leaky"):
        for row in GUARDED:
            _nothing_written_outside_the_output(qnnp, reference, kind, *row)
    for kind in ("table", "sigmoid"):
        for row in GUARDED_IN_PLACE:
            _in_place_writes_nothing_outside(qnnp, reference, kind, *row)


def _kernel_follows_alignment(qnnp, reference, batch, channels, si, so, mi, mo, in_place, kernel):
    for kind in ("table", "sigmoid"):
        case = lut.LutCase(kind, f"{kind}/path/b{batch}_c{channels}_s{si}_{so}_m{mi}_{mo}_{in_place}", batch, channels,
                           in_stride=si, out_stride=so, misalign_in=mi, misalign_out=mo, in_place=in_place)
        assert lut.check(qnnp, reference, case, to_device, from_device) == kernel, case.name


def _nothing_written_outside_the_output(qnnp, reference, kind, channels, si, so, offset_in, offset_out):
    case = lut.LutCase(kind, f"{kind}/guarded/c{channels}_{si}_{so}_{offset_in}_{offset_out}", 13, channels, in_stride=si, out_stride=so)
    x = lut.input_tensor(case)
    gx, gy = Guarded(x, offset_in), Guarded(lut.output_tensor(case), offset_out)
    op = lut.create(qnnp, case)[1]
    try:
        assert lut.setup_status(qnnp, case, op, case.batch, gx, gy) == Status.success
        qnnp.run_operator(op)
        assert np.array_equal(gy.read(), lut.expected(reference, case)[0]), case.name
        gy.assert_intact(case.name)
        gx.assert_intact(case.name + " (input)")
        assert np.array_equal(gx.read(), x), f"{case.name}: the input changed"
    finally:
        qnnp.delete_operator(op)


def _in_place_writes_nothing_outside(qnnp, reference, kind, channels, stride, offset):
    case = lut.LutCase(kind, f"{kind}/guarded_in_place/c{channels}", 13, channels, in_stride=stride, in_place=True)
    g = Guarded(lut.input_tensor(case), offset)
    op = lut.create(qnnp, case)[1]
    try:
        assert lut.setup_status(qnnp, case, op, case.batch, g, g) == Status.success
        qnnp.run_operator(op)
        assert np.array_equal(g.read(), lut.expected(reference, case)[0]), case.name
        g.assert_intact(case.name)
    finally:
        qnnp.delete_operator(op)


# ---- API behaviour -----------------------------------------------------------------------------------------------
S = 1.0 / 256.0
# (channels, input zero point, input scale, output zero point, output scale, output_min, output_max): reference
# src/sigmoid.c:39-80
SIGMOID_CREATE = [(8, 121, 0.75, 0, S, 0, 255), (1, 0, 1e-3, 0, S, 0, 1), (8, 255, 100.0, 0, S, 254, 255),
                  (0, 121, 0.75, 0, S, 0, 255), (8, 121, 0.0, 0, S, 0, 255), (8, 121, -1.0, 0, S, 0, 255),
                  (8, 121, float("inf"), 0, S, 0, 255), (8, 121, float("nan"), 0, S, 0, 255), (8, 121, 1e-40, 0, S, 0, 255),
                  (8, 121, 0.75, 0, 0.0, 0, 255), (8, 121, 0.75, 0, float("inf"), 0, 255), (8, 121, 0.75, 0, S, 100, 100),
                  (8, 121, 0.75, 0, S, 200, 100), (8, 121, 0.75, 0, 0.5, 200, 100), (0, 121, 0.75, 7, 0.5, 0, 255),
                  (8, 121, 0.75, 0, 0.5, 0, 255), (8, 121, 0.75, 0, S * 2, 0, 255), (8, 121, 0.75, 1, S, 0, 255),
                  (8, 121, 0.75, 255, 0.5, 0, 255)]
# (channels, slope, input zero point, input scale, output zero point, output scale, output_min, output_max): reference
# src/leaky-relu.c:40-88
LEAKY_CREATE = [(8, 0.5, 121, 1.25, 133, 0.75, 0, 255), (1, 1.0, 0, 1.0, 255, 256.0, 0, 1), (8, 1e-6, 0, 255.0, 0, 1.0, 3, 4),
                (0, 0.5, 121, 1.25, 133, 0.75, 0, 255), (8, 0.0, 121, 1.25, 133, 0.75, 0, 255),
                (8, -0.5, 121, 1.25, 133, 0.75, 0, 255), (8, float("nan"), 121, 1.25, 133, 0.75, 0, 255),
                (8, 1e-40, 121, 1.25, 133, 0.75, 0, 255), (8, 1.0000001, 121, 1.25, 133, 0.75, 0, 255),
                (8, 2.0, 121, 1.25, 133, 0.75, 0, 255), (8, 0.5, 121, 0.0, 133, 0.75, 0, 255),
                (8, 0.5, 121, float("inf"), 133, 0.75, 0, 255), (8, 0.5, 121, 1.25, 133, 0.0, 0, 255),
                (8, 0.5, 121, 1.25, 133, -0.75, 0, 255), (8, 0.5, 121, 1.25, 133, 0.75, 9, 9),
                (8, 0.5, 121, 1.25, 133, 0.75, 200, 100), (8, 0.5, 121, 1.0, 133, 1000.0, 200, 100),
                (8, 0.5, 121, 1.0, 133, 257.0, 0, 255), (8, 0.5, 121, 1.0, 133, 256.0, 0, 255),
                (8, 0.5, 121, 256.0, 133, 1.0, 0, 255), (8, 0.5, 121, 255.9, 133, 1.0, 0, 255), (8, 0.5, 121, 1e30, 133, 1e-30, 0, 255)]


def test_api_behaviour(qnnp, reference):
    """create and setup statuses against the reference's and the product-only refusals, the setup limits, async mode
    with three runs, re-setup to a smaller batch, in place"""
    for which, rows in (("sigmoid", SIGMOID_CREATE), ("leaky_relu", LEAKY_CREATE)):
        for args in rows:
            _create_statuses_match_the_reference(qnnp, reference, which, args)
    _create_statuses_of_the_product_only_refusals(qnnp)
    _any_table_setup_takes_any_table_operator_and_no_other(qnnp)
    for kind in ("sigmoid", "leaky", "table"):
        _setup_statuses(qnnp, reference, kind)
        _setup_limits(qnnp, reference, kind)
        _async_mode_and_resetup(qnnp, reference, kind)


def _create_statuses_match_the_reference(qnnp, reference, which, args):
    got = [getattr(lib, f"create_{which}_nc_q8_status")(*args) for lib in (qnnp, reference)]
    for lib, (st, op) in zip((qnnp, reference), got):
        if op:
            lib.delete_operator(op)
    assert got[0][0] == got[1][0], (which, args, got[0][0], got[1][0])
    assert bool(got[0][1]) == (got[0][0] == Status.success), (which, args)


def _create_statuses_of_the_product_only_refusals(qnnp):
    table = lut.permutation(3)
    assert qnnp.create_lut_nc_x8_status(0, table)[0] == Status.invalid_parameter
    assert qnnp.create_lut_nc_x8_status(8, None)[0] == Status.invalid_parameter
    assert qnnp.create_lut_nc_x8_status(0, None)[0] == Status.invalid_parameter
    # channels beyond the kernels' index range
    assert qnnp.create_lut_nc_x8_status(2 ** 31, table)[0] == Status.unsupported_parameter
    assert qnnp.create_sigmoid_nc_q8_status(2 ** 31, 121, 0.75, 0, S, 0, 255)[0] == Status.unsupported_parameter
    assert qnnp.create_leaky_relu_nc_q8_status(2 ** 31, 0.5, 121, 1.25, 133, 0.75, 0, 255)[0] == Status.unsupported_parameter
    st, op = qnnp.create_lut_nc_x8_status(2 ** 31 - 1, table)
    assert st == Status.success
    qnnp.delete_operator(op)


def _setup_statuses(qnnp, reference, kind):
    case = lut.LutCase(kind, f"{kind}/setup", 3, 16)
    x = np.zeros(4096, np.uint8)
    y = np.zeros(4096, np.uint8)
    for lib in (qnnp, reference) if kind != "table" else (qnnp,):
        # reference sigmoid.c:138-141, leaky-relu.c:145-148: batch 0 succeeds and does nothing
        op = lut.create(lib, case)[1]
        assert lut.setup_status(lib, case, op, 0, None, None) == Status.success
        assert lib.run_operator_status(op) == Status.success
        assert lut.setup_status(lib, case, op, 3, x, y) == Status.success
        assert lib.run_operator_status(op) == Status.success
        assert lut.setup_status(lib, case, op, 3, x, x) == Status.success      # in place, host memory
        assert lib.run_operator_status(op) == Status.success
        lib.delete_operator(op)
    # where the reference checks nothing and would go out of range, the product refuses (include/qnnpack_gfx950.h)
    setup = getattr(qnnp, lut._SETUP[kind])
    op = lut.create(qnnp, case)[1]
    d = to_device(np.zeros(4096, np.uint8))
    try:
        assert qnnp.run_operator_status(op) == Status.invalid_parameter          # before any setup
        assert setup(op, 3, None, 16, y, 16) == Status.invalid_parameter
        assert setup(op, 3, x, 16, None, 16) == Status.invalid_parameter
        assert setup(op, 3, x, 15, y, 16) == Status.invalid_parameter
        assert setup(op, 3, x, 16, y, 15) == Status.invalid_parameter
        assert setup(op, 3, d, 16, d.data_ptr() + 1, 16) == Status.invalid_parameter
        assert setup(op, 3, d, 16, d, 17) == Status.invalid_parameter
        assert setup(op, 3, d, 16, d, 16) == Status.success          # in place
        assert setup(op, 3, d, 16, d.data_ptr() + 48, 16) == Status.success
        assert setup(op, 2 ** 31, d, 16, d, 16) == Status.unsupported_parameter
        assert setup(op, 3, d, 16, d.data_ptr() + 48, 16) == Status.success
        # a setup refused by its checks leaves the previous one runnable
        assert setup(op, 3, d, 15, d, 16) == Status.invalid_parameter
        assert qnnp.run_operator_status(op) == Status.success
    finally:
        qnnp.delete_operator(op)


def _any_table_setup_takes_any_table_operator_and_no_other(qnnp):
    x, y = to_device(np.arange(256, dtype=np.uint8)), to_device(np.zeros(256, np.uint8))
    op = qnnp.create_lut_nc_x8(256, lut.permutation(5))
    clamp = qnnp.create_clamp_nc_u8(256, 0, 255)
    try:
        assert qnnp.setup_sigmoid_nc_q8_status(op, 1, x, 256, y, 256) == Status.success
        qnnp.run_operator(op)
        assert np.array_equal(from_device(y), lut.permutation(5))
        assert qnnp.setup_lut_nc_x8_status(clamp, 1, x, 256, y, 256) == Status.invalid_parameter
        assert qnnp.setup_leaky_relu_nc_q8_status(clamp, 1, x, 256, y, 256) == Status.invalid_parameter
        assert qnnp.setup_clamp_nc_u8_status(op, 1, x, 256, y, 256) == Status.invalid_parameter
    finally:
        qnnp.delete_operator(op)
        qnnp.delete_operator(clamp)


def _async_mode_and_resetup(qnnp, reference, kind):
    import torch
    case = lut.LutCase(kind, f"{kind}/async", 4 * 28 * 28, 200)
    x = lut.input_tensor(case)
    want = lut.expected(reference, case)[0]
    op = lut.create(qnnp, case)[1]
    d_x, d_y = to_device(x), to_device(lut.output_tensor(case))
    try:
        qnnp.set_async(True)
        assert lut.setup_status(qnnp, case, op, case.batch, d_x, d_y) == 0
        for _ in range(3):
            qnnp.run_operator(op)
        qnnp.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(from_device(d_y), want), f"{kind}: async runs"
        qnnp.set_async(False)
        d_y.fill_(lut.FILL)
        assert lut.setup_status(qnnp, case, op, 5, d_x, d_y) == 0          # a smaller batch
        qnnp.run_operator(op)
        got = from_device(d_y)
        assert np.array_equal(got[:1000], want[:1000]) and np.all(got[1000:] == lut.FILL)
        # in place on the input buffer, with the first geometry
        assert lut.setup_status(qnnp, case, op, case.batch, d_x, d_x) == 0
        qnnp.run_operator(op)
        assert np.array_equal(from_device(d_x), want), f"{kind}: in place"
    finally:
        qnnp.set_async(False)
        qnnp.delete_operator(op)


def test_graph_of_a_convolution_and_a_sigmoid(qnnp, reference):
    import torch
    conv = ConvCase("lut_graph_conv", (14, 14), (3, 3), (1, 1, 1, 1), gic=16, goc=32, batch=2)
    inp, kernel, bias = conv_tensors(conv)
    mid_want, (oscale, ozp), (oh, ow) = conv_expected(conv, inp, kernel, bias)
    assert np.unique(mid_want).size > 16, "the convolution output should reach many entries of the table"
    case = lut.LutCase("sigmoid", "sigmoid/graph", conv.batch * oh * ow, 32, in_stride=conv.out_stride, out_stride=40,
                       input_scale=0.05, input_zero_point=int(ozp))
    want = lut.apply_table(case, lut.reference_table(reference, case), mid_want, case.batch)
    c_op = qnnp.create_convolution2d_nhwc_q8(
        conv.padding[0], conv.padding[1], conv.padding[2], conv.padding[3], conv.kernel_size[0], conv.kernel_size[1],
        conv.subsampling[0], conv.subsampling[1], conv.dilation[0], conv.dilation[1], conv.groups, conv.gic, conv.goc,
        conv.izp, 1.0, conv.kzp, 1.0, kernel, bias, ozp, float(oscale), conv.qmin, conv.qmax, 0)
    s_op = lut.create(qnnp, case)[1]
    d_in, d_mid, d_out = to_device(inp), to_device(np.full(mid_want.size, lut.FILL, np.uint8)), to_device(lut.output_tensor(case))
    try:
        qnnp.setup_convolution2d_nhwc_q8(c_op, conv.batch, 14, 14, d_in, conv.in_stride, d_mid, conv.out_stride)
        assert lut.setup_status(qnnp, case, s_op, case.batch, d_mid, d_out) == Status.success
        qnnp.graph_begin()
        try:
            qnnp.run_operator(c_op)
            qnnp.run_operator(s_op)
            # neither create nor setup can be recorded: both refuse and leave the operator as it was
            assert lut.create(qnnp, case)[0] == Status.invalid_parameter
            assert lut.setup_status(qnnp, case, s_op, case.batch, d_mid, d_out) == Status.invalid_parameter
        finally:
            graph = qnnp.graph_end()
        assert np.all(from_device(d_out) == lut.FILL), "nothing runs during the capture"
        try:
            for rep in range(2):
                d_mid.fill_(lut.FILL)
                d_out.fill_(lut.FILL)
                torch.cuda.synchronize()
                qnnp.graph_launch(graph)
                qnnp.graph_synchronize(graph)
                assert np.array_equal(from_device(d_mid), mid_want), f"replay {rep}: convolution"
                assert np.array_equal(from_device(d_out), want), f"replay {rep}: sigmoid"
        finally:
            qnnp.graph_destroy(graph)
    finally:
        qnnp.delete_operator(c_op)
        qnnp.delete_operator(s_op)


# ---- tensors past 2 GiB and 4 GiB --------------------------------------------------------------------------------
ROWS = 37           # rows per unit: not a multiple of the rows a workgroup takes, so units straddle workgroups
P = lg.PERIOD


@pytest.fixture()
def _release_device_memory():
    lg.free_memory()
    yield
    lg.free_memory()


def _large(qnnp, name, rows, channels, si, so, in_place, names):
    """`rows` rows through the permutation table operator on periodic tensors with marker units at the 2^31 / 2^32
    boundaries (_large.py), compared on the device"""
    case = lut.LutCase("table", name, rows, channels, in_stride=si, out_stride=so, in_place=in_place, table_seed=21)
    si, so = case.strides
    table = lut.permutation(case.table_seed)
    iu, ou = ROWS * si, ROWS * so
    ispan, ospan = (rows - 1) * si + channels, (rows - 1) * so + channels
    assert ispan > (1 << 32), name
    mk = lg.markers((rows + ROWS - 1) // ROWS, [(ispan, iu), (ospan, ou)])
    n = P + len(mk)
    ins = np.random.default_rng(lut._seed(name)).integers(0, 256, size=(n, iu), dtype=np.uint8)
    unit_case = lut.LutCase("table", name, n * ROWS, channels, in_stride=si, out_stride=so, in_place=in_place)
    flat = lut.apply_table(unit_case, table, ins.reshape(-1)[:(n * ROWS - 1) * si + channels], n * ROWS)
    outs = lg.units(flat, ou, n, lut.FILL)
    if in_place:
        outs.reshape(-1)[flat.size:] = ins.reshape(-1)[flat.size:]     # past the last row: the input's own bytes
    imarks = {i: ins[P + j] for j, i in enumerate(mk)}
    omarks = {i: outs[P + j] for j, i in enumerate(mk)}
    lg.require_memory((ispan if in_place else ispan + ospan) + 2 * lg.CHUNK, name)
    t_in = lg.Tensor(ispan, salt=3)
    t_in.fill_units(iu, ins[:P], imarks)
    if in_place:
        t_out = t_in
    else:
        t_out = lg.Tensor(ospan, salt=1)
        t_out.fill(lut.FILL)
    op = lut.create(qnnp, case)[1]
    try:
        assert lut.setup_status(qnnp, case, op, rows, t_in.view, t_out.view) == Status.success
        qnnp.run_operator(op)
        kernel = qnnp.operator_kernel(op)
    finally:
        qnnp.delete_operator(op)
    assert kernel in names, f"{name}: ran {kernel}, the case is there for {sorted(names)}"
    t_out.assert_units(ou, outs[:P], omarks, f"gfx950 {kernel} [{name}], output")
    if not in_place:
        t_in.assert_units(iu, ins[:P], imarks, f"gfx950 {kernel} [{name}]: the input was written")


def test_tensors_past_4g(qnnp, _release_device_memory):
    """a flat tensor whose span crosses 2^32 bytes, in place; then a strided one whose last rows start past 2^31 and 2^32
    bytes in both tensors"""
    _large(qnnp, "lut_flat_past_4g", (1 << 26) + 5, 64, 0, 0, True, {"x8_lut_flat_x16"})
    lg.free_memory()
    rows = ((1 << 32) // 58) + 3
    assert (rows - 1) * 61 > (1 << 32) and (rows - 1) * 64 > (1 << 32)
    _large(qnnp, "lut_58_past_4g", rows, 58, 61, 64, False, {"x8_lut_rows_x1"})


def _setup_limits(qnnp, reference, kind):
    """lut.c: batch <= 2^31 - 1 at setup, channels <= 2^31 - 1 at create; the operator still runs a valid setup afterwards"""
    case = lut.LutCase(kind, f"{kind}/limit", 33, 58)
    x = lut.input_tensor(case)
    want = lut.expected(reference, case)[0]
    assert lut.create(qnnp, case, channels=1 << 31)[0] == Status.unsupported_parameter
    op = lut.create(qnnp, case)[1]
    d_x, d_y = to_device(x), to_device(lut.output_tensor(case))
    try:
        assert lut.setup_status(qnnp, case, op, 1 << 31, d_x, d_y) == Status.unsupported_parameter
        assert lut.setup_status(qnnp, case, op, case.batch, d_x, d_y) == Status.success
        qnnp.run_operator(op)
        assert np.array_equal(from_device(d_y), want), kind
        assert np.array_equal(from_device(d_x), x), kind
    finally:
        qnnp.delete_operator(op)
