"""GPU tier of clamp (hip/x8shuffle.hip behind clamp.c).

Every clamp case of tests/_x8.py -- the restated reference test list (test/clamp.cc, its qmin / qmax sweeps included),
the extra cases (in place among them) and the bench shapes -- runs on the MI355X on device buffers (host buffers where
the case says so) and must give the bytes of the COMPILED REFERENCE (oracle/_ref/libqnnpack_ref.so, on the host) and of
the numpy model, including the FILL bytes between strided pixels. Then: the kernel each alignment class takes, no byte
written outside the output tensor, the status codes against the reference's, async mode and re-setup.
"""
import numpy as np
import pytest

import _x8 as x8
from _gpu import Guarded, from_device, to_device
from oracle import ref
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

_REF_GROUPS = {}
for _c in x8.reference_clamp_cases():
    _REF_GROUPS.setdefault(_c.name.rsplit("/", 1)[0], []).append(_c)


@pytest.fixture(scope="module")
def reference():
    if not ref.available():
        pytest.fail("oracle/_ref/libqnnpack_ref.so was not built (build() makes it where the reference tree exists)")
    return ref.lib()


@pytest.mark.parametrize("test", sorted(_REF_GROUPS))
def test_reference_test_list(qnnp, reference, test):
    for case in _REF_GROUPS[test]:
        x8.check(qnnp, reference, case, to_device, from_device)


@pytest.mark.parametrize("case", [c for c in x8.extra_cases() if c.kind == "clamp"], ids=lambda c: c.name)
def test_extra_cases(qnnp, reference, case):
    x8.check(qnnp, reference, case, to_device, from_device)


@pytest.mark.parametrize("case", [c for c in x8.bench_cases(1) if c.kind == "clamp"], ids=lambda c: c.name)
def test_bench_shapes_batch_1(qnnp, reference, case):
    x8.check(qnnp, reference, case, to_device, from_device)


@pytest.mark.parametrize("name", ["c24_112x112", "c200_28x28", "c1024_7x7"])
def test_bench_shapes_batch_128(qnnp, reference, name):
    case = {c.name: c for c in x8.bench_cases(128)}[f"clamp/bench/{name}/b128"]
    x8.check(qnnp, reference, case, to_device, from_device)


@pytest.mark.parametrize("channels,si,so,mi,mo,in_place,kernel", [
    (64, 0, 0, 0, 0, False, "u8_clamp_flat_x16"), (7, 0, 0, 3, 3, False, "u8_clamp_flat_x16"),
    (7, 0, 0, 0, 4, False, "u8_clamp_flat_x4"), (64, 0, 0, 1, 0, False, "u8_clamp_flat_x1"),
    (64, 0, 0, 2, 0, True, "u8_clamp_flat_x16"), (24, 40, 56, 0, 0, False, "u8_clamp_rows_x16"),
    (24, 40, 44, 0, 0, False, "u8_clamp_rows_x4"), (24, 41, 44, 0, 0, False, "u8_clamp_rows_x1"),
    (24, 41, 0, 1, 0, True, "u8_clamp_rows_x16"), (24, 40, 40, 0, 3, False, "u8_clamp_rows_x1")])
def test_kernel_follows_alignment(qnnp, reference, channels, si, so, mi, mo, in_place, kernel):
    case = x8.X8Case("clamp", f"clamp/path/c{channels}_s{si}_{so}_m{mi}_{mo}_{in_place}", 9, clamp_channels=channels,
                     in_stride=si, out_stride=so, qmin=50, qmax=150, misalign_in=mi, misalign_out=mo, in_place=in_place)
    assert x8.check(qnnp, reference, case, to_device, from_device) == kernel


@pytest.mark.parametrize("channels,si,so,offset_in,offset_out", [
    (64, 0, 0, 0, 0), (7, 0, 0, 3, 3), (100, 0, 0, 1, 9), (24, 41, 44, 2, 0), (24, 40, 56, 5, 5), (33, 50, 50, 7, 3)])
def test_nothing_written_outside_the_output(qnnp, channels, si, so, offset_in, offset_out):
    case = x8.X8Case("clamp", f"clamp/guarded/c{channels}", 13, clamp_channels=channels, in_stride=si, out_stride=so,
                     qmin=60, qmax=190)
    x = x8.input_tensor(case)
    gx, gy = Guarded(x, offset_in), Guarded(x8.output_tensor(case), offset_out)
    op = qnnp.create_clamp_nc_u8(channels, 60, 190)
    try:
        assert x8.setup_status(qnnp, case, op, case.batch, gx, gy) == Status.success
        qnnp.run_operator(op)
        assert np.array_equal(gy.read(), x8.expected(case)[0])
        gy.assert_intact(case.name)
        gx.assert_intact(case.name + " (input)")
    finally:
        qnnp.delete_operator(op)


@pytest.mark.parametrize("channels,stride,offset", [(64, 0, 0), (7, 0, 3), (24, 41, 1), (100, 116, 4)])
def test_in_place_writes_nothing_outside(qnnp, channels, stride, offset):
    case = x8.X8Case("clamp", f"clamp/guarded_in_place/c{channels}", 13, clamp_channels=channels, in_stride=stride,
                     qmin=60, qmax=190, in_place=True)
    x = x8.input_tensor(case)
    g = Guarded(x, offset)
    op = qnnp.create_clamp_nc_u8(channels, 60, 190)
    try:
        si = case.strides[0]
        assert qnnp.setup_clamp_nc_u8_status(op, case.batch, g, si, g, si) == Status.success
        qnnp.run_operator(op)
        assert np.array_equal(g.read(), x8.expected(case)[0])
        g.assert_intact(case.name)
    finally:
        qnnp.delete_operator(op)


# (channels, output_min, output_max) -> both libraries must answer the same status (reference src/clamp.c:35-48)
CREATE = [(0, 0, 255), (8, 200, 100), (0, 200, 100), (8, 100, 100), (1, 0, 0), (8, 255, 255), (8, 0, 255)]


@pytest.mark.parametrize("args", CREATE)
def test_create_statuses_match_the_reference(qnnp, reference, args):
    got = [lib.create_clamp_nc_u8_status(*args) for lib in (qnnp, reference)]
    for lib, (st, op) in zip((qnnp, reference), got):
        if op:
            lib.delete_operator(op)
    assert got[0][0] == got[1][0], (args, got[0][0], got[1][0])


def test_setup_statuses(qnnp, reference):
    x = np.zeros(4096, np.uint8)
    y = np.zeros(4096, np.uint8)
    for lib in (qnnp, reference):            # reference src/clamp.c:80-95: batch 0 succeeds and does nothing
        op = lib.create_clamp_nc_u8(16, 0, 6)
        assert lib.setup_clamp_nc_u8_status(op, 0, None, 0, None, 0) == Status.success
        assert lib.run_operator_status(op) == Status.success
        assert lib.setup_clamp_nc_u8_status(op, 3, x, 16, y, 16) == Status.success
        assert lib.run_operator_status(op) == Status.success
        lib.delete_operator(op)
    # where the reference checks nothing and would go out of range, the product refuses (include/qnnpack_gfx950.h)
    op = qnnp.create_clamp_nc_u8(16, 0, 6)
    d = to_device(np.zeros(4096, np.uint8))
    try:
        assert qnnp.setup_clamp_nc_u8_status(op, 3, None, 16, y, 16) == Status.invalid_parameter
        assert qnnp.setup_clamp_nc_u8_status(op, 3, x, 16, None, 16) == Status.invalid_parameter
        assert qnnp.setup_clamp_nc_u8_status(op, 3, x, 15, y, 16) == Status.invalid_parameter
        assert qnnp.setup_clamp_nc_u8_status(op, 3, x, 16, y, 15) == Status.invalid_parameter
        assert qnnp.setup_clamp_nc_u8_status(op, 3, d, 16, d.data_ptr() + 1, 16) == Status.invalid_parameter
        assert qnnp.setup_clamp_nc_u8_status(op, 3, d, 16, d, 17) == Status.invalid_parameter
        assert qnnp.setup_clamp_nc_u8_status(op, 3, d, 16, d, 16) == Status.success          # in place
        assert qnnp.setup_clamp_nc_u8_status(op, 3, d, 16, d.data_ptr() + 48, 16) == Status.success
        assert qnnp.setup_clamp_nc_u8_status(op, 2 ** 31, d, 16, d, 16) == Status.unsupported_parameter
    finally:
        qnnp.delete_operator(op)


def test_async_mode_and_resetup(qnnp):
    import torch
    case = x8.X8Case("clamp", "clamp/async", 4 * 28 * 28, clamp_channels=200, qmin=0, qmax=6)
    x = x8.input_tensor(case)
    want = x8.expected(case)[0]
    op = qnnp.create_clamp_nc_u8(200, 0, 6)
    d_x, d_y = to_device(x), to_device(x8.output_tensor(case))
    try:
        qnnp.set_async(True)
        assert x8.setup_status(qnnp, case, op, case.batch, d_x, d_y) == 0
        for _ in range(3):
            qnnp.run_operator(op)
        qnnp.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(from_device(d_y), want), "async runs"
        qnnp.set_async(False)
        d_y.fill_(x8.FILL)
        assert x8.setup_status(qnnp, case, op, 5, d_x, d_y) == 0
        qnnp.run_operator(op)
        got = from_device(d_y)
        assert np.array_equal(got[:1000], want[:1000]) and np.all(got[1000:] == x8.FILL)
        # in place on the input buffer, then back to the first geometry
        assert qnnp.setup_clamp_nc_u8_status(op, case.batch, d_x, 200, d_x, 200) == 0
        qnnp.run_operator(op)
        assert np.array_equal(from_device(d_x), want), "in place"
    finally:
        qnnp.set_async(False)
        qnnp.delete_operator(op)
