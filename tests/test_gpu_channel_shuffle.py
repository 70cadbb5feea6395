"""GPU tier of channel shuffle (hip/x8shuffle.hip behind channel-shuffle.c).

Every case of tests/_x8.py -- the restated reference test list (test/channel-shuffle.cc), the extra cases and the
ShuffleNet shapes of the reference's bench lists -- runs on the MI355X on device buffers (host buffers where the case
says so) and must give the bytes of the COMPILED REFERENCE (oracle/_ref/libqnnpack_ref.so, on the host) and of the numpy
model, including the FILL bytes between strided pixels. Then: the kernel each alignment class takes, no byte written
outside the output tensor, the status codes against the reference's, async mode and re-setup.
"""
import numpy as np
import pytest

import _x8 as x8
from _gpu import Guarded, from_device, to_device
from oracle import ref
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

_REF_GROUPS = {}
for _c in x8.reference_shuffle_cases():
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


@pytest.mark.parametrize("case", [c for c in x8.extra_cases() if c.kind == "shuffle"], ids=lambda c: c.name)
def test_extra_cases(qnnp, reference, case):
    x8.check(qnnp, reference, case, to_device, from_device)


@pytest.mark.parametrize("case", [c for c in x8.bench_cases(1) if c.kind == "shuffle"], ids=lambda c: c.name)
def test_bench_shapes_batch_1(qnnp, reference, case):
    x8.check(qnnp, reference, case, to_device, from_device)


BATCH_128 = ["ShuffleNetV1G2_g2_gc25_28x28", "ShuffleNetV1G3_g3_gc20_28x28", "ShuffleNetV1G8_g8_gc12_28x28",
             "ShuffleNetV1G4_g4_gc68_14x14", "ShuffleNetV2X05_g2_gc24_56x56", "ShuffleNetV2X10_g2_gc58_28x28",
             "ShuffleNetV2X20_g2_gc488_7x7"]


@pytest.mark.parametrize("name", BATCH_128)
def test_bench_shapes_batch_128(qnnp, reference, name):
    case = {c.name: c for c in x8.bench_cases(128)}[f"shuffle/bench/{name}/b128"]
    x8.check(qnnp, reference, case, to_device, from_device)


@pytest.mark.parametrize("groups,gc,stride,misalign,kernel", [
    (2, 64, 0, 0, "x8_shuffle_g2_x16"), (2, 24, 0, 0, "x8_shuffle_g2_x4"), (2, 64, 0, 4, "x8_shuffle_g2_x4"),
    (2, 64, 132, 0, "x8_shuffle_g2_x4"), (4, 32, 0, 0, "x8_shuffle_g4_x16"), (4, 68, 0, 0, "x8_shuffle_g4_x4"),
    (2, 64, 0, 2, "x8_shuffle_lds"), (2, 58, 0, 0, "x8_shuffle_lds"), (3, 20, 0, 0, "x8_shuffle_lds"),
    (8, 12, 0, 0, "x8_shuffle_lds"), (4, 16, 66, 0, "x8_shuffle_lds"), (2, 20000, 0, 0, "x8_shuffle_g2_x16"),
    (3, 11000, 0, 0, "x8_shuffle_gather")])
def test_kernel_follows_alignment(qnnp, reference, groups, gc, stride, misalign, kernel):
    case = x8.X8Case("shuffle", f"shuffle/path/g{groups}_gc{gc}_s{stride}_m{misalign}", 5, groups, gc,
                     in_stride=stride, misalign_in=misalign)
    assert x8.check(qnnp, reference, case, to_device, from_device) == kernel


@pytest.mark.parametrize("groups,gc,si,so,offset_in,offset_out", [
    (2, 64, 0, 0, 0, 0), (2, 24, 0, 0, 4, 12), (4, 68, 0, 0, 0, 0), (3, 20, 0, 0, 1, 3), (8, 12, 97, 101, 2, 1),
    (5, 7, 0, 0, 3, 2), (3, 11000, 0, 0, 1, 1)])
def test_nothing_written_outside_the_output(qnnp, groups, gc, si, so, offset_in, offset_out):
    case = x8.X8Case("shuffle", f"shuffle/guarded/g{groups}_gc{gc}", 11, groups, gc, in_stride=si, out_stride=so)
    x = x8.input_tensor(case)
    gx, gy = Guarded(x, offset_in), Guarded(x8.output_tensor(case), offset_out)
    op = qnnp.create_channel_shuffle_nc_x8(groups, gc)
    try:
        assert x8.setup_status(qnnp, case, op, case.batch, gx, gy) == Status.success
        qnnp.run_operator(op)
        assert np.array_equal(gy.read(), x8.expected(case)[0])
        gy.assert_intact(case.name)
        gx.assert_intact(case.name + " (input)")
    finally:
        qnnp.delete_operator(op)


# (groups, group_channels) -> both libraries must answer the same status (reference src/channel-shuffle.c:35-49)
CREATE = [(0, 4), (1, 4), (2, 0), (1, 0), (2, 1), (3, 99), (1000, 1)]


@pytest.mark.parametrize("args", CREATE)
def test_create_statuses_match_the_reference(qnnp, reference, args):
    got = [lib.create_channel_shuffle_nc_x8_status(*args) for lib in (qnnp, reference)]
    for lib, (st, op) in zip((qnnp, reference), got):
        if op:
            lib.delete_operator(op)
    assert got[0][0] == got[1][0], (args, got[0][0], got[1][0])


def test_setup_statuses(qnnp, reference):
    x = np.zeros(4096, np.uint8)
    y = np.zeros(4096, np.uint8)
    for lib in (qnnp, reference):            # reference src/channel-shuffle.c:81-96: batch 0 succeeds and does nothing
        op = lib.create_channel_shuffle_nc_x8(2, 8)
        assert lib.setup_channel_shuffle_nc_x8_status(op, 0, None, 0, None, 0) == Status.success
        assert lib.run_operator_status(op) == Status.success
        assert lib.setup_channel_shuffle_nc_x8_status(op, 3, x, 16, y, 16) == Status.success
        assert lib.run_operator_status(op) == Status.success
        lib.delete_operator(op)
    # where the reference checks nothing and would go out of range, the product refuses (include/qnnpack_gfx950.h)
    op = qnnp.create_channel_shuffle_nc_x8(2, 8)
    d = to_device(np.zeros(4096, np.uint8))
    try:
        assert qnnp.setup_channel_shuffle_nc_x8_status(op, 3, None, 16, y, 16) == Status.invalid_parameter
        assert qnnp.setup_channel_shuffle_nc_x8_status(op, 3, x, 16, None, 16) == Status.invalid_parameter
        assert qnnp.setup_channel_shuffle_nc_x8_status(op, 3, x, 15, y, 16) == Status.invalid_parameter
        assert qnnp.setup_channel_shuffle_nc_x8_status(op, 3, x, 16, y, 15) == Status.invalid_parameter
        assert qnnp.setup_channel_shuffle_nc_x8_status(op, 3, d, 16, d, 16) == Status.invalid_parameter
        assert qnnp.setup_channel_shuffle_nc_x8_status(op, 3, d, 16, d.data_ptr() + 40, 16) == Status.invalid_parameter
        assert qnnp.setup_channel_shuffle_nc_x8_status(op, 3, d, 16, d.data_ptr() + 48, 16) == Status.success
        assert qnnp.setup_channel_shuffle_nc_x8_status(op, 2 ** 31, d, 16, d, 16) == Status.unsupported_parameter
    finally:
        qnnp.delete_operator(op)
    st, op = qnnp.create_channel_shuffle_nc_x8_status(65536, 65536)
    assert st == Status.unsupported_parameter and not op


def test_async_mode_and_resetup(qnnp):
    import torch
    case = x8.X8Case("shuffle", "shuffle/async", 4 * 28 * 28, 2, 58)
    x = x8.input_tensor(case)
    want = x8.expected(case)[0]
    op = qnnp.create_channel_shuffle_nc_x8(2, 58)
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
        # fewer pixels on the same buffers: only their bytes change
        d_y.fill_(x8.FILL)
        assert x8.setup_status(qnnp, case, op, 5, d_x, d_y) == 0
        qnnp.run_operator(op)
        got = from_device(d_y)
        assert np.array_equal(got[:5 * 116], want[:5 * 116]) and np.all(got[5 * 116:] == x8.FILL)
        assert x8.setup_status(qnnp, case, op, case.batch, d_x, d_y) == 0
        qnnp.run_operator(op)
        assert np.array_equal(from_device(d_y), want), "second run after re-setup"
    finally:
        qnnp.set_async(False)
        qnnp.delete_operator(op)
