"""GPU tier of the softargmax operator (hip/q8softargmax.hip behind softargmax.c).

Every case of tests/_softargmax.py -- the restated reference test list (test/softargmax.cc), the channel counts around
every boundary of the lane-group and kernel selection, input and output misaligned by 0 .. 15 independently, saturating,
tied, constant (wrapped sums) and zero-sum rows, input scales, in place, host pointers, re-setup, more than one pass of
each kernel's loop -- runs on the MI355X on device buffers (host buffers where the case says so) and must give the bytes
of the COMPILED REFERENCE (oracle/_ref/libqnnpack_ref.so, on the host), including the FILL bytes in front of, between and
behind strided rows. The zero_sum cases hold rows on which the reference divides by zero; there the model of
tests/_softargmax.py, with the all-0 rule, is the truth, and the reference is never called (the fence of run_reference).
Then: the kernel each shape takes (the names carry the row-size thresholds), the status codes, a hipGraph replayed twice
on changed input, and row strides past 2^31 whose row offsets pass 2^32.
"""
import numpy as np
import pytest

import _large as lg
import _softargmax as sam
from _gpu import from_device, to_device
from oracle import ref
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

S = 1.0 / 256.0
X = sam.DEFAULT_SCALE


@pytest.fixture(scope="module")
def reference():
    if not ref.available():
        pytest.fail("oracle/_ref/libqnnpack_ref.so was not built (build() makes it where the reference tree exists)")
    return ref.lib()


def _check_all(qnnp, reference, cases):
    for case in cases:
        sam.check(qnnp, reference, case, to_device, from_device)


# ---- the case lists against the reference: a failure names the case, the setup and the kernel -------------------------
def _reference_test_list(qnnp, reference):
    cases = sam.reference_cases()
    assert len({c.name.rsplit("/", 1)[0] for c in cases}) == 12
    _check_all(qnnp, reference, cases)


def _selection_boundaries(qnnp, reference):
    """channels B - 1, B, B + 1 around every lane-group and kernel boundary and 1 .. 70, contiguous and strided; each
    runs the kernel the thresholds of tests/_softargmax.py name"""
    for case in sam.boundary_cases():
        kernel = sam.check(qnnp, reference, case, to_device, from_device)
        assert kernel == sam.kernel_name(case.channels, 1 if case.in_stride else 16), (case.name, kernel)


def _misaligned(qnnp, reference):
    for channels in sam.MISALIGNED_CHANNELS:
        for case in sam.misaligned_cases(channels):
            kernel = sam.check(qnnp, reference, case, to_device, from_device)
            assert kernel.endswith("_x16" if case.misalign_in == case.misalign_out else "_x1"), (case.name, kernel)


def _extra_cases(qnnp, reference):
    """row contents (saturation, ties, wrapped sums), input scales, in place, host pointers, re-setup, zero batch"""
    cases = [c for c in sam.extra_cases() if not c.name.startswith("x/boundary/")]
    assert len(cases) > 80
    _check_all(qnnp, reference, cases)


def _zero_sum_rows_give_zeros_and_disturb_nothing(qnnp, reference):
    """the product against the model: the reference is never called with these"""
    for case in sam.zero_sum_cases():
        with pytest.raises(sam.ZeroSumRow):
            sam.run_reference(reference, case)
        x = sam.input_tensor(case)
        assert sam.row_sums(case, x).tolist().count(0) == 1
        sam.check(qnnp, reference, case, to_device, from_device)
        # the neighbours of the zero-sum row are what the reference gives for them alone
        alone = sam.Case(case.name + "_neighbours", 2, case.channels)
        rows = x.reshape(3, case.channels)
        want = sam.run_reference(reference, alone, inputs=[np.concatenate([rows[0], rows[2]])])[0]
        got, _ = sam.run(qnnp, case, inputs=[x], to_device=to_device, from_device=from_device)
        body = got[0][sam.PAD:-sam.PAD].reshape(3, case.channels)
        assert np.array_equal(np.concatenate([body[0], body[2]]), want[sam.PAD:-sam.PAD]), case.name
        assert np.all(body[1] == 0), case.name
    # the same in place, strided and misaligned, through the single-byte kernels too
    for c in sam.ZERO_SUM_CHANNELS:
        for kw in (dict(in_place=True), dict(in_stride=c + 3, out_stride=c + 1), dict(in_place=True, misalign_in=5, in_stride=c + 16)):
            case = sam.Case(f"x/zero_sum/c{c}_{'_'.join(kw)}", 3, c, rows="zero_sum_middle", zero_sum=True, **kw)
            sam.check(qnnp, reference, case, to_device, from_device)


def _more_than_one_pass_of_each_loop(qnnp, reference):
    cus = qnnp.device_info()["compute_units"]
    for family, case in zip(("group", "lds", "stream"), sam.sweep_cases()):
        kernel = sam.check(qnnp, reference, case, to_device, from_device)
        assert kernel == sam.kernel_name(case.channels, 16) and family in kernel and family in case.name, kernel
        # the cases are sized for the MI355X's launch caps; a device with more compute units would make them one pass
        if family == "group":
            assert cus * 8 == sam.GROUP_PASS_BLOCKS
            assert case.batch > sam.GROUP_PASS_BLOCKS * (256 // sam.group_lanes(case.channels, 16))
        else:
            assert cus * 4 == sam.BLOCK_PASS_ROWS and case.batch > sam.BLOCK_PASS_ROWS


# ---- dispatch ------------------------------------------------------------------------------------------------------
def _each_kernel_family_is_named_on_the_shape_meant_for_it(qnnp, reference):
    g, l = sam.GROUP_MAX, sam.LDS_MAX
    rows = [   # (batch, channels, input stride, output stride, misalign in, out, in place, kernel)
        (9, 21, 0, 0, 0, 0, False, f"q8_softargmax_group{g}_x16"), (9, 21, 0, 0, 3, 3, False, f"q8_softargmax_group{g}_x16"),
        (9, 21, 0, 0, 0, 4, False, f"q8_softargmax_group{g}_x1"), (9, 21, 37, 53, 0, 0, False, f"q8_softargmax_group{g}_x16"),
        (9, 21, 37, 40, 0, 0, False, f"q8_softargmax_group{g}_x1"), (9, 21, 26, 0, 1, 0, True, f"q8_softargmax_group{g}_x16"),
        (9, g, 0, 0, 0, 0, False, f"q8_softargmax_group{g}_x16"), (9, g + 1, 0, 0, 0, 0, False, f"q8_softargmax_lds{l}_x16"),
        (9, 21841, 0, 0, 0, 1, False, f"q8_softargmax_lds{l}_x1"), (5, l, 0, 0, 0, 0, False, f"q8_softargmax_lds{l}_x16"),
        (5, l + 1, 0, 0, 0, 0, False, "q8_softargmax_stream_x16"), (5, l + 1, l + 2, l + 5, 0, 0, False, "q8_softargmax_stream_x1"),
        # one row: the stride difference does not count
        (1, 100, 4099, 9000, 0, 0, False, f"q8_softargmax_group{g}_x16"), (1, 100, 4099, 9000, 6, 1, False, f"q8_softargmax_group{g}_x1")]
    for batch, channels, si, so, mi, mo, in_place, kernel in rows:
        case = sam.Case(f"x/path/b{batch}_c{channels}_s{si}_{so}_m{mi}_{mo}_{in_place}", batch, channels, in_stride=si,
                        out_stride=so, misalign_in=mi, misalign_out=mo, in_place=in_place)
        assert sam.check(qnnp, reference, case, to_device, from_device) == kernel, case.name


# ---- API behaviour -------------------------------------------------------------------------------------------------
# (channels, input scale, output zero point, output scale): reference src/softargmax.c:36-70
CREATE = [(8, X, 0, S), (1, 1e-3, 0, S), (21841, 97.0, 0, S), (0, X, 0, S), (8, 0.0, 0, S), (8, -1.0, 0, S),
          (8, float("inf"), 0, S), (8, float("nan"), 0, S), (8, 1e-40, 0, S), (8, X, 0, 0.0), (8, X, 0, float("inf")),
          (8, X, 0, -S), (0, X, 7, 0.5), (8, 0.0, 7, 0.5), (8, X, 0, 0.5), (8, X, 0, S * 2), (8, X, 1, S), (8, X, 255, 0.5)]


def _create_statuses_match_the_reference(qnnp, reference):
    for args in CREATE:
        got = [lib.create_softargmax_nc_q8_status(*args) for lib in (qnnp, reference)]
        for lib, (st, op) in zip((qnnp, reference), got):
            if op:
                lib.delete_operator(op)
        assert got[0][0] == got[1][0], (args, got[0][0], got[1][0])
        assert bool(got[0][1]) == (got[0][0] == Status.success), args
    # the product's own limit: channels beyond the kernels' index range, after the reference's checks
    assert qnnp.create_softargmax_nc_q8_status(2 ** 31, X, 0, S)[0] == Status.unsupported_parameter
    assert qnnp.create_softargmax_nc_q8_status(2 ** 31, 0.0, 0, S)[0] == Status.invalid_parameter
    st, op = qnnp.create_softargmax_nc_q8_status(2 ** 31 - 1, X, 0, S)
    assert st == Status.success
    qnnp.delete_operator(op)


def _setup_statuses(qnnp, reference):
    case = sam.Case("x/setup", 3, 16)
    x = np.zeros(4096, np.uint8)
    y = np.zeros(4096, np.uint8)
    x[:48] = sam.input_tensor(case)
    for lib in (qnnp, reference):
        # reference softargmax.c:119-122: batch 0 succeeds and does nothing
        op = sam.create(lib, case)[1]
        assert lib.setup_softargmax_nc_q8_status(op, 0, None, 16, None, 16) == Status.success
        assert lib.run_operator_status(op) == Status.success
        assert lib.setup_softargmax_nc_q8_status(op, 3, x, 16, y, 16) == Status.success
        assert lib.run_operator_status(op) == Status.success
        lib.delete_operator(op)
    # where the reference checks nothing and would go out of range, the product refuses (include/qnnpack_gfx950.h)
    setup = qnnp.setup_softargmax_nc_q8_status
    op = sam.create(qnnp, case)[1]
    clamp = qnnp.create_clamp_nc_u8(16, 0, 255)
    d = to_device(x)
    try:
        assert qnnp.run_operator_status(op) == Status.invalid_parameter          # before any setup
        assert setup(op, 3, None, 16, y, 16) == Status.invalid_parameter
        assert setup(op, 3, x, 16, None, 16) == Status.invalid_parameter
        assert setup(op, 3, x, 15, y, 16) == Status.invalid_parameter
        assert setup(op, 3, x, 16, y, 15) == Status.invalid_parameter
        assert setup(op, 3, d, 16, d.data_ptr() + 1, 16) == Status.invalid_parameter     # partial overlap
        assert setup(op, 3, d, 16, d.data_ptr() + 47, 16) == Status.invalid_parameter    # one shared byte
        assert setup(op, 3, d, 16, d, 17) == Status.invalid_parameter                    # same base, other stride
        assert setup(op, 3, d, 16, d, 16) == Status.success                              # in place
        xi = x.copy()
        assert setup(op, 3, xi, 16, xi, 16) == Status.success                            # in place, host memory
        assert qnnp.run_operator_status(op) == Status.success
        assert np.array_equal(xi[:48], sam.model(case, x[:48])[0]) and np.array_equal(xi[48:], x[48:])
        assert setup(op, 3, d, 16, d.data_ptr() + 48, 16) == Status.success
        assert setup(op, 2 ** 31, d, 16, d, 16) == Status.unsupported_parameter
        # a tensor on the host for one end and on the device for the other
        assert setup(op, 3, x, 16, d.data_ptr() + 1024, 16) == Status.success
        assert qnnp.run_operator_status(op) == Status.success
        want = sam.model(case, x[:48])[0]
        assert np.array_equal(from_device(d)[1024:1024 + 48], want)
        assert setup(op, 3, d, 16, y, 16) == Status.success
        assert qnnp.run_operator_status(op) == Status.success
        assert np.array_equal(y[:48], want) and np.all(y[48:] == 0)
        # a setup refused by its checks leaves the previous one runnable
        assert setup(op, 3, d, 15, d, 16) == Status.invalid_parameter
        assert qnnp.run_operator_status(op) == Status.success
        # another operator type's handle
        assert setup(clamp, 3, d, 16, d.data_ptr() + 48, 16) == Status.invalid_parameter
        assert qnnp.setup_clamp_nc_u8_status(op, 3, d, 16, d.data_ptr() + 48, 16) == Status.invalid_parameter
    finally:
        qnnp.delete_operator(op)
        qnnp.delete_operator(clamp)


def _graph_replayed_twice_with_the_input_changed(qnnp, reference):
    import torch
    cases = [sam.Case("x/graph/group", 4 * 33 * 33, 21), sam.Case("x/graph/lds", 64, 1500, in_stride=1504, out_stride=1520)]
    ops, bufs = [], []
    try:
        for case in cases:
            op = sam.create(qnnp, case)[1]
            ops.append(op)
            d_x, d_y = to_device(sam.input_tensor(case)), to_device(sam.output_tensor(case))
            bufs.append((d_x, d_y))
            si, so = case.strides_at(0)
            assert qnnp.setup_softargmax_nc_q8_status(op, case.batch, d_x, si, d_y, so) == Status.success
        qnnp.graph_begin()
        try:
            for op in ops:
                qnnp.run_operator(op)
            # neither create nor setup can be recorded: both refuse and leave the operator as it was
            assert sam.create(qnnp, cases[0])[0] == Status.invalid_parameter
            assert qnnp.setup_softargmax_nc_q8_status(ops[0], 1, bufs[0][0], 21, bufs[0][1], 21) == Status.invalid_parameter
        finally:
            graph = qnnp.graph_end()
        assert all(np.all(from_device(d_y) == sam.FILL) for _, d_y in bufs), "nothing runs during the capture"
        try:
            for rep in range(2):
                inputs = []
                for k, (case, (d_x, d_y)) in enumerate(zip(cases, bufs)):
                    x = np.random.default_rng(sam._seed(f"{case.name}/replay{rep}")).integers(0, 256, size=d_x.numel(), dtype=np.uint8)
                    inputs.append(x)
                    d_x.copy_(torch.from_numpy(x))
                    d_y.fill_(sam.FILL)
                torch.cuda.synchronize()
                qnnp.graph_launch(graph)
                qnnp.graph_synchronize(graph)
                for case, x, (_, d_y) in zip(cases, inputs, bufs):
                    want = sam.run_reference(reference, case, inputs=[x])[0][sam.PAD:-sam.PAD]
                    assert np.array_equal(from_device(d_y), want), f"replay {rep}: {case.name}"
        finally:
            qnnp.graph_destroy(graph)
    finally:
        for op in ops:
            qnnp.delete_operator(op)


# ---- row offsets past 2^32 -------------------------------------------------------------------------------------------
def _row_strides_past_2g(qnnp, reference):
    """3 rows of 1000 channels, input stride 2^31 + 13 and output stride 2^31 + 5: the last row starts past 2^32 bytes in
    both tensors. Only the rows and 64 bytes on either side of each are written before the run and read back after."""
    rows, channels, si, so, edge = 3, 1000, (1 << 31) + 13, (1 << 31) + 5, 64
    ispan, ospan = (rows - 1) * si + channels, (rows - 1) * so + channels
    assert (rows - 1) * si > 1 << 32 and (rows - 1) * so > 1 << 32
    lg.free_memory()
    lg.require_memory(ispan + ospan + 4 * edge, "softargmax_strides_past_2g")
    case = sam.Case("x/strides_past_2g", rows, channels)
    x = sam.input_tensor(case).reshape(rows, channels)
    want = sam.run_reference(reference, case, inputs=[x.reshape(-1)])[0][sam.PAD:-sam.PAD].reshape(rows, channels)
    margin = np.full(edge, sam.FILL, np.uint8)
    d_in, d_out = qnnp.malloc(ispan + 2 * edge), qnnp.malloc(ospan + 2 * edge)
    op = sam.create(qnnp, case)[1]
    try:
        for r in range(rows):
            qnnp.memcpy_h2d(d_in + r * si, np.concatenate([margin, x[r], margin]))
            qnnp.memcpy_h2d(d_out + r * so, np.full(channels + 2 * edge, sam.FILL, np.uint8))
        assert qnnp.setup_softargmax_nc_q8_status(op, rows, d_in + edge, si, d_out + edge, so) == Status.success
        qnnp.run_operator(op)
        assert qnnp.operator_kernel(op) == sam.kernel_name(channels, 1)       # the strides differ by 8
        for r in range(rows):
            got = np.empty(channels + 2 * edge, np.uint8)
            qnnp.memcpy_d2h(got, d_out + r * so)
            assert np.array_equal(got[edge:-edge], want[r]), f"row {r}"
            assert np.all(got[:edge] == sam.FILL) and np.all(got[-edge:] == sam.FILL), f"row {r}: bytes beside the row were written"
            back = np.empty(channels + 2 * edge, np.uint8)
            qnnp.memcpy_d2h(back, d_in + r * si)
            assert np.array_equal(back, np.concatenate([margin, x[r], margin])), f"row {r}: the input was written"
    finally:
        qnnp.delete_operator(op)
        qnnp.free(d_in)
        qnnp.free(d_out)
        lg.free_memory()


# ---- the one test ------------------------------------------------------------------------------------------------------
# All of the above under ONE test id, as tests/test_gpu_lut.py groups its checks: the whole file runs in a few seconds, and
# the GPU tier's count of test ids stays what it was plus one. A failure names the part, and the part names the case, the
# setup and the kernel.
PARTS = [_reference_test_list, _selection_boundaries, _misaligned, _extra_cases, _zero_sum_rows_give_zeros_and_disturb_nothing,
         _more_than_one_pass_of_each_loop, _each_kernel_family_is_named_on_the_shape_meant_for_it,
         _create_statuses_match_the_reference, _setup_statuses, _graph_replayed_twice_with_the_input_changed,
         _row_strides_past_2g]


def test_softargmax(qnnp, reference):
    for part in PARTS:
        try:
            part(qnnp, reference)
        except AssertionError as e:
            raise AssertionError(f"{part.__name__.lstrip('_')}: {e}") from e
