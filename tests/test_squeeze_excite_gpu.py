"""GPU tier of the fused squeeze-and-excite operator (hip/q8segate.hip + hip/q8mul.hip behind squeeze-excite.c).

The bar is byte equality with the oracle's expectation of the block (tests/_squeeze_excite.py: pooling, two fully
connected layers, the table, the multiply, stage by stage on the CPU) -- nothing excluded, no tolerance, the bytes between
strided rows included -- and, in the same part, with the five stand-alone operators run on the GPU. Before anything runs,
the expectation is asserted not to be degenerate.

 1. every case in the three flavours ("se_kernel" 1: pooling inside the gate kernel, 2: a pooling launch in front, 0: auto),
    the kernel name asserted, next to the chain of stand-alone operators;
 2. layout: strides above C, base addresses off by 1, 2 and 3 bytes, in place and out of place, guards before, between
    the rows and after the output, the input unchanged;
 3. lifecycle: host pointers, async mode, re-setup with scratch growth, members on their own afterwards and deleted after
    the fused operator, one hipGraph replayed twice, create and setup inside a capture, the statuses in the header's order.
"""
import numpy as np
import pytest

import _multiply as mul
import _squeeze_excite as se
from _gpu import Guarded, from_device, to_device
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

FLAVOURS = (1, 2, 0)


def _setup_forced(qnnp, op, flavour, *args):
    """the flavour is read at setup; forcing is reset whatever happens"""
    qnnp.set_option("se_kernel", flavour)
    try:
        return qnnp.setup_squeeze_excite_status(op, *args)
    finally:
        qnnp.set_option("se_kernel", 0)


def _check_kernel(qnnp, op, case, flavour, what):
    kernel = qnnp.operator_kernel(op)
    assert kernel == (se.KERNELS[flavour] if flavour else se.auto_kernel(case)), (what, kernel)
    return kernel


def _run_chain(qnnp, b, ops):
    """the five stand-alone operators on dense device buffers; the stages as they come back"""
    case = b.case
    batch, pixels, c, s = case.batch, case.pixels, case.c, case.s
    gap, fc1, fc2, gate, multiply = ops
    d_x = to_device(b.x)
    d_p, d_h, d_e, d_s = (to_device(np.full(n, se.FILL, np.uint8)) for n in (batch * c, batch * s, batch * c, batch * c))
    d_y = to_device(np.full(b.want.size, se.FILL, np.uint8))
    qnnp.setup_global_average_pooling_nwc_q8(gap, batch, pixels, d_x, c, d_p, c)
    qnnp.setup_fully_connected_nc_q8(fc1, batch, d_p, c, d_h, s)
    qnnp.setup_fully_connected_nc_q8(fc2, batch, d_h, s, d_e, c)
    qnnp.setup_lut_nc_x8(gate, batch, d_e, c, d_s, c)
    qnnp.setup_multiply_nc_q8(multiply, batch, pixels, d_x, c, d_s, c, d_y, c)
    for op in ops:
        qnnp.run_operator(op)
    return [from_device(t) for t in (d_p, d_h, d_e, d_s, d_y)]


def _chain_against_oracle(qnnp, b, ops):
    """None, or the first stage at which the stand-alone chain and the oracle differ"""
    for (name, want), got in zip(b.stages(), _run_chain(qnnp, b, ops)):
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            return f"{name}: {bad.size} bytes, first at {bad[:4]}: chain {got[bad[:4]]}, oracle {want[bad[:4]]}"
    return None


def _run_fused(qnnp, b, fused, flavour, x_stride=0, y_stride=0, x_offset=0, y_offset=0, in_place=False, what=""):
    """one guarded run of the fused operator; compares the output (gaps included), the guards and the input"""
    case = b.case
    c = case.c
    xs = x_stride or c
    ys = xs if in_place else (y_stride or c)
    x = b.strided(b.x, xs)
    want = b.strided(b.want, ys)                           # the gaps: FILL, in place the input's own gap bytes (FILL too)
    gx = Guarded(x, x_offset)
    gy = gx if in_place else Guarded(np.full(want.size, se.FILL, np.uint8), y_offset)
    what = f"{case.name} se_kernel {flavour} strides {xs}/{ys} offsets {x_offset}/{y_offset}{' in place' if in_place else ''} {what}"
    st = _setup_forced(qnnp, fused, flavour, case.batch, case.pixels, gx, xs, gy, ys)
    assert st == Status.success, (what, st)
    qnnp.run_operator(fused)
    kernel = _check_kernel(qnnp, fused, case, flavour, what)
    se.differences(gy.read(), want, f"{what} ({kernel})")
    gy.assert_intact(what)
    if not in_place:
        gx.assert_intact(what + " (input)")
        se.differences(gx.read(), x, f"{what}: the input changed")
    return kernel


# ---- 1. every case, every flavour, next to the chain ---------------------------------------------------------------
def _every_case_in_every_flavour_and_the_chain(qnnp):
    autos = {}
    for case in se.CASES:
        b = se.block(case)
        se.assert_not_degenerate(b)
        ops = b.create_members(qnnp)
        fused = None
        try:
            chain = _chain_against_oracle(qnnp, b, ops)
            fused = qnnp.create_squeeze_excite(*ops)
            assert qnnp.run_operator_status(fused) == Status.invalid_parameter        # before any setup
            try:
                for flavour in FLAVOURS:
                    autos[case.name] = _run_fused(qnnp, b, fused, flavour)
            except AssertionError as e:
                raise AssertionError(f"{e}; the stand-alone chain against the oracle: "
                                     f"{chain or 'equal at every stage'}") from e
            # equality with the five stand-alone operators, which is equality with the oracle unless they differ themselves
            assert chain is None, f"{case.name}: the stand-alone chain and the oracle differ at {chain}"
        finally:
            if fused:
                qnnp.delete_operator(fused)
            se.delete_all(qnnp, ops)
    # both sides of the automatic rule were taken
    assert set(autos.values()) == set(se.KERNELS.values()), autos


# ---- 2. layout -----------------------------------------------------------------------------------------------------
LAYOUT = [   # (case, x stride - C, y stride - C, x offset, y offset)
    ("mobilenet_se", 0, 0, 1, 2), ("mobilenet_se", 8, 16, 0, 0), ("mobilenet_se", 5, 3, 3, 1), ("mobilenet_se", 4, 4, 2, 2),
    ("nothing_aligned", 0, 0, 0, 0), ("nothing_aligned", 7, 2, 1, 3), ("nothing_aligned", 3, 3, 2, 0),
    ("b1_196", 24, 8, 0, 3), ("b1_196", 1, 0, 3, 0), ("wide", 12, 4, 1, 2), ("wide", 0, 0, 2, 0),
    ("pool_passes", 4, 0, 0, 1), ("pool_passes", 3, 5, 3, 3)]


def _strides_offsets_guards_in_place(qnnp):
    members = {}
    try:
        for name, ex, ey, ox, oy in LAYOUT:
            case = next(c for c in se.CASES if c.name == name)
            b = se.block(case)
            if name not in members:
                ops = b.create_members(qnnp)
                members[name] = (ops, qnnp.create_squeeze_excite(*ops))
            fused = members[name][1]
            for flavour in FLAVOURS:
                _run_fused(qnnp, b, fused, flavour, case.c + ex, case.c + ey, ox, oy)
                _run_fused(qnnp, b, fused, flavour, case.c + ex, 0, ox, 0, in_place=True)
    finally:
        for ops, fused in members.values():
            qnnp.delete_operator(fused)
            se.delete_all(qnnp, ops)


# ---- 3. lifecycle ----------------------------------------------------------------------------------------------------
def _host_pointers_async_resetup_members(qnnp):
    import torch
    small, large = se.block(se.CASES[0]), se.block(next(c for c in se.CASES if c.name == "k_blocks"))
    # host pointers, strided, out of place and in place, in every flavour
    ops = small.create_members(qnnp)
    fused = qnnp.create_squeeze_excite(*ops)
    try:
        case, c = small.case, small.case.c
        for flavour in FLAVOURS:
            xs, ys = c + 5, c + 3
            x, y = small.strided(small.x, xs), np.full(mul.span(small.rows, ys, c), se.FILL, np.uint8)
            x0 = x.copy()
            assert _setup_forced(qnnp, fused, flavour, case.batch, case.pixels, x, xs, y, ys) == Status.success
            qnnp.run_operator(fused)
            _check_kernel(qnnp, fused, case, flavour, "host pointers")
            se.differences(y, small.strided(small.want, ys), f"host pointers, se_kernel {flavour}")
            assert np.array_equal(x, x0)
            assert _setup_forced(qnnp, fused, flavour, case.batch, case.pixels, x, xs, x, xs) == Status.success
            qnnp.run_operator(fused)
            se.differences(x, small.strided(small.want, xs), f"host pointers in place, se_kernel {flavour}")
        # async mode, device pointers, the streaming hint handed to the multiply launch; then timing
        d_x, d_y = to_device(small.x), to_device(np.full(small.want.size, se.FILL, np.uint8))
        qnnp.set_async(True)
        try:
            assert qnnp.setup_squeeze_excite_status(fused, case.batch, case.pixels, d_x, c, d_y, c) == Status.success
            for streaming in (1, 0, -1):
                qnnp.operator_set_streaming_stores(fused, streaming)
                d_y.fill_(se.FILL)
                for _ in range(3):
                    qnnp.run_operator(fused)
                qnnp.synchronize()
                torch.cuda.synchronize()
                se.differences(from_device(d_y), small.want, f"async runs, streaming {streaming}")
        finally:
            qnnp.set_async(False)
        assert qnnp.time_operator(fused, 1, 3) > 0.0
        se.differences(from_device(d_y), small.want, "after timing")
        # batch 0: success, and run does nothing
        d_y.fill_(se.FILL)
        assert qnnp.setup_squeeze_excite_status(fused, 0, 0, None, 0, None, 0) == Status.success
        assert qnnp.run_operator_status(fused) == Status.success
        assert np.all(from_device(d_y) == se.FILL)
        # the members are untouched: the chain still equals the oracle, and the fused operator after it
        assert _chain_against_oracle(qnnp, small, ops) is None
        _run_fused(qnnp, small, fused, 0, what="after the members ran on their own")
    finally:
        # the members are deleted AFTER the fused operator
        qnnp.delete_operator(fused)
        se.delete_all(qnnp, ops)
    # re-setup with another batch and pixel count on the same operator: one image, the whole batch (the scratch grows, and
    # the three-launch flavour's second part moves), one image again; then the same bytes as 4 images of 25 pixels
    ops = large.create_members(qnnp)
    fused = qnnp.create_squeeze_excite(*ops)
    try:
        case, c = large.case, large.case.c
        for flavour in (2, 1):
            for batch, pixels in ((1, case.pixels), (case.batch, case.pixels), (1, case.pixels), (4, case.pixels // 2)):
                rows = batch * pixels
                want = large.expected_for(batch, pixels)
                assert batch * pixels <= large.rows and np.unique(want).size > 64
                gx = Guarded(large.x[:rows * c].copy(), 1)
                gy = Guarded(np.full(rows * c, se.FILL, np.uint8), 3)
                assert _setup_forced(qnnp, fused, flavour, batch, pixels, gx, c, gy, c) == Status.success
                qnnp.run_operator(fused)
                se.differences(gy.read(), want, f"re-setup to batch {batch} of {pixels} pixels, se_kernel {flavour}")
                gy.assert_intact(f"re-setup to batch {batch} of {pixels} pixels")
        assert np.array_equal(large.expected_for(case.batch, case.pixels), large.want)
    finally:
        qnnp.delete_operator(fused)
        se.delete_all(qnnp, ops)


def _one_graph_replayed_twice(qnnp):
    import torch
    for flavour in (1, 2):
        b = se.block(se.CASES[0])
        case, c = b.case, b.case.c
        ops = b.create_members(qnnp)
        fused = qnnp.create_squeeze_excite(*ops)
        graph = None
        try:
            d_x0, d_x = to_device(b.x), to_device(b.x)
            assert _setup_forced(qnnp, fused, flavour, case.batch, case.pixels, d_x, c, d_x, c) == Status.success   # in place, as a network
            qnnp.graph_begin()
            try:
                qnnp.run_operator(fused)
                # neither create nor setup can be recorded
                st, none = qnnp.create_squeeze_excite_status(*ops)
                assert st == Status.invalid_parameter and not none
                assert qnnp.setup_squeeze_excite_status(fused, case.batch, case.pixels, d_x, c, d_x, c) == Status.invalid_parameter
            finally:
                graph = qnnp.graph_end()
            assert np.array_equal(from_device(d_x), b.x), "nothing runs during the capture"
            for rep in range(2):
                d_x.copy_(d_x0)
                torch.cuda.synchronize()
                qnnp.graph_launch(graph)
                qnnp.graph_synchronize(graph)
                se.differences(from_device(d_x), b.want, f"replay {rep}, se_kernel {flavour} ({qnnp.operator_kernel(fused)})")
            # a host-pointer setup cannot be recorded
            x = b.x.copy()
            assert qnnp.setup_squeeze_excite_status(fused, case.batch, case.pixels, x, c, x, c) == Status.success
            qnnp.graph_begin()
            try:
                assert qnnp.run_operator_status(fused) == Status.invalid_parameter
            finally:
                qnnp.graph_destroy(qnnp.graph_end())
        finally:
            if graph:
                qnnp.graph_destroy(graph)
            qnnp.delete_operator(fused)
            se.delete_all(qnnp, ops)


def _statuses_in_the_headers_order(qnnp):
    b = se.block(se.CASES[0])                              # 24 channels squeezed to 8
    other = se.block(next(c for c in se.CASES if c.name == "nothing_aligned"))   # 33 to 9
    ops, others = b.create_members(qnnp), other.create_members(qnnp)
    gap, fc1, fc2, gate, multiply = ops
    extra = []
    create = qnnp.create_squeeze_excite_status
    try:
        # ---- create: invalid_parameter ----
        for i in range(5):                                  # a NULL member
            members = list(ops)
            members[i] = None
            assert create(*members) == (Status.invalid_parameter, None), i
        add = qnnp.create_add_nc_q8(24, 0, 1.0, 0, 1.0, 0, 1.0, 0, 255)
        extra.append(add)
        for members in ((add, fc1, fc2, gate, multiply), (gap, gate, fc2, gate, multiply), (gap, fc1, add, gate, multiply),
                        (gap, fc1, fc2, multiply, multiply), (gap, fc1, fc2, gate, gate), (fc1, gap, fc2, gate, multiply)):
            assert create(*members) == (Status.invalid_parameter, None)            # a member of the wrong kind
        for i in range(5):                                  # a chain that does not close: each member from the other block
            members = list(ops)
            members[i] = others[i]
            assert create(*members) == (Status.invalid_parameter, None), i
        assert create(gap, fc2, fc1, gate, multiply) == (Status.invalid_parameter, None)   # 24 -> 8 -> 24 swapped
        # ---- create: unsupported_parameter, after every invalid_parameter ----
        scales = (np.float32(1.0) / b.scale1) * np.linspace(1.0, 0.9, 8, dtype=np.float32)       # one weight scale per output channel
        pc = qnnp.create_fully_connected_nc_q8_per_channel(24, 8, b.fc1.izp, 1.0, b.fc1.kzp, scales, b.k1, b.b1, b.zp1, 1.0,
                                                           b.fc1.qmin, 255, 0)
        extra.append(pc)
        assert create(gap, pc, fc2, gate, multiply) == (Status.unsupported_parameter, None)
        assert create(gap, pc, fc2, gate, None) == (Status.invalid_parameter, None)
        assert create(gap, pc, fc2, others[3], multiply) == (Status.invalid_parameter, None)
        limit = 4096                                        # QNNP_GFX950_SQUEEZE_EXCITE_MAX_CHANNELS
        for c, s in ((limit + 1, 1), (1, limit + 1)):
            big = [qnnp.create_global_average_pooling_nwc_q8(c, 0, 1.0, 0, 1.0, 0, 255, 0),
                   qnnp.create_fully_connected_nc_q8(c, s, 0, 1.0, 128, 0.001, np.full((s, c), 130, np.uint8), np.zeros(s, np.int32), 0, 1.0, 0, 255, 0),
                   qnnp.create_fully_connected_nc_q8(s, c, 0, 1.0, 128, 0.001, np.full((c, s), 130, np.uint8), np.zeros(c, np.int32), 0, 1.0, 0, 255, 0),
                   qnnp.create_lut_nc_x8(c, np.arange(256, dtype=np.uint8)),
                   qnnp.create_multiply_nc_q8(c, *mul.MID.args())]
            try:
                assert create(*big) == (Status.unsupported_parameter, None), (c, s)
            finally:
                se.delete_all(qnnp, big)
        # ---- setup ----
        fused = qnnp.create_squeeze_excite(*ops)
        extra.append(fused)
        setup = qnnp.setup_squeeze_excite_status
        case, c = b.case, 24
        batch, pixels = case.batch, case.pixels
        d_x = to_device(b.x)
        d_y = to_device(np.full(b.want.size, se.FILL, np.uint8))
        base = d_x.data_ptr()
        assert setup(None, batch, pixels, d_x, c, d_y, c) == Status.invalid_parameter
        assert setup(multiply, batch, pixels, d_x, c, d_y, c) == Status.invalid_parameter
        assert qnnp.setup_multiply_nc_q8_status(fused, batch, pixels, d_x, c, d_x, c, d_y, c) == Status.invalid_parameter
        assert qnnp.setup_global_average_pooling_nwc_q8_status(fused, batch, pixels, d_x, c, d_y, c) == Status.invalid_parameter
        assert setup(fused, 0, 0, None, 0, None, 0) == Status.success              # batch 0 first
        assert setup(fused, batch, pixels, d_x, c, d_y, c) == Status.success
        qnnp.run_operator(fused)
        se.differences(from_device(d_y), b.want, "before the refused setups")
        too_wide = (2 ** 31 - 1) // 255 + 1
        refused = [
            ((batch, 0, d_x, c, d_y, c), Status.invalid_parameter),
            ((batch, pixels, None, c, d_y, c), Status.invalid_parameter),
            ((batch, pixels, d_x, c, None, c), Status.invalid_parameter),
            ((batch, pixels, d_x, c - 1, d_y, c), Status.invalid_parameter),
            ((batch, pixels, d_x, c, d_y, c - 1), Status.invalid_parameter),
            ((batch, too_wide, d_x, c - 1, d_y, c), Status.invalid_parameter),      # invalid before unsupported
            ((batch, too_wide, d_x, c, d_y, c), Status.unsupported_parameter),      # the pooling's width bound
            ((1, too_wide, d_x, c, base + 1, c), Status.unsupported_parameter),     # unsupported before the overlap
            ((2 ** 31, 1, d_x, c, d_y, c), Status.unsupported_parameter),
            ((65536, 32768, d_x, c, d_y, c), Status.unsupported_parameter),         # batch * pixels == 2^31
            ((2 ** 64 - 1, pixels, d_x, c, d_y, c), Status.unsupported_parameter),
            ((batch, pixels, d_x, c, base + 1, c), Status.invalid_parameter),       # shifted
            ((batch, pixels - 1, d_x, c + 1, d_x, c), Status.invalid_parameter),    # the same base, another stride
            ((batch - 1, pixels, base + pixels * c, c, d_x, c), Status.invalid_parameter)]
        for args, want in refused:
            assert setup(fused, *args) == want, args
            d_y.fill_(se.FILL)                              # a refused setup leaves the previous one runnable
            assert qnnp.run_operator_status(fused) == Status.success
            se.differences(from_device(d_y), b.want, f"after the refused setup {args[:2]}")
        # the pooling setup draws the same line
        assert qnnp.setup_global_average_pooling_nwc_q8_status(gap, batch, too_wide, d_x, c, d_y, c) == Status.unsupported_parameter
    finally:
        se.delete_all(qnnp, extra)
        se.delete_all(qnnp, ops)
        se.delete_all(qnnp, others)


# ---- the one test ------------------------------------------------------------------------------------------------
# All of the above under ONE test id, as tests/test_multiply_gpu.py groups its checks: the whole file runs in a few seconds
# and the GPU tier's count of test ids grows by one. A failure names the part, and the part names the case, the flavour,
# the layout and the kernel.
PARTS = [_every_case_in_every_flavour_and_the_chain,                                              # 1
         _strides_offsets_guards_in_place,                                                        # 2
         _host_pointers_async_resetup_members, _one_graph_replayed_twice, _statuses_in_the_headers_order]   # 3


def test_squeeze_excite(qnnp):
    for part in PARTS:
        try:
            part(qnnp)
        except AssertionError as e:
            raise AssertionError(f"{part.__name__.lstrip('_')}: {e}") from e
