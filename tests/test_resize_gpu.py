"""GPU tier of the bilinear resize operator (hip/u8resize.hip behind resize-bilinear.c).

No reference operator exists; the definition in include/qnnpack_gfx950.h is integers only, and tests/_resize.py restates
it in numpy. All comparisons are byte-exact and include the FILL bytes between strided pixels.

 1. geometry: every (n_in, n_out) of two small size lists on either axis, both modes, batch 1 and 3, 16 and 5 channels;
 2. channel counts around the piece widths, dense and with padded pixel strides, the kernel of each class;
 3. 1 .. 20 channels with both base addresses misaligned by 0 .. 15 bytes;
 4. guarded tensors at odd offsets, the x4 kernel's tail and the tensor's last pixel at the guard;
 5. more than one pass of each grid-stride loop of each kernel, pixels longer than a workgroup's pieces;
 6. create and setup statuses, overlaps, operator kinds, host pointers, async mode, timing, re-setup;
 7. average pooling -> resize back -> add with the original (the shape of an LR-ASPP merge) as one hipGraph.
"""
import numpy as np
import pytest

import _pointwise as pw
import _pooling as pool
import _resize as rs
from _gpu import Guarded, from_device, to_device
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu


def _differences(got, want, what):
    if not np.array_equal(got, want):
        assert got.size == want.size, (what, got.size, want.size)
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[:4]}: got {got[bad[:4]]}, want {want[bad[:4]]}")


def _run(qnnp, c, name, misalign=(0, 0), op=None):
    """one case on fresh device buffers at the given base misalignments; returns the kernel name"""
    x, y = rs.tensors(name, c)
    want = rs.expected(c, x, y)
    if rs.has_extremes(c):
        # the bottom and the 255 * 2^22 top of the accumulator
        pixels = rs.pixels_view(want, c.batch, c.out_h, c.out_w, c.out_stride, c.channels)
        assert pixels.min() == 0 and pixels.max() == 255, (name, c)
    own = op is None
    if own:
        op = qnnp.create_resize_bilinear2d_nhwc_u8(c.channels, c.flags)
    try:
        d_x, d_y = to_device(x, misalign[0]), to_device(y, misalign[1])
        assert qnnp.setup_resize_bilinear2d_nhwc_u8_status(op, *c.setup_args(d_x, d_y)) == Status.success, (name, c)
        qnnp.run_operator(op)
        kernel = qnnp.operator_kernel(op)
        _differences(from_device(d_y), want, f"{name} {c} ({kernel})")
        _differences(from_device(d_x), x, f"{name} {c} ({kernel}): the input changed")
        assert kernel == rs.kernel_for(c.channels, (d_x.data_ptr(), d_y.data_ptr()), (c.in_stride, c.out_stride)), (name, c, kernel)
        return kernel
    finally:
        if own:
            qnnp.delete_operator(op)


# ---- 1. geometry -----------------------------------------------------------------------------------------------------
def _geometry_in_both_modes(qnnp):
    for align in (False, True):
        for channels in (16, 5):
            op = qnnp.create_resize_bilinear2d_nhwc_u8(channels, rs.ALIGN_CORNERS if align else 0)
            try:
                for n_in in rs.GEOMETRY_IN:
                    for n_out in rs.GEOMETRY_OUT:
                        for batch in (1, 3):
                            for in_h, in_w, out_h, out_w in ((n_in, 3, n_out, 4), (3, n_in, 4, n_out)):
                                c = rs.Case(batch, in_h, in_w, out_h, out_w, channels, align=align)
                                _run(qnnp, c, f"geometry/{c}", op=op)
            finally:
                qnnp.delete_operator(op)


# ---- 2. channels and strides -----------------------------------------------------------------------------------------
def _channels_dense_and_strided(qnnp):
    seen = set()
    for channels in rs.CHANNELS:
        strides = [(0, 0), (channels + 3, channels + 7)]
        if channels in (16, 32, 64):
            strides.append((channels + 16, channels + 16))
        for align in (False, True):
            op = qnnp.create_resize_bilinear2d_nhwc_u8(channels, rs.ALIGN_CORNERS if align else 0)
            try:
                for si, so in strides:
                    c = rs.Case(2, 3, 5, 7, 4, channels, si, so, align)
                    seen.add(_run(qnnp, c, f"channels/{c}", op=op))
            finally:
                qnnp.delete_operator(op)
    assert seen == {"u8_resize_x16", "u8_resize_x4", "u8_resize_x1"}


# ---- 3. misalignment -------------------------------------------------------------------------------------------------
def _base_misalignments(qnnp):
    seen = set()
    for channels in range(1, 21):
        op = qnnp.create_resize_bilinear2d_nhwc_u8(channels, 0)
        try:
            for m in range(16):
                c = rs.Case(2, 2, 3, 3, 5, channels)
                seen.add(_run(qnnp, c, f"misalign/c{channels}_m{m}", (m, m), op=op))
                if channels == 16 and m % 5 == 1:
                    seen.add(_run(qnnp, c, f"misalign/c{channels}_in{m}", (m, 0), op=op))
                    seen.add(_run(qnnp, c, f"misalign/c{channels}_out{m}", (0, m), op=op))
        finally:
            qnnp.delete_operator(op)
    assert seen == {"u8_resize_x16", "u8_resize_x4", "u8_resize_x1"}


# ---- 4. guards -------------------------------------------------------------------------------------------------------
GUARDED = [   # (channels, input stride, output stride, input offset, output offset, align corners)
    (64, 0, 0, 0, 0, False), (64, 80, 96, 16, 48, True), (16, 0, 0, 0, 0, False), (16, 0, 0, 3, 16, False),
    (5, 0, 0, 1, 3, False), (5, 9, 6, 7, 5, True), (7, 0, 0, 3, 1, False), (7, 7, 10, 0, 13, True),
    (21, 0, 0, 1, 1, False), (21, 0, 0, 15, 2, True), (21, 24, 29, 5, 7, False), (4, 0, 0, 1, 2, False),
    (3, 0, 0, 1, 1, False), (1, 0, 0, 15, 13, True), (2, 5, 3, 3, 9, False), (33, 0, 0, 7, 3, False)]


def _nothing_is_written_outside_the_output(qnnp):
    for channels, si, so, oi, oo, align in GUARDED:
        c = rs.Case(2, 3, 4, 5, 7, channels, si, so, align)
        name = f"guarded/{c}_{oi}_{oo}"
        x, y = rs.tensors(name, c)
        # exact spans: the last pixel of either tensor ends where the guard begins
        assert x.size == c.in_span and y.size == c.out_span
        gx, gy = Guarded(x, oi), Guarded(y, oo)
        op = qnnp.create_resize_bilinear2d_nhwc_u8(channels, c.flags)
        try:
            assert qnnp.setup_resize_bilinear2d_nhwc_u8_status(op, *c.setup_args(gx, gy)) == Status.success, name
            qnnp.run_operator(op)
            kernel = qnnp.operator_kernel(op)
            assert kernel == rs.kernel_for(channels, (gx.data_ptr(), gy.data_ptr()), (c.in_stride, c.out_stride)), (name, kernel)
            _differences(gy.read(), rs.expected(c, x, y), f"{name} ({kernel})")
            gy.assert_intact(f"{name} ({kernel}, output)")
            gx.assert_intact(f"{name} ({kernel}, input)")
            _differences(gx.read(), x, f"{name} ({kernel}): the input changed")
        finally:
            qnnp.delete_operator(op)


# ---- 5. more than one pass -------------------------------------------------------------------------------------------
def _more_than_one_pass_of_each_loop(qnnp):
    """hip/u8resize.hip launches at most compute units x 16 workgroups; beyond that its grid-stride loops take further
    passes. Per kernel the smallest tensors whose pixel groups exceed one pass of grid x (pixels of 129 or 130 pieces, the
    fewest that fill a workgroup alone; for the byte kernel 85 pixels of 3 pieces a workgroup), pixels longer than a
    workgroup's pieces, and -- where the kernel can have them -- one pixel with more 256-piece chunks than one pass of
    grid y."""
    cap = qnnp.device_info()["compute_units"] * 16
    rows = cap // 64 + 1
    for c, kernel, pieces in ((rs.Case(1, 3, 5, rows, 64, 16 * 129), "u8_resize_x16", 129),
                              (rs.Case(1, 3, 5, rows, 64, 4 * 129 + 1, align=True), "u8_resize_x4", 130)):
        assert 128 < pieces <= 256 and c.out_pixels > cap, (c, cap)      # one pixel a workgroup, more workgroups than the cap
        assert _run(qnnp, c, f"sweep/{kernel}") == kernel
    c = rs.Case(2, 5, 3, (cap * 85) // 1024 + 2, 512, 3)
    assert c.out_pixels > cap * 85                                       # 256 // 3 = 85 pixels a workgroup
    assert _run(qnnp, c, "sweep/u8_resize_x1") == "u8_resize_x1"
    # pixels longer than a workgroup's pieces: 300 and 301 pieces, two chunks
    for c, kernel in ((rs.Case(2, 2, 3, 3, 5, 16 * 300), "u8_resize_x16"),
                      (rs.Case(2, 2, 3, 3, 5, 4 * 300 + 1, 1208, 1203, True), "u8_resize_x4")):
        assert _run(qnnp, c, f"sweep_long/{kernel}") == kernel
    # more chunks than the launch cap: the chunk loop takes a second pass (the byte kernel has at most 3 pieces a pixel)
    long_pixel = cap * 256 + 300
    for c, kernel in ((rs.Case(1, 1, 2, 1, 3, 16 * long_pixel), "u8_resize_x16"),
                      (rs.Case(1, 2, 1, 3, 1, 4 * long_pixel + 3), "u8_resize_x4")):
        assert -(-long_pixel // 256) > cap
        assert _run(qnnp, c, f"sweep_chunks/{kernel}") == kernel


# ---- 6. API ----------------------------------------------------------------------------------------------------------
RESIZE_CREATE = [   # (channels, flags) -> status, in the documented order
    ((8, 0), Status.success), ((8, rs.ALIGN_CORNERS), Status.success), ((1, 0), Status.success),
    ((2 ** 31 - 1, rs.ALIGN_CORNERS), Status.success),
    ((0, 0), Status.invalid_parameter), ((0, 2), Status.invalid_parameter), ((8, 2), Status.invalid_parameter),
    ((8, 3), Status.invalid_parameter), ((8, 0x80000000), Status.invalid_parameter), ((8, 0xFFFFFFFF), Status.invalid_parameter),
    ((2 ** 31, 2), Status.invalid_parameter),                      # invalid before unsupported
    ((2 ** 31, 0), Status.unsupported_parameter), ((2 ** 40, rs.ALIGN_CORNERS), Status.unsupported_parameter)]


def _create_statuses(qnnp):
    for args, want in RESIZE_CREATE:
        st, op = qnnp.create_resize_bilinear2d_nhwc_u8_status(*args)
        if op:
            qnnp.delete_operator(op)
        assert st == want and bool(op) == (want == Status.success), (args, st)
    op = qnnp.create_resize_bilinear2d_nhwc_u8(8)
    assert qnnp.run_operator_status(op) == Status.invalid_parameter     # before any setup
    qnnp.operator_set_streaming_stores(op, 1)
    qnnp.operator_set_streaming_stores(op, 0)
    qnnp.operator_set_streaming_stores(op, -1)
    qnnp.delete_operator(op)


def _setup_statuses_and_overlaps(qnnp):
    ch = 16
    op = qnnp.create_resize_bilinear2d_nhwc_u8(ch)
    d = to_device(np.arange(16384, dtype=np.uint32).astype(np.uint8))
    e = to_device(np.zeros(16384, np.uint8))
    base = d.data_ptr()
    setup = qnnp.setup_resize_bilinear2d_nhwc_u8_status
    big = rs.SIZE_LIMIT
    in_span = 2 * 3 * 4 * ch          # 384 bytes
    try:
        # no images: success, and run does nothing, whatever the rest
        assert setup(op, 0, 0, 0, 0, 0, None, 0, None, 0) == Status.success
        assert qnnp.run_operator_status(op) == Status.success
        assert np.all(from_device(e) == 0)
        # the reference point of "a refused setup leaves the last one runnable"
        d[8192:].zero_()
        assert setup(op, 2, 3, 4, 5, 6, d, ch, base + 8192, ch) == Status.success
        qnnp.run_operator(op)
        want = from_device(d)
        assert want[8192:8192 + 2 * 5 * 6 * ch].any()
        refused = [   # in the documented order
            ((2, 0, 4, 5, 6, d, ch, e, ch), Status.invalid_parameter), ((2, 3, 0, 5, 6, d, ch, e, ch), Status.invalid_parameter),
            ((2, 3, 4, 0, 6, d, ch, e, ch), Status.invalid_parameter), ((2, 3, 4, 5, 0, d, ch, e, ch), Status.invalid_parameter),
            ((2, 0, big, 5, 6, d, ch, e, ch), Status.invalid_parameter),                     # invalid before unsupported
            ((2, 3, 4, 5, 6, None, ch, e, ch), Status.invalid_parameter), ((2, 3, 4, 5, 6, d, ch, None, ch), Status.invalid_parameter),
            ((2, big, 4, 5, 6, None, ch, e, ch), Status.invalid_parameter),
            ((2, 3, 4, 5, 6, d, ch - 1, e, ch), Status.invalid_parameter), ((2, 3, 4, 5, 6, d, ch, e, ch - 1), Status.invalid_parameter),
            ((2, 3, 4, 5, 6, d, 0, e, ch), Status.invalid_parameter),
            ((2, big, 4, 5, 6, d, ch, e, ch), Status.unsupported_parameter), ((2, 3, big, 5, 6, d, ch, e, ch), Status.unsupported_parameter),
            ((2, 3, 4, big, 6, d, ch, e, ch), Status.unsupported_parameter), ((2, 3, 4, 5, big, d, ch, e, ch), Status.unsupported_parameter),
            ((2, 3, 4, 2 ** 64 - 1, 2 ** 64 - 1, d, ch, e, ch), Status.unsupported_parameter),
            ((2 ** 31, 1, 1, 1, 1, d, ch, e, ch), Status.unsupported_parameter),
            ((2 ** 64 - 1, big - 1, big - 1, 1, 1, d, ch, e, ch), Status.unsupported_parameter),
            ((129, 1, 1, big - 1, 1, d, ch, e, ch), Status.unsupported_parameter),
            ((1, 1, 1, 32768, 65536, d, ch, e, ch), Status.unsupported_parameter),          # 2^31 output pixels
            ((1, 65536, 32768, 1, 1, d, ch, e, ch), Status.unsupported_parameter),          # 2^31 input pixels
            ((2, 32768, 32768, 1, 1, d, ch, e, ch), Status.unsupported_parameter),
            # overlaps: the same base, the output inside the input, the input inside the output, one shared byte either way
            ((2, 3, 4, 5, 6, d, ch, d, ch), Status.invalid_parameter),
            ((2, 3, 4, 1, 1, d, ch, base + 48, ch), Status.invalid_parameter),
            ((1, 1, 1, 5, 6, base + 48, ch, d, ch), Status.invalid_parameter),
            ((2, 3, 4, 5, 6, d, ch, base + in_span - 1, ch), Status.invalid_parameter),
            ((2, 3, 4, 5, 6, base + 2 * 5 * 6 * ch - 1, ch, d, ch), Status.invalid_parameter)]
        for args, status in refused:
            assert setup(op, *args) == status, args
            d[8192:].zero_()
            assert qnnp.run_operator_status(op) == Status.success
            assert np.array_equal(from_device(d), want), args
        # the output directly behind the input, and directly in front of it, is accepted
        assert setup(op, 2, 3, 4, 5, 6, d, ch, base + in_span, ch) == Status.success
        assert setup(op, 2, 3, 4, 5, 6, base + 2 * 5 * 6 * ch, ch, d, ch) == Status.success
        # the setups of other operator kinds refuse a resize operator, and the resize setup refuses theirs
        add = qnnp.create_add_nc_q8(ch, 0, 1.0, 0, 1.0, 0, 1.0, 0, 255)
        clamp = qnnp.create_clamp_nc_u8(ch, 0, 255)
        mul = qnnp.create_multiply_nc_q8(ch, 121, 0.05, 0, 1 / 256, 133, 0.04, 0, 255)
        maxpool = qnnp.create_max_pooling2d_nhwc_u8(0, 0, 0, 0, 2, 2, 2, 2, 1, 1, ch, 0, 255)
        try:
            for other in (add, clamp, mul, maxpool):
                assert setup(other, 2, 3, 4, 5, 6, d, ch, e, ch) == Status.invalid_parameter
            assert setup(None, 2, 3, 4, 5, 6, d, ch, e, ch) == Status.invalid_parameter
            assert qnnp.setup_add_nc_q8_status(op, 15, d, ch, e, ch, base + 8192, ch) == Status.invalid_parameter
            assert qnnp.setup_clamp_nc_u8_status(op, 15, d, ch, e, ch) == Status.invalid_parameter
            assert qnnp.setup_lut_nc_x8_status(op, 15, d, ch, e, ch) == Status.invalid_parameter
            assert qnnp.setup_multiply_nc_q8_status(op, 15, 1, d, ch, d, ch, e, ch) == Status.invalid_parameter
            assert qnnp.setup_max_pooling2d_nhwc_u8_status(op, 2, 4, 4, d, ch, e, ch) == Status.invalid_parameter
        finally:
            for other in (add, clamp, mul, maxpool):
                qnnp.delete_operator(other)
    finally:
        qnnp.delete_operator(op)


def _host_pointers_async_mode_and_resetup(qnnp):
    import torch
    # host pointers for both tensors and mixed, dense and strided
    for si, so, align in ((0, 0, False), (27, 23, True)):
        c = rs.Case(2, 3, 5, 7, 4, 21, si, so, align)
        x, y = rs.tensors(f"host/{c}", c)
        want = rs.expected(c, x, y)
        x0 = x.copy()
        op = qnnp.create_resize_bilinear2d_nhwc_u8(c.channels, c.flags)
        try:
            assert qnnp.setup_resize_bilinear2d_nhwc_u8_status(op, *c.setup_args(x, y)) == Status.success
            qnnp.run_operator(op)
            _differences(y, want, f"host pointers {c}")
            assert np.array_equal(x, x0)
            d_x = to_device(x)
            y[...] = rs.FILL
            assert qnnp.setup_resize_bilinear2d_nhwc_u8_status(op, *c.setup_args(d_x, y)) == Status.success
            qnnp.run_operator(op)
            _differences(y, want, f"device input, host output {c}")
            d_y = to_device(np.full(c.out_span, rs.FILL, np.uint8))
            assert qnnp.setup_resize_bilinear2d_nhwc_u8_status(op, *c.setup_args(x, d_y)) == Status.success
            qnnp.run_operator(op)
            _differences(from_device(d_y), want, f"host input, device output {c}")
        finally:
            qnnp.delete_operator(op)
    # async mode with three runs under each streaming setting, timing, re-setup to a larger and a smaller geometry
    c = rs.Case(4, 14, 14, 28, 28, 96)
    x, y = rs.tensors("async", c)
    want = rs.expected(c, x, y)
    large = rs.Case(4, 14, 14, 56, 40, 96, align=False)
    small = rs.Case(2, 14, 14, 5, 9, 96)
    op = qnnp.create_resize_bilinear2d_nhwc_u8(c.channels)
    d_x = to_device(x)
    d_y = to_device(np.full(large.out_span, rs.FILL, np.uint8))
    try:
        qnnp.set_async(True)
        assert qnnp.setup_resize_bilinear2d_nhwc_u8_status(op, *c.setup_args(d_x, d_y)) == Status.success
        for streaming in (1, 0, -1):
            qnnp.operator_set_streaming_stores(op, streaming)
            d_y.fill_(rs.FILL)
            for _ in range(3):
                qnnp.run_operator(op)
            qnnp.synchronize()
            torch.cuda.synchronize()
            assert qnnp.operator_kernel(op) == "u8_resize_x16"
            got = from_device(d_y)
            _differences(got[:c.out_span], want, f"async runs, streaming {streaming}")
            assert np.all(got[c.out_span:] == rs.FILL)
        qnnp.set_async(False)
        assert qnnp.time_operator(op, 1, 3) > 0.0
        _differences(from_device(d_y)[:c.out_span], want, "after timing")
        for nxt, what in ((large, "larger"), (small, "smaller")):
            d_y.fill_(rs.FILL)
            assert qnnp.setup_resize_bilinear2d_nhwc_u8_status(op, *nxt.setup_args(d_x, d_y)) == Status.success
            qnnp.run_operator(op)
            got = from_device(d_y)
            _differences(got[:nxt.out_span], rs.expected(nxt, x[:nxt.in_span], np.full(nxt.out_span, rs.FILL, np.uint8)),
                         f"re-setup to a {what} geometry")
            assert np.all(got[nxt.out_span:] == rs.FILL), what
    finally:
        qnnp.set_async(False)
        qnnp.delete_operator(op)


# ---- 7. an LR-ASPP merge as one hipGraph -----------------------------------------------------------------------------
def _pool_resize_add_as_one_graph(qnnp):
    """x [3][6][8][24] -> average pooling 2x2 stride 2 -> bilinear resize x2 back -> add with x, chained on device buffers,
    captured once, replayed twice; every intermediate tensor is checked"""
    import torch
    batch, h, w, ch = 3, 6, 8, 24
    pc = pool.PoolCase("avg", "resize_graph_pool", batch, h, w, ch, 2, 2, stride_height=2, stride_width=2, in_zp=121, out_zp=121)
    x = pool.input_tensor(pc)
    pooled = pool.expected(pc, x)[-1]
    rc = rs.Case(batch, h // 2, w // 2, h, w, ch)
    up = rs.expected(rc, pooled, np.full(rc.out_span, rs.FILL, np.uint8))
    ac = pw.AddCase("resize_graph_add", batch * h * w, ch, a_zp=121, b_zp=121)
    total = pw.add_expected(ac, x, up)
    assert np.unique(pooled).size > 64 and np.unique(up).size > 64 and np.unique(total).size > 64

    ops = []
    try:
        st, p_op = pool.create(qnnp, pc)
        assert st == Status.success
        ops.append(p_op)
        r_op = qnnp.create_resize_bilinear2d_nhwc_u8(ch)
        ops.append(r_op)
        a_op = qnnp.create_add_nc_q8(ch, ac.a_zp, ac.a_scale, ac.b_zp, ac.b_scale, ac.y_zp, ac.y_scale, ac.qmin, ac.qmax, 0)
        ops.append(a_op)
        d_x = to_device(x)
        d_pool, d_up, d_sum = (to_device(np.full(n, rs.FILL, np.uint8)) for n in (pooled.size, up.size, total.size))
        assert pool.setup_status(qnnp, pc, p_op, batch, h, w, d_x, d_pool) == Status.success
        qnnp.setup_resize_bilinear2d_nhwc_u8(r_op, *rc.setup_args(d_pool, d_up))
        qnnp.setup_add_nc_q8(a_op, batch * h * w, d_x, ch, d_up, ch, d_sum, ch)
        qnnp.graph_begin()
        try:
            for op in ops:
                qnnp.run_operator(op)
            # neither create nor setup can be recorded
            assert qnnp.create_resize_bilinear2d_nhwc_u8_status(ch)[0] == Status.invalid_parameter
            assert qnnp.setup_resize_bilinear2d_nhwc_u8_status(r_op, *rc.setup_args(d_pool, d_up)) == Status.invalid_parameter
        finally:
            graph = qnnp.graph_end()
        assert np.all(from_device(d_sum) == rs.FILL), "nothing runs during the capture"
        try:
            for rep in range(2):
                for t in (d_pool, d_up, d_sum):
                    t.fill_(rs.FILL)
                torch.cuda.synchronize()
                qnnp.graph_launch(graph)
                qnnp.graph_synchronize(graph)
                _differences(from_device(d_pool), pooled, f"replay {rep}: average pooling")
                _differences(from_device(d_up), up, f"replay {rep}: resize ({qnnp.operator_kernel(r_op)})")
                _differences(from_device(d_sum), total, f"replay {rep}: add")
                _differences(from_device(d_x), x, f"replay {rep}: the input changed")
        finally:
            qnnp.graph_destroy(graph)
    finally:
        for op in ops:
            qnnp.delete_operator(op)


# ---- the one test ----------------------------------------------------------------------------------------------------
# All of the above under ONE test id, as tests/test_multiply_gpu.py groups its checks: the whole file runs in a few
# seconds and the GPU tier's count of test ids grows by one. A failure names the part, and the part names the case and
# the kernel.
PARTS = [_geometry_in_both_modes,                                                                  # 1
         _channels_dense_and_strided,                                                              # 2
         _base_misalignments,                                                                      # 3
         _nothing_is_written_outside_the_output,                                                   # 4
         _more_than_one_pass_of_each_loop,                                                         # 5
         _create_statuses, _setup_statuses_and_overlaps, _host_pointers_async_mode_and_resetup,    # 6
         _pool_resize_add_as_one_graph]                                                            # 7


def test_resize_bilinear(qnnp):
    for part in PARTS:
        try:
            part(qnnp)
        except AssertionError as e:
            raise AssertionError(f"{part.__name__.lstrip('_')}: {e}") from e
