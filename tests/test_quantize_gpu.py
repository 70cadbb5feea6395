"""GPU tier of the quantize and dequantize operators (hip/f32q8.hip behind quantize.c and dequantize.c).

No reference operator exists; the definition is bit-exact float32, and every expectation is its numpy restatement in
tests/_quantize.py. Bytes are compared as bytes, floats as uint32 bit patterns, the fill between strided rows and pixels
included; inputs must come back unchanged.

 1. values: every bucket centre, every tie with its float neighbours, the special values, NaNs of every kind and 65 536
    random bit patterns, for one parameter set per corner of the definition, through every row kernel;
 2. shapes: channel counts around the piece widths, batches, dense and padded strides, base misalignments on both
    sides, the kernel of each alignment class, more than one pass of each loop;
 3. planar: channel and pixel counts around the tile sizes, pixel strides, both directions, guarded at odd offsets;
 4. create and setup statuses, the switch between the two setups, host pointers, async mode, the streaming setting;
 5. quantize -> fully connected -> dequantize recorded into one hipGraph and replayed;
 6. rows whose float offsets pass 4 GiB.
"""
import numpy as np
import pytest

import _quantize as fq
from _cases import FcCase
from _gpu import Guarded, from_device, to_device
from _runner import fc_expected
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

F32 = np.float32
KERNELS = {d: {f"f32q8_{d}_x{w}" for w in (16, 4, 1)} for d in ("quantize", "dequantize")}


def _same(got, want, what):
    """bytes against bytes, or floats against floats by bit pattern"""
    assert got.size * got.itemsize == want.size * want.itemsize, (what, got.size, want.size)
    if want.dtype == np.float32:
        got, want = got.view(np.uint32), fq.bits(want)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ, first at {bad[:4]}: got {got[bad[:4]]}, want {want[bad[:4]]}")


def _quantize_rows(qnnp, op, q, s, x, f_mis=0, q_mis=0, what=""):
    """one rows run on fresh device buffers at the given base misalignments; returns the kernel name"""
    fs, qs = s.strides
    y = np.full(s.q_bytes, fq.FILL, np.uint8)
    d_x, d_y = to_device(x.view(np.uint8), f_mis), to_device(y, q_mis)
    assert qnnp.setup_quantize_nc_f32_q8_status(op, s.batch, d_x, fs, d_y, qs) == Status.success, what
    qnnp.run_operator(op)
    kernel = qnnp.operator_kernel(op)
    _same(from_device(d_y), fq.quantize_rows_expected(q, s, x, y), f"{what} ({kernel})")
    _same(from_device(d_x).view(np.uint32), fq.bits(x), f"{what} ({kernel}): input changed")
    assert kernel == fq.kernel_for("quantize", s, d_x.data_ptr(), d_y.data_ptr()), (what, kernel)
    return kernel


def _dequantize_rows(qnnp, op, q, s, y, f_mis=0, q_mis=0, what=""):
    fs, qs = s.strides
    x = fq.fill_f32(s.f_elements)
    d_y, d_x = to_device(y, q_mis), to_device(x.view(np.uint8), f_mis)
    assert qnnp.setup_dequantize_nc_q8_f32_status(op, s.batch, d_y, qs, d_x, fs) == Status.success, what
    qnnp.run_operator(op)
    kernel = qnnp.operator_kernel(op)
    _same(from_device(d_x).view(np.uint32), fq.dequantize_rows_expected(q, s, y, x), f"{what} ({kernel})")
    _same(from_device(d_y), y, f"{what} ({kernel}): input changed")
    assert kernel == fq.kernel_for("dequantize", s, d_x.data_ptr(), d_y.data_ptr()), (what, kernel)
    return kernel


# ---- 1. values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,q", fq.SETS, ids=[name for name, _ in fq.SETS])
def test_values_through_every_row_kernel(qnnp, name, q):
    x = fq.value_inputs(q)
    want = fq.quantize(x, q)
    assert np.unique(want).size == q.qmax - q.qmin + 1          # every byte of the range is reached
    s = fq.Rows(x.size, 1)
    op = qnnp.create_quantize_nc_f32_q8(x.size, *q.args())
    try:
        seen = {_quantize_rows(qnnp, op, q, s, x, f_mis, q_mis, f"values/{name}")
                for f_mis, q_mis in ((0, 0), (0, 4), (4, 8), (0, 1), (12, 3))}
        assert seen == KERNELS["quantize"]
    finally:
        qnnp.delete_operator(op)
    every = np.arange(256, dtype=np.uint8)
    s = fq.Rows(256, 1)
    op = qnnp.create_dequantize_nc_q8_f32(256, q.zp, q.scale)
    try:
        seen = {_dequantize_rows(qnnp, op, q, s, every, f_mis, q_mis, f"values/{name}")
                for f_mis, q_mis in ((0, 0), (4, 0), (0, 12), (0, 1), (8, 7))}
        assert seen == KERNELS["dequantize"]
    finally:
        qnnp.delete_operator(op)


# ---- 2. shapes ---------------------------------------------------------------------------------------------------
CHANNELS = (1, 3, 4, 15, 16, 17, 21, 33, 64, 100)
# byte-side base misaligned by 0 .. 15, the float side by 0 / 4 / 8 / 12 in turn; then the float side alone
MISALIGNMENTS = [(4 * ((b + b // 4) % 4), b) for b in range(16)] + [(4, 0), (8, 0), (12, 0)]


@pytest.mark.parametrize("direction", ["quantize", "dequantize"])
def test_row_shapes_strides_and_base_misalignments(qnnp, direction):
    assert {f for f, _ in MISALIGNMENTS} == {0, 4, 8, 12} and {b for _, b in MISALIGNMENTS} == set(range(16))
    q = fq.MID
    seen = set()
    for c in CHANNELS:
        if direction == "quantize":
            op = qnnp.create_quantize_nc_f32_q8(c, *q.args())
        else:
            op = qnnp.create_dequantize_nc_q8_f32(c, q.zp, q.scale)
        try:
            for batch in (1, 3):
                # dense; padded to the wide kernel's strides; padded off every grid
                for f_stride, q_stride in ((0, 0), (c + 4 - c % 4, c + 16 - c % 16), (c + 3, c + 5)):
                    s = fq.Rows(c, batch, f_stride, q_stride)
                    name = f"shape/{direction}/c{c}_b{batch}_f{f_stride}_q{q_stride}"
                    if direction == "quantize":
                        data = fq.float_inputs(name, s.f_elements, q)
                    else:
                        data = np.random.default_rng(fq._seed(name)).integers(0, 256, size=s.q_bytes, dtype=np.uint8)
                    for f_mis, q_mis in MISALIGNMENTS:
                        run = _quantize_rows if direction == "quantize" else _dequantize_rows
                        seen.add(run(qnnp, op, q, s, data, f_mis, q_mis, f"{name}_m{f_mis}_{q_mis}"))
        finally:
            qnnp.delete_operator(op)
    assert seen == KERNELS[direction]


def test_dense_3_and_21_channel_tensors_take_the_wide_kernel(qnnp):
    """rows dense on both sides are one long row, whatever the channel count; a last piece may be partial"""
    q = fq.MID
    for c, pixels in ((3, 224), (21, 64), (3, 37), (21, 5)):
        s = fq.Rows(c, pixels)
        op = qnnp.create_quantize_nc_f32_q8(c, *q.args())
        try:
            x = fq.float_inputs(f"dense/{c}/{pixels}", s.f_elements, q)
            assert _quantize_rows(qnnp, op, q, s, x, what=f"dense quantize c{c} x {pixels}") == "f32q8_quantize_x16"
        finally:
            qnnp.delete_operator(op)
        op = qnnp.create_dequantize_nc_q8_f32(c, q.zp, q.scale)
        try:
            y = np.random.default_rng(c * pixels).integers(0, 256, size=s.q_bytes, dtype=np.uint8)
            assert _dequantize_rows(qnnp, op, q, s, y, what=f"dense dequantize c{c} x {pixels}") == "f32q8_dequantize_x16"
        finally:
            qnnp.delete_operator(op)


def test_more_than_one_pass_of_each_row_loop(qnnp):
    """hip/f32q8.hip launches at most compute units x 16 workgroups; beyond that its grid-stride loops take further
    passes: short rows whose row groups exceed one pass of grid x, and one long row with more 256-piece chunks than
    one pass of grid y, for each piece width that keeps the tensors small"""
    cap = qnnp.device_info()["compute_units"] * 16
    q = fq.MID
    cases = [
        # rows of 129 pieces: one row a workgroup, more rows than the cap (the byte kernel: 129 bytes a row)
        (fq.Rows(129, cap + 3, 130, 131), 0, 0, "x1"),
        (fq.Rows(4 * 129, cap + 3, 4 * 129 + 1, 4 * 130), 0, 0, "x4"),
        # short strided rows, 256 rows a workgroup: rows beyond one workgroup
        (fq.Rows(16, 700, 20, 32), 0, 0, "x16"),
        # one row of more chunks than the cap, with a partial last piece
        (fq.Rows(cap * 256 + 301, 1), 0, 1, "x1"),
        (fq.Rows(4 * (cap * 256 + 301) + 3, 1), 0, 4, "x4"),
        (fq.Rows(16 * (cap * 256 + 301) + 7, 1), 0, 0, "x16"),
    ]
    for s, f_mis, q_mis, width in cases:
        name = f"sweep/{width}_c{s.channels}_b{s.batch}"
        op = qnnp.create_quantize_nc_f32_q8(s.channels, *q.args())
        try:
            x = np.resize(fq.float_inputs(name, min(s.f_elements, 1 << 20), q), s.f_elements)    # (repeats beyond 2^20)
            assert _quantize_rows(qnnp, op, q, s, x, f_mis, q_mis, name) == f"f32q8_quantize_{width}"
        finally:
            qnnp.delete_operator(op)
        op = qnnp.create_dequantize_nc_q8_f32(s.channels, q.zp, q.scale)
        try:
            y = np.resize(np.random.default_rng(fq._seed(name)).integers(0, 256, size=min(s.q_bytes, 1 << 20), dtype=np.uint8), s.q_bytes)
            assert _dequantize_rows(qnnp, op, q, s, y, f_mis, q_mis, name) == f"f32q8_dequantize_{width}"
        finally:
            qnnp.delete_operator(op)


# ---- 3. planar ---------------------------------------------------------------------------------------------------
def _planar_both_directions(qnnp, q, s, offset, what):
    """quantize NCHW floats -> NHWC bytes, then dequantize those bytes back, on guarded buffers at byte offset `offset`
    (the float side keeps its 4-byte alignment: offset rounded down to a multiple of 4)"""
    x = fq.float_inputs(what, s.f_elements, q)
    y0 = np.full(s.q_bytes, fq.FILL, np.uint8)
    gx, gy = Guarded(x, offset & ~3), Guarded(y0, offset)
    op = qnnp.create_quantize_nc_f32_q8(s.channels, *q.args())
    try:
        assert qnnp.setup_quantize_nchw_f32_nhwc_q8_status(op, s.batch, s.pixels, gx, gy, s.stride) == Status.success, what
        qnnp.run_operator(op)
        assert qnnp.operator_kernel(op) == "f32q8_quantize_planar"
        want = fq.quantize_planar_expected(q, s, x, y0)
        _same(gy.read(), want, f"{what}: quantize")
        gy.assert_intact(f"{what}: quantize")
        gx.assert_intact(f"{what}: quantize (input)")
        _same(gx.read().view(np.uint32), fq.bits(x), f"{what}: quantize changed its input")
    finally:
        qnnp.delete_operator(op)
    gz = Guarded(fq.fill_f32(s.f_elements), (offset * 4) % 64)
    op = qnnp.create_dequantize_nc_q8_f32(s.channels, q.zp, q.scale)
    try:
        assert qnnp.setup_dequantize_nhwc_q8_nchw_f32_status(op, s.batch, s.pixels, gy, s.stride, gz) == Status.success, what
        qnnp.run_operator(op)
        assert qnnp.operator_kernel(op) == "f32q8_dequantize_planar"
        _same(gz.read().view(np.uint32), fq.dequantize_planar_expected(q, s, want), f"{what}: dequantize")
        gz.assert_intact(f"{what}: dequantize")
        gy.assert_intact(f"{what}: dequantize (input)")
        _same(gy.read(), want, f"{what}: dequantize changed its input")
    finally:
        qnnp.delete_operator(op)


@pytest.mark.parametrize("channels", [1, 3, 4, 21, 33])
def test_planar_shapes_both_directions_guarded(qnnp, channels):
    k = 0
    for pixels in (1, 7, 63, 64, 65, 200):
        for batch in (1, 3):
            for extra in (0, 5):
                s = fq.Planar(channels, pixels, batch, extra)
                _planar_both_directions(qnnp, fq.MID, s, k % 16, f"planar/c{channels}_p{pixels}_b{batch}_e{extra}_o{k % 16}")
                k += 1


def test_planar_tiles_of_every_size_and_more_than_one_pass(qnnp):
    """a tile is up to 64 channels x 1024 (up to 16 channels), 512 (up to 32) or 256 pixels: pixel counts around each,
    more than one channel tile with a short last one, every byte-side alignment of a dense tensor, and more tiles than
    the launch cap of compute units x 16"""
    cap = qnnp.device_info()["compute_units"] * 16
    q = fq.Quant(7, 0.031, 3, 250)
    shapes = [fq.Planar(3, 1023, 2), fq.Planar(3, 1024, 1), fq.Planar(3, 2500, 2), fq.Planar(16, 1025, 1),
              fq.Planar(17, 513, 2), fq.Planar(21, 1100, 1), fq.Planar(32, 512, 1), fq.Planar(33, 257, 2, 3),
              fq.Planar(64, 300, 1), fq.Planar(65, 256, 2), fq.Planar(70, 257, 2), fq.Planar(150, 40, 2, 6),
              fq.Planar(1, 2057, 1), fq.Planar(2, 1, cap + 5), fq.Planar(1, 3, cap + 5, 2)]
    for k, s in enumerate(shapes):
        _planar_both_directions(qnnp, q, s, (k * 5) % 16, f"tiles/c{s.channels}_p{s.pixels}_b{s.batch}_e{s.extra}")
    for offset in range(16):
        _planar_both_directions(qnnp, q, fq.Planar(3, 70, 2), offset, f"tiles/alignment_{offset}")


# ---- 4. API ------------------------------------------------------------------------------------------------------
INF, NAN = float("inf"), float("nan")
# (channels, zero point, scale, min, max) -> status, in the documented order
QUANTIZE_CREATE = [
    ((8, 114, 0.0186, 0, 255), Status.success),
    ((1, 255, fq.SCALE_MIN, 0, 1), Status.success),
    ((2 ** 31 - 1, 0, fq.SCALE_MAX, 254, 255), Status.success),
    ((0, 114, 0.0186, 0, 255), Status.invalid_parameter),
    ((0, 114, 0.0, 9, 1), Status.invalid_parameter),
    ((8, 114, 0.0, 0, 255), Status.invalid_parameter),
    ((8, 114, -0.5, 0, 255), Status.invalid_parameter),
    ((8, 114, 1e-40, 0, 255), Status.invalid_parameter),
    ((8, 114, INF, 0, 255), Status.invalid_parameter),
    ((8, 114, NAN, 0, 255), Status.invalid_parameter),
    ((8, 114, 0.0186, 100, 100), Status.invalid_parameter),
    ((8, 114, 0.0186, 200, 100), Status.invalid_parameter),
    ((2 ** 31, 114, 0.0186, 200, 100), Status.invalid_parameter),           # invalid before unsupported
    ((8, 114, 2.0 ** -120, 200, 100), Status.invalid_parameter),
    ((2 ** 31, 114, 0.0186, 0, 255), Status.unsupported_parameter),
    ((8, 114, 2.0 ** -119, 0, 255), Status.unsupported_parameter),
    ((8, 114, float(np.nextafter(F32(fq.SCALE_MIN), F32(0))), 0, 255), Status.unsupported_parameter),
    ((8, 114, float(np.nextafter(F32(fq.SCALE_MAX), F32(INF))), 0, 255), Status.unsupported_parameter),
    ((8, 114, 2.0 ** 127, 0, 255), Status.unsupported_parameter)]
# (channels, zero point, scale) -> status
DEQUANTIZE_CREATE = [(args[:3], st) for args, st in QUANTIZE_CREATE if args[3:] == (0, 255)] + [
    ((1, 255, fq.SCALE_MIN), Status.success), ((2 ** 31 - 1, 0, fq.SCALE_MAX), Status.success),
    ((2 ** 31, 0, NAN), Status.invalid_parameter)]


def test_create_statuses(qnnp):
    for create, table in ((qnnp.create_quantize_nc_f32_q8_status, QUANTIZE_CREATE),
                          (qnnp.create_dequantize_nc_q8_f32_status, DEQUANTIZE_CREATE)):
        for args, want in table:
            st, op = create(*args)
            if op:
                qnnp.delete_operator(op)
            assert st == want and bool(op) == (want == Status.success), (args, st)
    st, op = qnnp.create_quantize_nc_f32_q8_status(8, *fq.MID.args(), flags=0xFFFFFFFF)     # accepted and ignored
    assert st == Status.success
    assert qnnp.run_operator_status(op) == Status.invalid_parameter                          # before any setup
    qnnp.delete_operator(op)
    st, op = qnnp.create_dequantize_nc_q8_f32_status(8, 3, 0.5, flags=0xFFFFFFFF)
    assert st == Status.success
    assert qnnp.run_operator_status(op) == Status.invalid_parameter
    qnnp.delete_operator(op)


def test_setup_statuses_switches_and_refusals(qnnp):
    c = 16
    q = fq.MID
    quant = qnnp.create_quantize_nc_f32_q8(c, *q.args())
    dequant = qnnp.create_dequantize_nc_q8_f32(c, q.zp, q.scale)
    clamp = qnnp.create_clamp_nc_u8(c, 0, 255)
    x = fq.float_inputs("setup", 6 * c * 4, q)
    d_f = to_device(x)                                        # 1536 bytes of floats
    d_q = to_device(np.full(4096, fq.FILL, np.uint8))
    f, b = d_f.data_ptr(), d_q.data_ptr()
    sq, sqp = qnnp.setup_quantize_nc_f32_q8_status, qnnp.setup_quantize_nchw_f32_nhwc_q8_status
    sd, sdp = qnnp.setup_dequantize_nc_q8_f32_status, qnnp.setup_dequantize_nhwc_q8_nchw_f32_status
    try:
        # no rows: success, and run does nothing, whatever the pointers
        for st in (sq(quant, 0, None, 0, None, 0), sqp(quant, 0, 0, None, None, 0), sd(dequant, 0, None, 0, None, 0),
                   sdp(dequant, 0, 0, None, 0, None)):
            assert st == Status.success
        assert qnnp.run_operator_status(quant) == Status.success and qnnp.run_operator_status(dequant) == Status.success
        assert np.all(from_device(d_q) == fq.FILL)
        inv, uns = Status.invalid_parameter, Status.unsupported_parameter
        # NULL tensors, no pixels, float alignment, strides
        assert sq(quant, 3, None, c, d_q, c) == inv and sq(quant, 3, d_f, c, None, c) == inv
        assert sqp(quant, 1, 3, None, d_q, c) == inv and sqp(quant, 1, 3, d_f, None, c) == inv
        assert sd(dequant, 3, None, c, d_f, c) == inv and sd(dequant, 3, d_q, c, None, c) == inv
        assert sdp(dequant, 1, 3, None, c, d_f) == inv and sdp(dequant, 1, 3, d_q, c, None) == inv
        assert sqp(quant, 1, 0, d_f, d_q, c) == inv and sdp(dequant, 1, 0, d_q, c, d_f) == inv
        for off in (1, 2, 3):
            assert sq(quant, 3, f + off, c, d_q, c) == inv and sqp(quant, 1, 3, f + off, d_q, c) == inv
            assert sd(dequant, 3, d_q, c, f + off, c) == inv and sdp(dequant, 1, 3, d_q, c, f + off) == inv
        assert sq(quant, 3, d_f, c - 1, d_q, c) == inv and sq(quant, 3, d_f, c, d_q, c - 1) == inv
        assert sd(dequant, 3, d_q, c - 1, d_f, c) == inv and sd(dequant, 3, d_q, c, d_f, c - 1) == inv
        assert sqp(quant, 1, 3, d_f, d_q, c - 1) == inv and sdp(dequant, 1, 3, d_q, c - 1, d_f) == inv
        # overlaps: spans are in bytes, 4 per float element -- 3 rows of 16 floats are 192 bytes
        assert sq(quant, 3, d_f, c, f, c) == inv and sq(quant, 3, d_f, c, f + 191, c) == inv
        assert sq(quant, 3, f + 44, c, d_f, c) == inv and sq(quant, 3, f + 48, c, d_f, c) == Status.success
        assert sd(dequant, 3, d_f, c, d_f, c) == inv and sd(dequant, 3, f + 191, c, d_f, c) == inv
        assert sqp(quant, 1, 3, d_f, f + 191, c) == inv and sdp(dequant, 1, 3, f + 100, c, d_f) == inv
        assert sq(quant, 3, d_f, c, f + 192, c) == Status.success        # right behind the floats
        assert sd(dequant, 3, f + 192, c, d_f, c) == Status.success
        # the index range, by status alone
        for batch in (2 ** 31, 2 ** 40, 2 ** 64 - 1):
            assert sq(quant, batch, d_f, c, d_q, c) == uns and sd(dequant, batch, d_q, c, d_f, c) == uns
        for batch, pixels in ((2 ** 31, 1), (1, 2 ** 31), (65536, 32768), (1, 2 ** 27), (2 ** 33, 2 ** 31),
                              (2 ** 64 - 1, 2 ** 64 - 1), (2 ** 32, 2 ** 32)):
            assert sqp(quant, batch, pixels, d_f, d_q, c) == uns, (batch, pixels)
            assert sdp(dequant, batch, pixels, d_q, c, d_f) == uns, (batch, pixels)
        # operator kinds
        assert sq(dequant, 3, d_f, c, d_q, c) == inv and sqp(dequant, 1, 3, d_f, d_q, c) == inv
        assert sd(quant, 3, d_q, c, d_f, c) == inv and sdp(quant, 1, 3, d_q, c, d_f) == inv
        assert sq(clamp, 3, d_f, c, d_q, c) == inv and sd(clamp, 3, d_q, c, d_f, c) == inv
        assert sq(None, 3, d_f, c, d_q, c) == inv and sdp(None, 1, 3, d_q, c, d_f) == inv
        assert qnnp.setup_clamp_nc_u8_status(quant, 3, d_q, c, b + 1024, c) == inv

        # one handle, set up rows -> planar -> rows; a refused setup in between leaves the last one runnable
        rows, planar = fq.Rows(c, 6, 0, 24), fq.Planar(c, 6, 1, 8)
        want_rows = fq.quantize_rows_expected(q, rows, x[:6 * c], np.full(rows.q_bytes, fq.FILL, np.uint8))
        want_planar = fq.quantize_planar_expected(q, planar, x[:6 * c], np.full(planar.q_bytes, fq.FILL, np.uint8))
        assert not np.array_equal(want_rows, want_planar)
        for setup, want in ((lambda: sq(quant, 6, d_f, c, d_q, 24), want_rows),
                            (lambda: sqp(quant, 1, 6, d_f, d_q, 24), want_planar),
                            (lambda: sq(quant, 6, d_f, c, d_q, 24), want_rows)):
            assert setup() == Status.success
            for refused in (lambda: sq(quant, 6, d_f, c - 1, d_q, 24), lambda: sqp(quant, 1, 0, d_f, d_q, 24),
                            lambda: sq(quant, 6, None, c, d_q, 24), lambda: sqp(quant, 2 ** 31, 6, d_f, d_q, 24), None):
                if refused is not None:
                    assert refused() in (inv, uns)
                d_q.fill_(fq.FILL)
                qnnp.run_operator(quant)
                _same(from_device(d_q)[:want.size], want, "quantize after a setup switch")
        d_q.copy_(to_device(np.arange(4096, dtype=np.uint32).astype(np.uint8) * 7))
        y = from_device(d_q)
        d_out = to_device(fq.fill_f32(6 * c))
        want_rows = fq.dequantize_rows_expected(q, rows, y[:rows.q_bytes], fq.fill_f32(6 * c))
        want_planar = fq.dequantize_planar_expected(q, planar, y[:planar.q_bytes])
        for setup, want in ((lambda: sdp(dequant, 1, 6, d_q, 24, d_out), want_planar),
                            (lambda: sd(dequant, 6, d_q, 24, d_out, c), want_rows),
                            (lambda: sdp(dequant, 1, 6, d_q, 24, d_out), want_planar)):
            assert setup() == Status.success
            assert sd(dequant, 6, d_q, c - 1, d_out, c) == inv and sdp(dequant, 1, 6, d_q, 24, d_out.data_ptr() + 2) == inv
            qnnp.run_operator(dequant)
            _same(from_device(d_out).view(np.uint32), want, "dequantize after a setup switch")
    finally:
        for op in (quant, dequant, clamp):
            qnnp.delete_operator(op)


def test_host_pointers_async_mode_and_the_streaming_setting(qnnp):
    import torch
    q = fq.MID
    # host tensors on both sides, rows (dense and strided) and planar
    for s in (fq.Rows(40, 3), fq.Rows(40, 3, 45, 47)):
        x = fq.float_inputs(f"host/{s}", s.f_elements, q)
        y = np.full(s.q_bytes, fq.FILL, np.uint8)
        op = qnnp.create_quantize_nc_f32_q8(s.channels, *q.args())
        try:
            want = fq.quantize_rows_expected(q, s, x, y)
            x0 = x.copy()
            assert qnnp.setup_quantize_nc_f32_q8_status(op, s.batch, x, s.strides[0], y, s.strides[1]) == Status.success
            qnnp.run_operator(op)
            _same(y, want, f"host quantize {s}")
            _same(x, x0, "host quantize changed its input")
        finally:
            qnnp.delete_operator(op)
        op = qnnp.create_dequantize_nc_q8_f32(s.channels, q.zp, q.scale)
        try:
            z = fq.fill_f32(s.f_elements)
            back = fq.dequantize_rows_expected(q, s, want, z)
            assert qnnp.setup_dequantize_nc_q8_f32_status(op, s.batch, want, s.strides[1], z, s.strides[0]) == Status.success
            qnnp.run_operator(op)
            _same(z, back, f"host dequantize {s}")
        finally:
            qnnp.delete_operator(op)
    p = fq.Planar(3, 50, 2, 4)
    x = fq.float_inputs("host/planar", p.f_elements, q)
    y = np.full(p.q_bytes, fq.FILL, np.uint8)
    op = qnnp.create_quantize_nc_f32_q8(3, *q.args())
    de = qnnp.create_dequantize_nc_q8_f32(3, q.zp, q.scale)
    try:
        want = fq.quantize_planar_expected(q, p, x, y)
        assert qnnp.setup_quantize_nchw_f32_nhwc_q8_status(op, 2, 50, x, y, p.stride) == Status.success
        qnnp.run_operator(op)
        _same(y, want, "host planar quantize")
        z = fq.fill_f32(p.f_elements)
        assert qnnp.setup_dequantize_nhwc_q8_nchw_f32_status(de, 2, 50, y, p.stride, z) == Status.success
        qnnp.run_operator(de)
        _same(z, fq.dequantize_planar_expected(q, p, want), "host planar dequantize")
    finally:
        qnnp.delete_operator(op)
        qnnp.delete_operator(de)

    # async mode, three runs, with the streaming-store setting off, on and following the process: identical results
    rows, planar = fq.Rows(96, 4 * 28 * 28), fq.Planar(3, 56 * 56, 4)
    x = fq.float_inputs("async", rows.f_elements, q)
    assert rows.f_elements >= planar.f_elements
    d_x, d_y = to_device(x), to_device(np.full(rows.q_bytes, fq.FILL, np.uint8))
    d_z = to_device(fq.fill_f32(rows.f_elements))
    op = qnnp.create_quantize_nc_f32_q8(96, *q.args())
    op3 = qnnp.create_quantize_nc_f32_q8(3, *q.args())
    de = qnnp.create_dequantize_nc_q8_f32(96, q.zp, q.scale)
    de3 = qnnp.create_dequantize_nc_q8_f32(3, q.zp, q.scale)
    try:
        qnnp.set_async(True)
        want_rows = fq.quantize(x, q)
        y0 = np.full(planar.q_bytes, fq.FILL, np.uint8)
        want_planar = fq.quantize_planar_expected(q, planar, x[:planar.f_elements], y0)
        qnnp.setup_quantize_nc_f32_q8(op, rows.batch, d_x, 96, d_y, 96)
        qnnp.setup_quantize_nchw_f32_nhwc_q8(op3, 4, planar.pixels, d_x, d_y, 3)
        qnnp.setup_dequantize_nc_q8_f32(de, rows.batch, d_y, 96, d_z, 96)
        qnnp.setup_dequantize_nhwc_q8_nchw_f32(de3, 4, planar.pixels, d_y, 3, d_z)
        for streaming in (1, 0, -1):
            for handle in (op, op3, de, de3):
                qnnp.operator_set_streaming_stores(handle, streaming)
            for handle, kernel, want_q, want_f in (
                    (op, "f32q8_quantize_x16", want_rows, fq.dequantize(want_rows, q)),
                    (op3, "f32q8_quantize_planar", want_planar, fq.dequantize_planar_expected(q, planar, want_planar))):
                d_y.fill_(fq.FILL)
                d_z.copy_(to_device(fq.fill_f32(rows.f_elements)))
                for _ in range(3):
                    qnnp.run_operator(handle)
                    qnnp.run_operator(de if handle == op else de3)
                qnnp.synchronize()
                torch.cuda.synchronize()
                assert qnnp.operator_kernel(handle) == kernel
                _same(from_device(d_y)[:want_q.size], want_q, f"async {kernel}, streaming {streaming}")
                _same(from_device(d_z).view(np.uint32)[:want_f.size], want_f, f"async dequantize after {kernel}, streaming {streaming}")
        qnnp.set_async(False)
        assert qnnp.time_operator(op, 1, 3) > 0.0 and qnnp.time_operator(de3, 1, 3) > 0.0
    finally:
        qnnp.set_async(False)
        for handle in (op, op3, de, de3):
            qnnp.delete_operator(handle)


# ---- 5. a chain in one hipGraph ------------------------------------------------------------------------------------
def test_quantize_fully_connected_dequantize_as_one_graph(qnnp):
    """float [5][24] -> quantize -> FC 24 -> 10 -> dequantize -> float [5][10], on device buffers, captured once and
    replayed twice; expectations: the numpy ends around tests/_runner.py:fc_expected"""
    import torch
    batch, cin, cout = 5, 24, 10
    rng = np.random.default_rng(fq._seed("chain"))
    q_in = fq.Quant(121, 0.05)
    x = fq.float_inputs("chain", batch * cin, q_in)
    k = rng.integers(0, 256, size=(cout, cin), dtype=np.uint8)
    b = rng.integers(-2000, 2001, size=cout, dtype=np.int32)
    fc = FcCase("chain_fc", batch, cin, cout, izp=q_in.zp)
    xq = fq.quantize(x, q_in)
    assert np.unique(xq).size > 50
    mid, (scale, zp) = fc_expected(fc, xq, k, b)
    q_out = fq.Quant(int(zp), 0.37)
    want = fq.dequantize(mid, q_out)
    assert np.unique(mid).size > 8

    ops = []
    try:
        quant = qnnp.create_quantize_nc_f32_q8(cin, *q_in.args())
        ops.append(quant)
        op = qnnp.create_fully_connected_nc_q8(cin, cout, fc.izp, 1.0, fc.kzp, 1.0, k, b, int(zp), float(scale), 0, 255, 0)
        ops.append(op)
        dequant = qnnp.create_dequantize_nc_q8_f32(cout, q_out.zp, q_out.scale)
        ops.append(dequant)
        d_x = to_device(x)
        d_q, d_mid = to_device(np.full(batch * cin, fq.FILL, np.uint8)), to_device(np.full(batch * cout, fq.FILL, np.uint8))
        d_out = to_device(fq.fill_f32(batch * cout))
        qnnp.setup_quantize_nc_f32_q8(quant, batch, d_x, cin, d_q, cin)
        qnnp.setup_fully_connected_nc_q8(op, batch, d_q, cin, d_mid, cout)
        qnnp.setup_dequantize_nc_q8_f32(dequant, batch, d_mid, cout, d_out, cout)
        qnnp.graph_begin()
        try:
            for handle in ops:
                qnnp.run_operator(handle)
            # neither create nor setup can be recorded
            assert qnnp.create_quantize_nc_f32_q8_status(cin, *q_in.args())[0] == Status.invalid_parameter
            assert qnnp.create_dequantize_nc_q8_f32_status(cout, 3, 0.5)[0] == Status.invalid_parameter
            assert qnnp.setup_quantize_nc_f32_q8_status(quant, batch, d_x, cin, d_q, cin) == Status.invalid_parameter
            assert qnnp.setup_quantize_nchw_f32_nhwc_q8_status(quant, 1, batch, d_x, d_q, cin) == Status.invalid_parameter
            assert qnnp.setup_dequantize_nc_q8_f32_status(dequant, batch, d_mid, cout, d_out, cout) == Status.invalid_parameter
            assert qnnp.setup_dequantize_nhwc_q8_nchw_f32_status(dequant, 1, batch, d_mid, cout, d_out) == Status.invalid_parameter
        finally:
            graph = qnnp.graph_end()
        assert np.all(from_device(d_q) == fq.FILL), "nothing runs during the capture"
        try:
            for rep in range(2):
                d_q.fill_(fq.FILL)
                d_mid.fill_(fq.FILL)
                d_out.copy_(to_device(fq.fill_f32(batch * cout)))
                torch.cuda.synchronize()
                qnnp.graph_launch(graph)
                qnnp.graph_synchronize(graph)
                _same(from_device(d_q), xq, f"replay {rep}: quantize")
                _same(from_device(d_mid), mid, f"replay {rep}: fully connected")
                _same(from_device(d_out).view(np.uint32), want, f"replay {rep}: dequantize")
        finally:
            qnnp.graph_destroy(graph)
    finally:
        for handle in ops:
            qnnp.delete_operator(handle)


# ---- 6. float offsets past 4 GiB -----------------------------------------------------------------------------------
def test_rows_whose_float_offsets_pass_4_gib(qnnp):
    """three rows of 1024 channels, 2^29 float elements apart: the last row starts 4 GiB into the float tensor. Only
    the rows and their neighbourhoods are written and compared; the gigabytes between them are never touched."""
    import torch
    c, stride, near = 1024, 2 ** 29, 256
    s = fq.Rows(c, 3, stride, c)
    q = fq.MID
    big = torch.empty(s.f_elements * 4, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 16 == 0 and (2 * stride) * 4 == 2 ** 32
    words = big.view(torch.int32)
    fill_word = int(np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0])

    def window(r):
        """the row's elements with `near` elements on each side, inside the tensor"""
        return max(r * stride - near, 0), min(r * stride + c + near, s.f_elements)

    x = fq.float_inputs("far", 3 * c, q).reshape(3, c)
    for r in range(3):
        lo, hi = window(r)
        words[lo:hi] = fill_word
        words[r * stride:r * stride + c] = torch.from_numpy(x[r].view(np.int32).copy()).cuda()
    d_y = to_device(np.full(3 * c, fq.FILL, np.uint8))
    op = qnnp.create_quantize_nc_f32_q8(c, *q.args())
    try:
        qnnp.setup_quantize_nc_f32_q8(op, 3, big, stride, d_y, c)
        qnnp.run_operator(op)
        assert qnnp.operator_kernel(op) == "f32q8_quantize_x16"
        want = fq.quantize(x.reshape(-1), q)
        _same(from_device(d_y), want, "quantize from rows 2 GiB apart")
    finally:
        qnnp.delete_operator(op)
    # back into the same tensor: the rows are rewritten, their neighbourhoods stay
    for r in range(3):
        lo, hi = window(r)
        words[lo:hi] = fill_word
    op = qnnp.create_dequantize_nc_q8_f32(c, q.zp, q.scale)
    try:
        qnnp.setup_dequantize_nc_q8_f32(op, 3, d_y, c, big, stride)
        qnnp.run_operator(op)
        assert qnnp.operator_kernel(op) == "f32q8_dequantize_x16"
        back = fq.dequantize(want, q).reshape(3, c)
        for r in range(3):
            lo, hi = window(r)
            got = from_device(words[lo:hi]).view(np.uint32)
            expect = np.full(hi - lo, 0xA5A5A5A5, np.uint32)
            expect[r * stride - lo:r * stride - lo + c] = fq.bits(back[r])
            _same(got, expect, f"dequantize to row {r}, 2 GiB apart")
    finally:
        qnnp.delete_operator(op)
        del words, big
        torch.cuda.empty_cache()
