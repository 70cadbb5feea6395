"""GPU tier: a byte table attached to a convolution (qnnp_gfx950_attach_output_table, output-table.c; the table flavours
of hip/q8pwconv.hip's kernel units, hip/q8dwcol.hip and hip/q8dwcol5.hip, the in-place launch of hip/x8lut.hip everywhere else).

Every case is compared twice -- with the ORACLE's convolution bytes mapped through the table in numpy, and with the
library's own chain (convolution, then the stand-alone table operator in place on its output) -- on guarded outputs whose
bytes before, after and between strided pixels must stay as they were (tests/_output_table.py), and asserts the kernel's
name and whether the lookup rode in its epilogue.

Shapes are the smallest at which the kernels can go wrong. Pointwise: 2 x 5 x 7 = 70 rows (a partial last 32-row unit) of
K = 24 (8-byte activation loads), and every way out of the streaming kernels: n = 48 dense (one contiguous run), n = 24
dense (the 8-byte-row walk), n = 48 in pixels of 64 bytes and n = 128 split over workgroup columns (row chunks), n = 40 in
pixels of 56 bytes and n = 20 (dword stores), n = 7 (byte stores). n = 40 is no multiple of 16, so it leaves through dword
stores, not through row chunks; the chunks have the two cases named before it. The one-wave-per-block kernel ("gemm_kernel"
6) reads whole 16-byte pieces and refuses K = 24 with or without a table: that refusal is a case, and the kernel runs K = 32
(one wave per block) and K = 272 (the reduction split over the waves). Depthwise: 5 x 7 images, batch 2.

Without a GPU-side fold (table_folded == 0): a dense 3 x 3 on the generic tile kernel, a fully connected layer, per-channel
convolution and depthwise, the automatic choice at 70 rows (none of the streaming kernels), 3 x 3 depthwise layers kernel G
does not take (C = 6; pixels of C + 5 bytes), and a streaming-kernel launch whose LDS has no room for the table at its
residency.

Run time on an MI355X: see profiles/output_table/README.md.
"""
import numpy as np
import pytest

import _fused as F
import _output_table as T
import _perchannel as PC
from _output_table import Case
from _runner import FILL, assert_bytes_equal
from qnnpack_amd import QnnpackError, Status

pytestmark = pytest.mark.gpu

PW, LONGK, GW, GWK = T.PW_KERNELS
COL, COL_DOT4, COL_DILATED, COL5 = T.DW_KERNELS
OTHER = ""            # any kernel outside the carrying families (tests/_output_table.py hold)


def dw(name, c, **kw):
    kw.setdefault("kernel", 3)
    kw.setdefault("family", "dwconv_kernel")
    return Case(name, gic=1, goc=1, groups=c, **kw)


# ---- pointwise: every way out of the streaming kernels -----------------------------------------------------------------
WIDTHS = [("n48_dense", dict(goc=48)), ("n24_dense8", dict(goc=24)), ("n48_stride64_chunks", dict(goc=48, out_extra=16)),
          ("n128_columns", dict(goc=128)), ("n40_stride56_dwords", dict(goc=40, out_extra=16)), ("n20_dwords", dict(goc=20)),
          ("n7_bytes", dict(goc=7))]
POINTWISE = (
    [Case(f"pw_code5_{tag}", code=5, want=PW, **kw) for tag, kw in WIDTHS] +
    [Case(f"pw_code5_{tag}_hardswish", code=5, want=PW, table="hardswish", **kw) for tag, kw in WIDTHS[:1]] +
    [Case(f"pw_code5_{tag}_clamp", code=5, want=PW, clamp=(10, 200), **kw) for tag, kw in (WIDTHS[0], WIDTHS[5])] +
    # one channel block per row and 16-byte loads: the direct-store kernel with 16-byte stores
    [Case("pw_code5_k32_n32", gic=32, goc=32, code=5, want=PW)] +
    [Case(f"pw_code6_k32_{tag}", gic=32, code=6, want=GW, **kw) for tag, kw in WIDTHS] +
    [Case("pw_code6_k32_hardswish", gic=32, code=6, want=GW, table="hardswish"),
     Case("pw_code6_k32_clamp", gic=32, code=6, want=GW, clamp=(10, 200)),
     Case("pw_code6_k272_split", gic=272, code=6, want=GWK),
     Case("pw_code6_k272_split_n20", gic=272, goc=20, code=6, want=GWK),
     Case("pw_code9_k272", gic=272, code=9, want=LONGK),
     Case("pw_code9_k272_stride64", gic=272, out_extra=16, code=9, want=LONGK),
     Case("pw_code9_k272_hardswish", gic=272, code=9, want=LONGK, table="hardswish"),
     Case("pw_code9_k272_clamp", gic=272, code=9, want=LONGK, clamp=(10, 200))])
# the automatic choice at 70 rows is none of the streaming kernels: no table flavour, the in-place launch
AUTO = [Case(f"pw_auto_{tag}", want=OTHER, folded=0, **kw) for tag, kw in WIDTHS]


@pytest.mark.parametrize("case", POINTWISE + AUTO, ids=lambda c: c.name)
def test_pointwise(qnnp, case):
    T.hold(qnnp, case)


def test_the_one_wave_per_block_kernel_refuses_k24_with_and_without_a_table(qnnp):
    """K = 24 is not a whole number of 16-byte pieces: "gemm_kernel" 6 refuses the layer at run, and a table changes
    nothing about that"""
    case = Case("pw_code6_k24", code=6)
    p = T.problem(case)
    from _gpu import to_device
    d_in, d_out = to_device(p.x), to_device(np.full(p.plain().size, FILL, np.uint8))
    conv, lut = p.create(qnnp), p.create_table(qnnp)
    try:
        qnnp.set_option("gemm_kernel", 6)
        p.setup(qnnp, conv, d_in, d_out)
        with pytest.raises(QnnpackError) as plain:
            qnnp.run_operator(conv)
        qnnp.attach_output_table(conv, lut)
        with pytest.raises(QnnpackError) as attached:
            qnnp.run_operator(conv)
        assert plain.value.status == attached.value.status
        assert qnnp.operator_table_folded(conv) == 0
    finally:
        qnnp.set_option("gemm_kernel", 0)
        qnnp.delete_operator(conv)
        qnnp.delete_operator(lut)


# ---- depthwise column walks --------------------------------------------------------------------------------------------
DEPTHWISE = [
    dw("dw_c8_s1", 8, want=COL_DOT4),
    dw("dw_c24_s1", 24, want=COL_DOT4),
    dw("dw_c8_s2", 8, stride=2, want=COL),
    dw("dw_c24_s2", 24, stride=2, want=COL),
    dw("dw_c24_dilated", 24, dilation=2, want=COL_DILATED),
    dw("dw_c24_s1_stride29", 24, out_extra=5, want=OTHER, folded=0),                     # pixels of C + 5 bytes: no dword stores, not kernel G
    dw("dw_c24_s1_stride32", 24, out_extra=8, want=COL_DOT4),
    dw("dw_c24_s2_stride32", 24, stride=2, out_extra=8, want=COL),
    dw("dw_c8_s1_wide_weights", 8, kzp=60, wide=True, want=COL),                          # outside the dot-product flavour's range
    dw("dw_c24_s1_wide_weights", 24, kzp=60, wide=True, want=COL),
    dw("dw_c24_s1_long_segment", 24, size=(14, 7), batch=1, want=COL_DOT4),               # 14 rows: four rows in flight
    dw("dw_c24_wide_long_segment", 24, size=(14, 7), batch=1, kzp=60, wide=True, want=COL),
    dw("dw_c24_dilated_long_segment", 24, size=(26, 7), batch=1, dilation=2, want=COL_DILATED),
    dw("dw_c24_hardswish", 24, table="hardswish", want=COL_DOT4),
    dw("dw_c24_clamp", 24, clamp=(10, 200), want=COL_DOT4),
    dw("dw5_c8_s1", 8, kernel=5, want=COL5),
    dw("dw5_c8_s2", 8, kernel=5, stride=2, want=COL5),
    dw("dw5_c8_hardswish", 8, kernel=5, table="hardswish", want=COL5),
    dw("dw5_c8_clamp", 8, kernel=5, clamp=(10, 200), want=COL5),
    dw("dw5_c24_stride32", 24, kernel=5, out_extra=8, want=COL5),
]


@pytest.mark.parametrize("case", DEPTHWISE, ids=lambda c: c.name)
def test_depthwise(qnnp, case):
    T.hold(qnnp, case)


# ---- one case in each requantization class each table flavour instantiates (tests/test_requant_classes_fused_gpu.py) ----
CLASS_FAMILIES = {
    "pw_staged": dict(code=5, want=PW),
    "pw_direct": dict(goc=20, code=5, want=PW),
    "pw_longk": dict(gic=272, code=9, want=LONGK),
    "pw_gw": dict(gic=32, code=6, want=GW),
    "pw_gwk": dict(gic=272, code=6, want=GWK),
    "dw_s1": dict(gic=1, goc=1, groups=24, kernel=3, family="dwconv_kernel", want=COL_DOT4),
    "dw_s2": dict(gic=1, goc=1, groups=24, kernel=3, stride=2, family="dwconv_kernel", want=COL),
    "dw5": dict(gic=1, goc=1, groups=8, kernel=5, family="dwconv_kernel", want=COL5),
}
CLASSES = [Case(f"class_{fam}_mode{mode}", mode=mode, kzp=127 + (mode & 1), **kw)
           for fam, kw in CLASS_FAMILIES.items() for mode in F.MODES]


@pytest.mark.parametrize("case", CLASSES, ids=lambda c: c.name)
def test_every_requantization_class(qnnp, case):
    T.hold(qnnp, case)


# ---- not folded, still exact -------------------------------------------------------------------------------------------
NOT_FOLDED = [
    Case("dense_3x3_8_to_8_code1", gic=8, goc=8, kernel=3, code=1, want="q8_igemm_mfma_128x32", folded=0),
    Case("fully_connected", gic=20, goc=12, batch=5, fc=True, want=OTHER, folded=0),
    dw("dw_c6_not_kernel_g", 6, want=OTHER, folded=0),
    # 35 channel blocks of one K block: 40 KiB of weights and bias, four workgroups per CU -- and three with the table
    Case("pw_code5_no_room_in_lds", goc=1100, code=5, want=PW, folded=0),
]


@pytest.mark.parametrize("case", NOT_FOLDED, ids=lambda c: c.name)
def test_not_folded_is_the_table_kernel_behind_the_convolution(qnnp, case):
    name, folded = T.hold(qnnp, case)
    assert folded == 0, name


@pytest.mark.parametrize("depthwise", [False, True], ids=["convolution", "depthwise"])
def test_per_channel_operators_take_the_in_place_launch(qnnp, depthwise):
    from _gpu import Guarded, to_device
    if depthwise:
        prob = PC.conv_problem("output_table_pc_dw", 2, (5, 7), (3, 3), (1, 1, 1, 1), groups=24)
    else:
        prob = PC.conv_problem("output_table_pc_conv", 2, (5, 7), gic=24, goc=48)
    table = T._lut.permutation(77)
    rows, ch = prob.acc.shape
    plain = prob.expected(ch)
    want = plain.copy()
    want[...] = table[plain]
    conv = prob.create(qnnp)
    lut = qnnp.create_lut_nc_x8(ch, table, 0)
    d_in, d_out = to_device(prob.inp), Guarded(np.full(plain.size, FILL, np.uint8), 0)
    try:
        assert qnnp.attach_output_table_status(conv, lut) == Status.success
        prob.setup(qnnp, conv, d_in, d_out.view, ch)
        qnnp.run_operator(conv)
        got = d_out.read()
        d_out.assert_intact("per-channel output")
        assert qnnp.operator_table_folded(conv) == 0
        assert_bytes_equal(got, want, f"per-channel {'depthwise' if depthwise else 'convolution'} [{qnnp.operator_kernel(conv)}]")
    finally:
        qnnp.delete_operator(conv)
        qnnp.delete_operator(lut)


# ---- lifecycle ---------------------------------------------------------------------------------------------------------
LIFE = Case("life_pw", code=5, want=PW)
LIFE_UNFOLDED = Case("life_conv3x3", gic=8, goc=8, kernel=3, code=1, want="q8_igemm_mfma_128x32", folded=0)


def _device(p):
    from _gpu import to_device
    return to_device(p.x), to_device(np.full(p.plain().size, FILL, np.uint8))


def test_lifecycle_attach_before_setup_resetup_replace_detach(qnnp):
    from _gpu import from_device, to_device
    p = T.problem(LIFE)
    other = T._lut.permutation(4242)
    conv, lut, lut2 = p.create(qnnp), p.create_table(qnnp), p.create_table(qnnp, other)
    try:
        qnnp.set_option("gemm_kernel", 5)
        assert qnnp.operator_table_folded(conv) == -1
        qnnp.attach_output_table(conv, lut)                 # before the first setup
        qnnp.delete_operator(lut)                           # ... and the table operator deleted before the run
        lut = None
        assert qnnp.operator_table_folded(conv) == 0
        d_in, d_out = _device(p)
        p.setup(qnnp, conv, d_in, d_out)
        qnnp.run_operator(conv)
        assert qnnp.operator_table_folded(conv) == 1 and qnnp.operator_kernel(conv) == PW
        assert_bytes_equal(from_device(d_out), p.expected(), "attached before setup")
        # another shape with the table still in force: one image, pixels of 64 bytes
        half = p.x[:35 * LIFE.gic]
        d_half, d_wide = to_device(half), to_device(np.full(34 * 64 + 48, FILL, np.uint8))
        qnnp.setup_convolution2d_nhwc_q8(conv, 1, 5, 7, d_half, LIFE.gic, d_wide, 64)
        qnnp.run_operator(conv)
        assert_bytes_equal(from_device(d_wide), p.flat(p.table[p.conv[:35]], 64), "set up again at another shape")
        assert qnnp.operator_table_folded(conv) == 1
        # replace
        qnnp.attach_output_table(conv, lut2)
        p.setup(qnnp, conv, d_in, d_out)
        qnnp.run_operator(conv)
        assert_bytes_equal(from_device(d_out), p.expected(other), "table replaced")
        # detach: the plain bytes again
        qnnp.attach_output_table(conv, None)
        assert qnnp.operator_table_folded(conv) == -1
        qnnp.run_operator(conv)
        assert_bytes_equal(from_device(d_out), p.plain(), "table detached")
        qnnp.attach_output_table(conv, None)                # nothing attached: still fine
    finally:
        qnnp.set_option("gemm_kernel", 0)
        for h in (conv, lut, lut2):
            if h is not None:
                qnnp.delete_operator(h)


@pytest.mark.parametrize("case", [LIFE, LIFE_UNFOLDED], ids=["folded", "not_folded"])
def test_host_endpoints_async_mode_and_graph(qnnp, case):
    import torch
    from _gpu import from_device
    p = T.problem(case)
    conv, lut = p.create(qnnp), p.create_table(qnnp)
    try:
        qnnp.set_option(case.family, case.code)
        qnnp.attach_output_table(conv, lut)
        # host endpoints: the staged device output is what the table walks
        host_out = np.full(p.plain().size, FILL, np.uint8)
        p.setup(qnnp, conv, p.x, host_out)
        qnnp.run_operator(conv)
        assert_bytes_equal(host_out, p.expected(), f"{case.name}: host endpoints")
        assert qnnp.operator_table_folded(conv) == case.folded and qnnp.operator_kernel(conv) == case.want
        # async mode
        d_in, d_out = _device(p)
        p.setup(qnnp, conv, d_in, d_out)
        qnnp.set_async(True)
        try:
            qnnp.run_operator(conv)
            qnnp.synchronize()
        finally:
            qnnp.set_async(False)
        assert_bytes_equal(from_device(d_out), p.expected(), f"{case.name}: async mode")
        # one capture, one replay
        d_out.fill_(FILL)
        torch.cuda.synchronize()
        qnnp.graph_begin()
        try:
            qnnp.run_operator(conv)
        finally:
            graph = qnnp.graph_end()
        try:
            assert np.all(from_device(d_out) == FILL), "capturing ran the launch"
            qnnp.graph_launch(graph)
            qnnp.graph_synchronize(graph)
            assert_bytes_equal(from_device(d_out), p.expected(), f"{case.name}: graph replay")
        finally:
            qnnp.graph_destroy(graph)
        assert qnnp.operator_table_folded(conv) == case.folded
    finally:
        qnnp.set_option(case.family, 0)
        qnnp.delete_operator(conv)
        qnnp.delete_operator(lut)


def test_batch_zero(qnnp):
    p = T.problem(LIFE)
    conv, lut = p.create(qnnp), p.create_table(qnnp)
    try:
        qnnp.attach_output_table(conv, lut)
        d_in, d_out = _device(p)
        qnnp.setup_convolution2d_nhwc_q8(conv, 0, 5, 7, d_in, LIFE.gic, d_out, LIFE.out_stride)
        qnnp.run_operator(conv)
        from _gpu import from_device
        assert np.all(from_device(d_out) == FILL)
        assert qnnp.operator_table_folded(conv) == 0
    finally:
        qnnp.delete_operator(conv)
        qnnp.delete_operator(lut)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_status_codes_in_their_order_and_the_combination_refusals(qnnp):
    from _gpu import to_device
    k1 = np.full((1, 16, 1, 1, 32), 120, np.uint8)
    b16 = np.zeros(16, np.int32)
    make_conv = lambda: qnnp.create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 32, 16, 4, 1.0, 2, 1.0, k1, b16, 5, 2.0, 0, 255, 0)
    conv, conv2 = make_conv(), make_conv()
    deconv = qnnp.create_deconvolution2d_nhwc_q8(0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 1, 1, 1, 32, 16, 4, 1.0, 2, 1.0,
                                                 np.full((1, 32, 2, 2, 16), 120, np.uint8), b16, 5, 2.0, 0, 255, 0)
    table = T._lut.permutation(1)
    lut, lut8 = qnnp.create_lut_nc_x8(16, table, 0), qnnp.create_lut_nc_x8(8, table, 0)
    add = qnnp.create_add_nc_q8(16, 1, 1.0, 5, 1.0, 6, 2.0, 0, 255, 0)
    buf, out, res = (to_device(np.zeros(1 << 12, np.uint8)) for _ in range(3))
    made = []
    try:
        attach = qnnp.attach_output_table_status
        assert attach(None, lut) == Status.invalid_parameter
        assert attach(None, None) == Status.invalid_parameter
        assert attach(lut, lut) == Status.invalid_parameter            # not a convolution
        assert attach(add, lut) == Status.invalid_parameter
        assert attach(deconv, lut) == Status.invalid_parameter         # a deconvolution
        assert attach(conv, add) == Status.invalid_parameter           # not a table operator
        assert attach(conv, conv2) == Status.invalid_parameter
        assert attach(conv, lut8) == Status.invalid_parameter          # channel mismatch
        assert qnnp.operator_table_folded(conv) == -1
        # inside a graph capture: attach, replace and detach are refused, and the state stays
        assert attach(conv, lut) == Status.success
        qnnp.graph_begin()
        try:
            assert attach(conv, lut) == Status.invalid_parameter
            assert attach(conv, None) == Status.invalid_parameter
            assert attach(conv2, lut) == Status.invalid_parameter
        finally:
            qnnp.graph_destroy(qnnp.graph_end())
        assert qnnp.operator_table_folded(conv) == 0 and qnnp.operator_table_folded(conv2) == -1
        # a residual add on the convolution: unsupported, in both orders
        qnnp.setup_convolution2d_nhwc_q8(conv2, 1, 8, 8, buf, 32, out, 16)
        assert qnnp.attach_residual_add_status(conv2, add, res, 16) == Status.success
        assert attach(conv2, lut8) == Status.invalid_parameter         # the earlier check still answers first
        assert attach(conv2, lut) == Status.unsupported_parameter
        assert qnnp.operator_table_folded(conv2) == -1 and qnnp.operator_residual_folded(conv2) == 0
        assert attach(conv2, None) == Status.success                   # nothing to detach: nothing refused
        qnnp.setup_convolution2d_nhwc_q8(conv, 1, 8, 8, buf, 32, out, 16)
        assert qnnp.attach_residual_add_status(conv, add, res, 16) == Status.unsupported_parameter
        assert qnnp.operator_residual_folded(conv) == -1 and qnnp.operator_table_folded(conv) == 0
        # fused operators borrow their members' parameters: a member with a table is refused
        dwk = np.full((16, 1, 3, 3, 1), 120, np.uint8)
        dwc = qnnp.create_convolution2d_nhwc_q8(1, 1, 1, 1, 3, 3, 1, 1, 1, 1, 16, 1, 1, 4, 1.0, 2, 1.0, dwk, b16, 5, 2.0, 0, 255, 0)
        project = qnnp.create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 16, 16, 4, 1.0, 2, 1.0,
                                                    np.full((1, 16, 1, 1, 16), 120, np.uint8), b16, 5, 2.0, 0, 255, 0)
        made += [dwc, project]
        for member in (conv, dwc, project):
            if member is not conv:
                assert attach(member, lut) == Status.success
            st, fused = qnnp.create_fused_block_status(conv, dwc, project, None)
            assert st == Status.unsupported_parameter and not fused, (st, fused)
            assert attach(member, None) == Status.success
        st, fused = qnnp.create_fused_block_status(conv, dwc, project, None)
        assert st == Status.success                                    # ... and without tables the same block is accepted
        made.append(fused)
        pool = qnnp.create_global_average_pooling_nwc_q8(16, 4, 1.0, 5, 1.0, 0, 255, 0)
        fc1 = qnnp.create_fully_connected_nc_q8(16, 8, 4, 1.0, 2, 1.0, np.full((8, 16), 120, np.uint8), np.zeros(8, np.int32), 5, 2.0, 0, 255, 0)
        fc2 = qnnp.create_fully_connected_nc_q8(8, 16, 4, 1.0, 2, 1.0, np.full((16, 8), 120, np.uint8), b16, 5, 2.0, 0, 255, 0)
        mul = qnnp.create_multiply_nc_q8(16, 4, 1.0, 0, 1.0 / 256, 5, 1.0, 0, 255, 0)
        made += [pool, fc1, fc2, mul]
        for member, member_lut in ((fc1, lut8), (fc2, lut)):
            assert attach(member, member_lut) == Status.success
            st, se = qnnp.create_squeeze_excite_status(pool, fc1, fc2, lut, mul)
            assert st == Status.unsupported_parameter and not se, (st, se)
            assert attach(member, None) == Status.success
        st, se = qnnp.create_squeeze_excite_status(pool, fc1, fc2, lut, mul)
        assert st == Status.success
        made.append(se)
    finally:
        for h in made[::-1] + [conv, conv2, deconv, lut, lut8, add]:
            qnnp.delete_operator(h)
