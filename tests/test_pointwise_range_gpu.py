"""GPU tier: add, global average pooling and windowed average pooling over the whole accepted range of scale ratios.

The parameter sets are those of tests/_pointwise.py (add_range_sets, gap_range_cases) and tests/_pooling.py
(range_cases): both ends of the accepted ratios, both sides of the add's 2^-10 seam, the zero-point corners and tight
clamps. tests/test_pointwise_range_host.py holds their expectations -- the scalar oracle and the numpy pooling model --
to real arithmetic within half a step plus the float32 error of the scales; here every kernel must give those bytes.

 1. add: every set on q8_vadd_flat (dense, 16-byte aligned) and on q8_vadd_strided (strides 257 / 259 / 261, the fill
    between the rows included), all 65536 byte pairs each, a and b uploaded once;
 2. global average pooling: every case on q8_gavgpool_x4 and, with 255 channels and with an input stride of 257, on
    q8_gavgpool_x1;
 3. windowed average pooling: every case on each vector width, reached through the channel count, the input stride
    and the base alignment as in tests/test_gpu_pooling.py::test_kernel_path_follows_alignment;
 4. the add folded into a convolution (tests/test_gpu_residual.py's driver) below, at and above the seam, on each
    kernel that carries it and on the fallback, against the oracle and the two-operator sequence.

Run time on an MI355X: the whole file takes about 3 s; the slowest id is the first add id, 0.3 s with the upload of the
two input tensors, and no other id takes more than 0.1 s.
"""
from dataclasses import replace

import numpy as np
import pytest

import _pointwise as pw
import _pooling as pl
from _gpu import from_device, to_device
from test_gpu_residual import ADD_Q, _run_case

pytestmark = pytest.mark.gpu

SETS = pw.add_range_sets()
STRIDES = (257, 259, 261)      # a, b, sum: no two alike, none a multiple of 4


def _strided(rows: np.ndarray, stride: int, fill: int) -> np.ndarray:
    """[256][256] laid out with `stride` bytes between rows, `fill` in between"""
    flat = np.full(255 * stride + 256, fill, dtype=np.uint8)
    idx = np.arange(256, dtype=np.int64)[:, None] * stride + np.arange(256)[None, :]
    flat[idx] = rows
    return flat


@pytest.fixture(scope="module")
def add_tensors():
    a, b = pw.add_range_inputs()
    return {"flat": (to_device(a), to_device(b), to_device(np.full(65536, pw.FILL, np.uint8)), (256, 256, 256)),
            "strided": (to_device(_strided(a, STRIDES[0], 0x5A)), to_device(_strided(b, STRIDES[1], 0x3C)),
                        to_device(np.full(255 * STRIDES[2] + 256, pw.FILL, np.uint8)), STRIDES)}


def _run_add(qnnp, s, tensors, kernel):
    d_a, d_b, d_y, (sa, sb, sy) = tensors[kernel]
    want = pw.add_range_expected(s)
    if kernel == "strided":
        want = _strided(want, sy, pw.FILL)
    op = qnnp.create_add_nc_q8(256, s.a_zp, s.a_scale, s.b_zp, s.b_scale, s.y_zp, s.y_scale, s.qmin, s.qmax, 0)
    try:
        d_y.fill_(pw.FILL)
        qnnp.setup_add_nc_q8(op, 256, d_a, sa, d_b, sb, d_y, sy)
        qnnp.run_operator(op)
        kname = qnnp.operator_kernel(op)
        got = from_device(d_y)
    finally:
        qnnp.delete_operator(op)
    assert kname == f"q8_vadd_{kernel}", (s.name, kname)
    return np.flatnonzero(got != want.reshape(-1))


# ---- 1. add ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", pw.ADD_RANGE_BANDS)
@pytest.mark.parametrize("kernel", ["flat", "strided"])
def test_add_over_the_whole_ratio_range(qnnp, add_tensors, kernel, band):
    sets = [s for s in SETS if s.band == band]
    assert sets
    bad = []
    for s in sets:
        diff = _run_add(qnnp, s, add_tensors, kernel)
        if diff.size:
            bad.append((s.name, int(diff.size), diff[:4].tolist()))
    assert not bad, (len(bad), bad[:8])


def test_both_add_kernels_are_reached(qnnp, add_tensors):
    s = next(s for s in SETS if s.name == "r8_r8")      # both ratios 1: the sum sweeps the whole output range
    for kernel in ("flat", "strided"):                  # _run_add asserts the kernel's name
        assert _run_add(qnnp, s, add_tensors, kernel).size == 0
    assert np.unique(pw.add_range_expected(s)).size == 256      # no constant could pass


# ---- 2. global average pooling -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,channels,in_stride,kernel", [
    ("dense_c256", 256, 0, "q8_gavgpool_x4"), ("c255", 255, 0, "q8_gavgpool_x1"), ("stride257", 256, 257, "q8_gavgpool_x1")])
def test_global_average_pooling_over_the_whole_ratio_range(qnnp, layout, channels, in_stride, kernel):
    cases = pw.gap_range_cases(channels, in_stride)
    inputs = {}
    for w in pw.GAP_RANGE_WIDTHS:
        flat = pw.gap_range_input(next(c for c in cases if c.width == w), pw.gap_range_pixels(w, channels))
        inputs[w] = (flat, to_device(flat))
    d_out = to_device(np.full(4 * channels, pw.FILL, np.uint8))
    bad = []
    for case in cases:
        flat, d_in = inputs[case.width]
        si, so = case.strides
        want = pw.gap_expected(case, flat)
        op = qnnp.create_global_average_pooling_nwc_q8(channels, case.in_zp, case.in_scale, case.out_zp, case.out_scale,
                                                       case.qmin, case.qmax, 0)
        try:
            d_out.fill_(pw.FILL)
            qnnp.setup_global_average_pooling_nwc_q8(op, case.batch, case.width, d_in, si, d_out, so)
            qnnp.run_operator(op)
            assert qnnp.operator_kernel(op) == kernel, (case.name, qnnp.operator_kernel(op))
            got = from_device(d_out)
        finally:
            qnnp.delete_operator(op)
        diff = np.flatnonzero(got != want)
        if diff.size:
            bad.append((case.name, int(diff.size), diff[:4].tolist()))
    assert not bad, (len(bad), bad[:8])


# ---- 3. windowed average pooling ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,in_stride,misalign,vec", [
    (16, 0, 0, 16), (16, 20, 0, 4), (16, 0, 4, 4), (16, 19, 0, 1), (16, 0, 1, 1), (19, 0, 0, 1)])
def test_average_pooling_over_the_whole_ratio_range(qnnp, channels, in_stride, misalign, vec):
    cases = [replace(c, name=f"{c.name}_s{in_stride}_m{misalign}", in_stride=in_stride, misalign_in=misalign)
             for c in pl.range_cases() if c.channels == channels]
    assert len(cases) == 150
    bad = []
    for case in cases:
        x = pl.range_input(case)
        want = pl.expected(case, x)[0]
        got, kname = pl.run(qnnp, case, x, to_device=to_device, from_device=from_device)
        assert kname == f"q8_avgpool_x{vec}", (case.name, kname)
        diff = np.flatnonzero(got[0] != want)
        if diff.size:
            bad.append((case.name, int(diff.size), diff[:4].tolist()))
    assert not bad, (len(bad), bad[:8])


# ---- 4. the add folded into a convolution ------------------------------------------------------------------------------
TOP = pw.f32_below(2.0 ** 8)
FOLDED_RATIOS = [("both_below_seam", 2.0 ** -12, 2.0 ** -13), ("at_seam", 2.0 ** -10, 2.0 ** -14), ("top_and_bottom", TOP, 2.0 ** -14),
                 ("mid", 0.75, 1.25)]
# the smallest shape of each carrying kernel in tests/test_gpu_residual.py::test_each_carrying_kernel, and the fallback
FOLDED_SHAPES = [(5, 3, 33, 40, 24, "q8_pw_stream_mfma", 1), (9, 3, 14, 576, 96, "q8_pw_stream_longk_mfma", 1),
                 (6, 3, 7, 960, 160, "q8_pw_stream_gwk_mfma", 1), (6, 16, 7, 192, 48, "q8_pw_stream_gw_mfma", 1),
                 (1, 1, 9, 24, 40, "", 0)]


@pytest.mark.parametrize("variant,batch,hw,cin,cout,want,folds", FOLDED_SHAPES)
@pytest.mark.parametrize("tag,ra,rb", FOLDED_RATIOS)
def test_folded_add_over_the_ratio_range(qnnp, tag, ra, rb, variant, batch, hw, cin, cout, want, folds):
    """a = the residual at ratio ra, b = the convolution's output at ratio rb, sum scale 1; _run_case compares with the
    oracle and with the two-operator sequence"""
    add_q = dict(ADD_Q, a_scale=ra, b_scale=rb, y_scale=1.0)
    kernel_name, folded = _run_case(qnnp, batch, hw, cin, cout, variant=variant, seed=variant, add_q=add_q)
    assert kernel_name.startswith(want), kernel_name
    assert folded == folds, (kernel_name, folded)
