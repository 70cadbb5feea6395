"""CPU tier: add, global average pooling and windowed average pooling held to REAL arithmetic over the whole accepted
range of scale ratios.

Every byte-level check of these operators compares the kernels with the scalar oracle (oracle/oracle_q8.c) or with the
numpy model of tests/_pooling.py, which restate the integer algorithm: a defect of the algorithm itself would be
reproduced by the expectation. Here the expectations themselves are checked against float64 models
(tests/_pointwise.py add_real / gap_real, tests/_pooling.py avg_real) on parameter sets at the edges of the accepted
ratios, with tolerances that are derived next to their constants, and every output is asserted, clamped or not.

This found a defect: where both add ratios are below 2^-10 the reference's parameter builder shifts 32-bit values by
32 ... 35 and the result was garbage (the oracle returned only {0, 133, 255} for a sum that is within 0.498 of 133
everywhere). The product's builder (qnnp_compute_add_params, requantization.h) and the oracle now answer
clamp(sum zero point) there, the correctly rounded sum, and are bit-identical to the reference's formulas elsewhere.

 1. add: the oracle against the real sum, on all 65536 byte pairs of every set;
 2. add: the product's parameter builder (through qnnp_debug_add_params) with add_quantize emulated in numpy, against the
    oracle byte for byte on every set, and field by field against the reference's formulas from the seam up;
 3. add below the seam: the expectation is the constant clamp(sum zero point);
 4. global average pooling: the oracle against the real mean;
 5. windowed average pooling: the numpy model against the real mean.
The host code itself runs over the same range under the sanitizers in tests/host_asan_test.c
(tests/test_host_sanitizers.py).

Largest distance from the real value seen (each bound is derived, these are records):
    add, larger ratio >= 2^-10      0.5000153   (bound 0.5156; 355 sets)
    add, larger ratio <  2^-10      0.4980468   (bound 0.5156; 59 sets; up to 255 before the fix, all 59 failing)
    global average pooling          0.5000000   (bound 0.5078)
    windowed average pooling        0.5000000   (bound 0.5078)
"""
import ctypes

import numpy as np
import pytest

import _pointwise as pw
import _pooling as pl

SETS = pw.add_range_sets()
BANDS = {band: [s for s in SETS if s.band == band] for band in pw.ADD_RANGE_BANDS}


def test_the_lists_are_what_they_claim():
    assert len(pw.ADD_RANGE_RATIOS) == 13 and len(set(pw.ADD_RANGE_RATIOS)) == 13
    assert min(pw.ADD_RANGE_RATIOS) == 2.0 ** -14 and max(pw.ADD_RANGE_RATIOS) == pw.f32_below(256.0) < 256.0
    assert pw.f32_below(pw.ADD_SEAM) in pw.ADD_RANGE_RATIOS and pw.ADD_SEAM in pw.ADD_RANGE_RATIOS
    assert len({s.name for s in SETS}) == len(SETS) == 169 + 15 * 16 + 5
    assert sum(len(v) for v in BANDS.values()) == len(SETS) and all(BANDS.values())
    assert all(s.below_seam == (s.band == "below_seam") for s in SETS)
    for s in SETS:                                          # create accepts every set
        assert all(2.0 ** -14 <= float(r) < 2.0 ** 8 for r in s.ratios) and s.qmin < s.qmax, s
    a, b = pw.add_range_inputs()
    assert np.unique(a.astype(np.uint32) * 256 + b).size == 65536
    assert len(pw.gap_range_cases()) == 5 * 5 * 5 * 2 and len(pl.range_cases()) == 3 * 2 * 5 * 5 * 2
    assert pw.ADD_TOL < 0.52 and pw.POOL_TOL < 0.51 and pl.RANGE_TOL == pw.POOL_TOL


# ---- 1. add: the oracle against the real sum -------------------------------------------------------------------------
@pytest.mark.parametrize("band", pw.ADD_RANGE_BANDS)
def test_add_oracle_is_within_rounding_of_the_real_sum(band):
    a, b = pw.add_range_inputs()
    worst, bad = 0.0, []
    for s in BANDS[band]:
        d = pw.worst_distance(pw.add_range_expected(s), pw.add_real(s, a, b), s.qmin, s.qmax)
        worst = max(worst, d)
        if not d <= pw.ADD_TOL:
            bad.append((s.name, d))
    print(f"add oracle vs real, {band}: {len(BANDS[band])} sets, largest distance {worst:.7f} (bound {pw.ADD_TOL:.7f})")
    assert not bad, (len(bad), bad[:8])


# ---- 2. add: the product's parameter builder -------------------------------------------------------------------------
class AddParams(ctypes.Structure):
    """struct qnnp_hip_add_params (qnnpack_amd/csrc/hip/qnnp_hip.h)"""
    _fields_ = [("a_multiplier", ctypes.c_uint32), ("b_multiplier", ctypes.c_uint32), ("zero_point_product", ctypes.c_int32),
                ("shift", ctypes.c_uint32), ("remainder_mask", ctypes.c_int32), ("remainder_threshold", ctypes.c_int32),
                ("y_zero_point", ctypes.c_int32), ("y_min", ctypes.c_int32), ("y_max", ctypes.c_int32)]


@pytest.fixture(scope="module")
def add_params(debug_hooks):
    fn = debug_hooks.lib.qnnp_debug_add_params
    fn.restype = None
    fn.argtypes = [ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_float, ctypes.c_float, ctypes.c_uint8,
                   ctypes.c_uint8, ctypes.POINTER(AddParams)]

    def build(s):
        p = AddParams()
        ra, rb = s.ratios
        fn(s.a_zp, s.b_zp, s.y_zp, ra, rb, s.qmin, s.qmax, ctypes.byref(p))
        return p
    return build


def _add_quantize(p, a, b):
    """add_quantize of hip/add_math.hip.h on uint8 arrays: 32-bit wrap-around, 5-bit shift count, as the device has"""
    a32, b32 = a.astype(np.uint32), b.astype(np.uint32)
    with np.errstate(over="ignore"):
        acc = (np.uint32(p.zero_point_product & 0xFFFFFFFF) + a32 * np.uint32(p.a_multiplier)
               + b32 * np.uint32(p.b_multiplier)).astype(np.uint32).view(np.int32)
    rem = (acc & np.int32(p.remainder_mask)) - (acc < 0).astype(np.int32)
    acc = (acc >> np.int32(p.shift & 31)) + (rem > np.int32(p.remainder_threshold)).astype(np.int32)
    y = acc + np.int32(p.y_zero_point)
    y = np.where(y >= p.y_max, p.y_max, y)
    y = np.where(y <= p.y_min, p.y_min, y)
    return y.astype(np.uint8)


@pytest.mark.parametrize("band", pw.ADD_RANGE_BANDS)
def test_add_parameter_builder_gives_the_oracle_bytes(add_params, band):
    a, b = pw.add_range_inputs()
    bad = []
    for s in BANDS[band]:
        p = add_params(s)
        if not (14 <= p.shift <= 31 and p.remainder_mask == (1 << p.shift) - 1
                and p.remainder_threshold == p.remainder_mask >> 1):
            bad.append((s.name, "shift", p.shift))
        elif not np.array_equal(_add_quantize(p, a, b), pw.add_range_expected(s)):
            bad.append((s.name, "bytes"))
    assert not bad, (len(bad), bad[:8])


def test_add_parameters_are_the_references_from_the_seam_up(add_params):
    """qnnp_compute_add_quantization_params, scalar member (reference src/qnnpack/requantization.h:327-360, :400-413),
    restated with exact integer arithmetic: every field, for every set whose larger ratio is 2^-10 or more"""
    checked = 0
    for s in SETS:
        if s.below_seam:
            continue
        ra, rb = (float(v) for v in s.ratios)
        shift = 21 - (int(np.float32(max(ra, rb)).view(np.uint32)) >> 23) + 127
        ma, mb = round(ra * 2.0 ** shift), round(rb * 2.0 ** shift)        # exact products; round() is half to even, as lrintf
        assert 14 <= shift <= 31 and 2 ** 21 <= max(ma, mb) <= 2 ** 22     # 2^22: a 24-bit mantissa of all ones, rounded
        zpp = -(ma * s.a_zp + mb * s.b_zp)
        zpp = (zpp + 2 ** 31) % 2 ** 32 - 2 ** 31
        p = add_params(s)
        got = (p.a_multiplier, p.b_multiplier, p.zero_point_product, p.shift, p.remainder_mask, p.remainder_threshold,
               p.y_zero_point, p.y_min, p.y_max)
        assert got == (ma, mb, zpp, shift, (1 << shift) - 1, ((1 << shift) - 1) >> 1, s.y_zp, s.qmin, s.qmax), s.name
        checked += 1
    assert checked == len(SETS) - len(BANDS["below_seam"])


# ---- 3. below the seam -----------------------------------------------------------------------------------------------
def test_below_the_seam_every_output_is_the_clamped_zero_point(add_params):
    assert len(BANDS["below_seam"]) == 9 + 3 * 16 + 2
    for s in BANDS["below_seam"]:
        want = min(max(s.y_zp, s.qmin), s.qmax)
        y = pw.add_range_expected(s)
        assert y.min() == y.max() == want, (s.name, int(y.min()), int(y.max()), want)
        p = add_params(s)
        assert (p.a_multiplier, p.b_multiplier, p.zero_point_product) == (0, 0, 0) and p.shift <= 31, s.name


# ---- 4. global average pooling: the oracle against the real mean ---------------------------------------------------------
def test_global_average_pooling_oracle_is_within_rounding_of_the_real_mean():
    worst, bad = 0.0, []
    pixels = {w: pw.gap_range_pixels(w) for w in pw.GAP_RANGE_WIDTHS}
    for case in pw.gap_range_cases():
        px = pixels[case.width]
        got = pw.gap_expected(case, pw.gap_range_input(case, px)).reshape(case.batch, case.channels)
        d = pw.worst_distance(got, pw.gap_real(case, px), case.qmin, case.qmax)
        worst = max(worst, d)
        if not d <= pw.POOL_TOL:
            bad.append((case.name, d))
    print(f"global average pooling oracle vs real: largest distance {worst:.7f} (bound {pw.POOL_TOL:.7f})")
    assert not bad, (len(bad), bad[:8])


def test_global_average_pooling_oracle_reads_strided_and_narrow_tensors_alike():
    """the layouts the GPU tier uses to reach the byte kernel give the same bytes as the dense 256-channel tensor"""
    for w in (1, 7, 300):
        px = pw.gap_range_pixels(w)
        dense, strided, narrow = (pw.gap_range_cases(*args)[::7] for args in ((256, 0), (256, 257), (255, 0)))
        for d, s, n in zip(dense, strided, narrow):
            if d.width != w:
                continue
            want = pw.gap_expected(d, pw.gap_range_input(d, px)).reshape(4, 256)
            assert np.array_equal(pw.gap_expected(s, pw.gap_range_input(s, px)).reshape(4, 256), want), s.name
            assert np.array_equal(pw.gap_expected(n, pw.gap_range_input(n, px[:, :, :255])).reshape(4, 255), want[:, :255]), n.name


# ---- 5. windowed average pooling: the numpy model against the real mean -----------------------------------------------------
def test_average_pooling_model_is_within_rounding_of_the_real_mean():
    worst, bad = 0.0, []
    for case in pl.range_cases():
        x = pl.range_input(case)
        oh, ow = case.output_size(case.input_height, case.input_width)
        got = pl.avg_pool(case, x, case.batch, case.input_height, case.input_width)
        real = pl.avg_real(case, x)
        assert got.shape == real.shape == (2, oh, ow, case.channels)
        d = pw.worst_distance(got, real, case.qmin, case.qmax)
        worst = max(worst, d)
        if not d <= pl.RANGE_TOL:
            bad.append((case.name, d))
    print(f"average pooling model vs real: largest distance {worst:.7f} (bound {pl.RANGE_TOL:.7f})")
    assert not bad, (len(bad), bad[:8])
