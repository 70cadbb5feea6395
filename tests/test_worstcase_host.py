"""CPU tier of the worst-case operands (tests/_worstcase.py): the builders hit the accumulator bound they claim, the
reference's bytes are not a saturated image (the same conditions tests/test_gpu_worstcase.py asserts before it touches
the device), and the lane requantization forms hold with row terms DERIVED from extreme operands, unfiltered.

Shares of the oracle's bytes strictly inside (0, 255), as measured with these builders over all eight corners
(test_reference_bytes_are_not_a_saturated_image prints them):
  regime B, zero point 127, lowest scale class to highest (0.3 is the low end; 100 % where the scale sends every accumulator
      of a cancelled window next to the zero point):  fc_k512_n512 11.5-100 %, pw_c64_n64 12.9-100 %, c33_64_64 9.5-100 %,
      c33_64_256 11.8-100 %, dc_4x4_s2 17.4-100 %, dw3_c32 17.6-100 %, dw5_c64 8.5-100 %;
  regime A at 1.5 * 2^-20, sign-matched zero point:  fc 39-41 %, pw 26-37 %, c33 44-46 %, dc 46-47 %, dw3_c32 28-36 %,
      dw5_c64 39-48 % (with the spread bias of _worstcase._build_depthwise; 0 % at the centred 3x3 corners without it).
  c3_7x7_s2 (GPU tier only): regime B 8.7-100 % with bands of eight rows (_worstcase.band_rows; 4.5 % at 0.3 with four)."""
import ctypes

import numpy as np
import pytest

import _worstcase as wc
from _cases import FcCase
from oracle import o1
from test_gpu_kernel_contract import DW_CASES, GEMM_CASES

_BY_NAME = {c.name: c for c in GEMM_CASES + DW_CASES}
CASES = [_BY_NAME[n] for n in ("fc_k512_n512", "pw_c64_n64", "c33_64_64", "c33_64_256", "dw3_c32", "dw5_c64", "dc_4x4_s2")]


@pytest.fixture(scope="module")
def accumulator_bits(debug_hooks):
    fn = debug_hooks.lib.qnnp_debug_accumulator_bits
    fn.restype = ctypes.c_uint32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t]
    return lambda bias, k: fn(np.ascontiguousarray(bias, np.int32).ctypes.data, bias.size, k)


def test_scales_have_the_shifts_they_are_listed_for():
    for i, (nominal, shift) in enumerate(wc.SCALES):
        kernel_scale, output_scale, scale = wc.scale_arguments(i)
        assert np.float32(np.float32(1.0) * np.float32(kernel_scale) / np.float32(output_scale)) == scale
        assert o1.q31_params(scale, 0, 0, 255).shift == shift
        assert abs(float(scale) / nominal - 1) < 1e-6
    assert wc.scale_arguments(0)[2] == np.float32(float.fromhex("0x1.FFFFFEp-1"))
    assert [s for _, s in wc.SCALES] == [0, 1, 7, 4, 8, 19, 20, 21]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_regime_a_sits_at_the_bound(accumulator_bits, case):
    """classified b = 30 for B = 2^30 and b = 31 for B = 2^30 + 1; at the outer corners the oracle's largest accumulator
    is exactly B - 1; over the four signs both saturations occur"""
    K = wc.reduction_length(case)
    seen = set()
    for corner in wc.CORNERS:
        for regime, B in wc.BOUNDS.items():
            ops = wc.operands(case, corner, regime)
            assert accumulator_bits(ops.bias, K) == (30 if B == 2 ** 30 else 31), (case.name, corner, regime)
            top = int(np.abs(ops.acc.astype(np.int64)).max())
            if corner in wc.OUTER_CORNERS:
                if isinstance(case, wc.DeconvCase):
                    # the bound counts all kh * kw taps; an output of a stride-2 4x4 deconvolution sums four of them
                    assert top == B - 1 - 65025 * (K - 4 * case.gic), (case.name, corner, regime, top)
                else:
                    assert top == B - 1, (case.name, corner, regime, top)
            assert top < B
            for run in wc.runs(regime, ops.product):
                out = o1.requantize_rows(ops.acc, run.scale, run.zero_point, run.qmin, run.qmax)
                seen |= {v for v in (0, 1, 254, 255) if (out == v).any()}
    assert {0, 255} <= seen, (case.name, seen)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_bytes_are_not_a_saturated_image(case, capsys):
    shares = {}
    for corner in wc.CORNERS:
        for regime in wc.regimes(case):
            ops = wc.operands(case, corner, regime)
            for run in wc.runs(regime, ops.product):
                share, count = wc.assert_not_vacuous(ops, regime, run)
                if regime == "B" or (run.index == wc.SCALE_AT_BOUND and regime == "A30"):
                    shares.setdefault((regime[0], run.index), []).append(share)
    with capsys.disabled():
        print(f"\n  {case.name}: " + ", ".join(f"{r}{i} {min(v):.3f}-{max(v):.3f}" for (r, i), v in sorted(shares.items())))


def test_regime_b_cancels_to_one_centred_byte():
    """where a full window meets a full channel the accumulator is r plus one centred byte: |acc| <= 60 + 128"""
    for case in CASES:
        for corner in wc.CORNERS:
            ops = wc.operands(case, corner, "B")
            small = np.abs(ops.acc) <= 188 + (255 if wc.is_depthwise(case) else 0)
            assert small.mean() > (0.02 if wc.is_depthwise(case) else 0.05), (case.name, corner, float(small.mean()))


def test_weight_range_operands_reach_the_class_ends():
    for name in ("dw3_c32", "dw5_c32"):
        reached = set()
        for corner in wc.CORNERS:
            ops = wc.weight_range_operands(_BY_NAME[name], corner)
            reached |= set((ops.kernel.astype(np.int32) - corner[1]).reshape(-1).tolist())
            inside = np.abs(ops.acc) <= 60
            assert inside.mean() > 0.2, (name, corner)
        assert reached == {-255, -128, -127, 127, 128, 255}


EDGE = {k: FcCase(f"fc_edge_k{k}", 64, k, 64) for k in (16512, 16576)}


def test_reduction_length_crosses_the_classification_edge(accumulator_bits):
    for k, bits in ((16512, 30), (16576, 31)):
        for corner in wc.OUTER_CORNERS:
            ops = wc.operands(EDGE[k], corner, "E")
            assert accumulator_bits(ops.bias, k) == bits
            top = int(np.abs(ops.acc.astype(np.int64)).max())
            assert top >= 65025 * k - 10000 and (k != 16512 or top > 2 ** 30 - 2 ** 17)


def test_lane_forms_with_derived_row_terms(debug_hooks):
    """qnnp_debug_requant_lane at bits = 30 on a K = 16512 reduction of extreme operands: the row term is
    (128 - kzp) * sum(a ^ 0x80) and a = n - rowterm what the matrix cores deliver from bias2; a fits
    int32, the bytes are the oracle's and the kind is dispatch's: 1 at shift 0 (0 for the one multiplier whose zero point
    cannot be folded), 2 for shifts 1..20, 0 above."""
    fn = debug_hooks.lib.qnnp_debug_requant_lane
    fn.restype = None
    fn.argtypes = [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint8, ctypes.c_uint8,
                   ctypes.c_uint8, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    case = EDGE[16512]
    kinds = set()
    for corner in wc.OUTER_CORNERS + [(0, 127), (255, 128)]:
        ops = wc.operands(case, corner, "E")
        n = ops.acc.astype(np.int64)
        centred = (ops.input.reshape(case.batch, case.input_channels) ^ 0x80).view(np.int8).astype(np.int64)
        rowterm = np.broadcast_to(((128 - corner[1]) * centred.sum(axis=1))[:, None], n.shape)
        a = n - rowterm
        assert np.abs(rowterm).max() <= 2 ** 30 and a.min() >= -2 ** 31 and a.max() < 2 ** 31, (corner, int(np.abs(rowterm).max()))
        # a is bias2 + the dot product of the centred images
        w_c = (ops.kernel ^ 0x80).view(np.int8).astype(np.int64)
        bias2 = ops.bias + (128 - corner[0]) * w_c.sum(axis=1) + case.input_channels * (128 - corner[0]) * (128 - corner[1])
        assert np.array_equal(a, centred @ w_c.T + bias2[None, :]), corner
        acc32 = np.ascontiguousarray(ops.acc.reshape(-1))
        rt32 = np.ascontiguousarray(rowterm.astype(np.int32).reshape(-1))
        extra = [wc.Run(-1, 1.0, 1.0, np.float32(0.75), zp, 0, 255) for zp in (0, 127, 255)]      # so that kind 1 occurs
        for run in wc.runs("E", ops.product) + [r._replace(zero_point=127) for r in wc.runs("E", ops.product)] + extra:
            out = np.empty(acc32.size, np.uint8)
            kind = ctypes.c_int(-1)
            fn(acc32.size, acc32.ctypes.data, rt32.ctypes.data, run.scale, run.zero_point, run.qmin, run.qmax, 30,
               out.ctypes.data, ctypes.byref(kind))
            p = o1.q31_params(run.scale, run.zero_point, run.qmin, run.qmax)
            want = (1 if p.multiplier <= 0x7FFFFF00 else 0) if p.shift == 0 else (2 if p.shift <= 20 else 0)
            assert kind.value == want, (corner, float(run.scale), kind.value, want)
            kinds.add(kind.value)
            exp = o1.q31_requantize(acc32, run.scale, run.zero_point, run.qmin, run.qmax)
            bad = np.flatnonzero(out != exp)
            assert bad.size == 0, (corner, float(run.scale), run.zero_point, int(acc32[bad[0]]), int(rt32[bad[0]]), int(out[bad[0]]), int(exp[bad[0]]))
    assert kinds == {0, 1, 2}
