"""GPU tier: every forced kernel with worst-case operands at the accumulator bound (tests/_worstcase.py).

The other device tests draw uniform bytes (|accumulator| < 2^22 or so) or reach large accumulators with a huge bias against
all-zero-point inputs, which classifies the operator as unbounded. Here real products carry the accumulator to the bound
max|bias| + 65025 * K < 2^30 from which create time picks the bounded, offset, lane and packed-tail requantization forms
(DESIGN section 2), one step past it (b = 31: the unbounded sequences must answer), and through huge product sums that
the bias cancels, so that bias2, the row sums over raw bytes, the centred images, the depthwise fold and the int8 splits
of the depthwise weights are as large as they get while the bytes stay inside the clamp.

Per (family, code, case) -- code 0 and every code of ACCEPTS, with at most one case of each kind it lists -- eight zero-point
corners x regimes (A at 2^30, A at 2^30 + 1, B) x eight scales: operator created, set up, run and deleted, byte for byte
against the scalar oracle, kernel name in the code's set. A forced code may refuse a corner (unsupported_parameter);
code 0 never refuses; every id completes each regime at least once.

Corners taken (izp/kzp; the eight of _worstcase.CORNERS), as recorded on an MI355X -- every id completed all three
regimes, b = 30 and b = 31 included:
  gemm_kernel 0, 1, 2, 3, 5, 6, 7, 8, 9, 12, 13, 14, 15, 22, 27, 29, 30, 31 and dwconv_kernel 0, 1, 2, 3, 4, 5, 8, 9: all eight
      (dwconv_kernel 6: all eight on 3x3 -- the int16 column kernel at the outer corners, dot4 at the centred ones);
  gemm_kernel 20, 23, 24, 25, 26, 32, dwconv_kernel 7 and dwconv_kernel 6 on 5x5: the centred corners 0/127 0/128 255/127 255/128
      (a centred image or an int8 weight class needs kernel zero point 127 / 128);
  gemm_kernel 28: all but 0/128 and 255/128 (kernel zero point 128 has no row term: that operator is gemm_kernel 23's).
  Classification edge (64 x 64, K = 16512 / 16576, outer corners): codes 0, 1, 2, 6, 13, 29 ran both lengths; the others
      refuse the shape or the outer zero points.
  Weight-range classes: as above; dwconv_kernel 3, 4, 5, 7, 8 are 3x3 kernels and refuse dw5_c32.
Slowest id: fc_k512_n512-gemm0, 1.05 s (c33_64_256-gemm0 1.02 s; every other id below 0.7 s); the whole file 16 s."""
import collections

import numpy as np
import pytest

import _worstcase as wc
from _cases import DeconvCase, FcCase
from _gpu import from_device, to_device
from _runner import FILL, assert_bytes_equal
from qnnpack_amd import QnnpackError, Status
from test_gpu_kernel_contract import ACCEPTS, DECONV_CODES, DW_CASES, DW_CODES, FORCED_NAMES, GEMM_CASES, GEMM_CODES

pytestmark = pytest.mark.gpu

_BY_NAME = {c.name: c for c in GEMM_CASES + DW_CASES}


def _one_of_each_kind(names):
    """the first FcCase, 1x1 ConvCase, k x k ConvCase and DeconvCase; for depthwise the first 3x3 and the first 5x5"""
    picked = {}
    for case in (_BY_NAME[n] for n in names):
        if isinstance(case, FcCase):
            kind = "fc"
        elif isinstance(case, DeconvCase):
            kind = "deconv"
        elif wc.is_depthwise(case):
            kind = f"dw{case.kernel_size[0]}"
        else:
            kind = "1x1" if case.kernel_size == (1, 1) else "kxk"
        picked.setdefault(kind, case)
    return list(picked.values())


def _matrix():
    rows = []
    for (family, code), names in ACCEPTS.items():
        rows += [(family, code, case) for case in _one_of_each_kind(names)
                 if not isinstance(case, DeconvCase) or code in DECONV_CODES]
    rows += sorted({(family, 0, case) for family, _, case in rows}, key=lambda r: r[2].name)
    rows.sort(key=lambda r: (r[2].name, r[1]))       # one case after the other: the oracle cache holds two cases
    return [pytest.param(f, c, case, id=f"{case.name}-{f.split('_')[0]}{c}") for f, c, case in rows]


def _names(family, case, code):
    if code == 0:
        return None
    return DECONV_CODES[code] if isinstance(case, DeconvCase) else FORCED_NAMES[family][code]


def _create(lib, case, kernel, bias, run):
    tail = (case.izp, 1.0, case.kzp, run.kernel_scale, kernel, bias, run.zero_point, run.output_scale, run.qmin, run.qmax, 0)
    if isinstance(case, FcCase):
        return lib.create_fully_connected_nc_q8(case.input_channels, case.output_channels, *tail)
    geometry = (case.kernel_size[0], case.kernel_size[1], case.subsampling[0], case.subsampling[1], case.dilation[0],
                case.dilation[1], case.groups, case.gic, case.goc)
    if isinstance(case, DeconvCase):
        return lib.create_deconvolution2d_nhwc_q8(*case.padding, *case.adjustment, *geometry, *tail)
    return lib.create_convolution2d_nhwc_q8(*case.padding, *geometry, *tail)


def _setup(lib, op, case, d_in, d_out):
    if isinstance(case, FcCase):
        return lib.setup_fully_connected_nc_q8(op, case.batch, d_in, case.in_stride, d_out, case.out_stride)
    setup = lib.setup_deconvolution2d_nhwc_q8 if isinstance(case, DeconvCase) else lib.setup_convolution2d_nhwc_q8
    return setup(op, case.batch, case.input_size[0], case.input_size[1], d_in, case.in_stride, d_out, case.out_stride)


def run_once(lib, ops, run, d_in, size, dense=False):
    """create, set up, run, delete: (output, kernel name), or (None, status) when the forced code refuses"""
    op = None
    try:
        op = _create(lib, ops.case, ops.kernel, ops.bias, run)
        d_out = to_device(np.full(size, FILL, np.uint8))
        _setup(lib, op, ops.case, d_in, d_out)
        lib.run_operator(op)
        out = from_device(d_out)
        if dense:
            assert lib.operator_ran_dense(op), f"{ops.case.name}: gemm_kernel 31 ran, but not on the dense image"
        return out, lib.operator_kernel(op)
    except QnnpackError as e:
        return None, e.status
    finally:
        if op is not None:
            lib.delete_operator(op)


def check_bytes(out, expected, ops, what):
    try:
        assert_bytes_equal(out, expected, what)
    except AssertionError as e:
        i = int(np.flatnonzero(out != expected)[0]) if out.shape == expected.shape else 0
        row, ch = divmod(i, ops.case.out_stride)
        raise AssertionError(f"{e}; row {row}, channel {ch}, oracle accumulator {int(ops.acc[row, ch])}, "
                             f"bias {int(ops.bias[ch])}") from None


def sweep(lib, family, code, what, names, operand_sets, dense=False):
    """Every (label, regime, operands) of `operand_sets` at each of its runs under the forced code. Returns
    {regime: completed runs}, {label: kernel names} for the sets that ran."""
    done, ran = collections.Counter(), {}
    lib.set_option(family, code)
    try:
        uploaded = (None, None)
        for label, regime, ops in operand_sets:
            # (the non-vacuity conditions hold on the reference alone, before the device is touched)
            plan = [(run, wc.reference(ops, regime, run)) for run in wc.runs(regime, ops.product)]
            if uploaded[0] is not ops.input:     # once per operand set (both bounds of regime A share theirs)
                uploaded = (ops.input, to_device(ops.input))
            for run, expected in plan:
                where = (f"{what} at {label} regime {regime} scale {float(run.scale):.4e} zero point {run.zero_point} "
                         f"clamp [{run.qmin}, {run.qmax}]")
                out, got = run_once(lib, ops, run, uploaded[1], expected.size, dense)
                if out is None:
                    assert code != 0, f"{where}: the automatic choice refused a valid operator ({got.name})"
                    assert got == Status.unsupported_parameter, f"{where}: refused with {got.name}"
                    continue
                assert got is not None, where
                assert names is None or got in names, f"{where}: ran {got}, not one of {sorted(names)} -- a forced kernel rerouted"
                check_bytes(out, expected, ops, f"gfx950 {got} vs oracle [{where}]")
                done[regime] += 1
                ran.setdefault(label, set()).add(got)
    finally:
        lib.set_option(family, 0)
    return done, ran


def _report(what, ran, labels):
    taken = [l for l in labels if l in ran]
    kernels = sorted(set().union(*ran.values())) if ran else []
    print(f"WORSTCASE {what}: corners {'all' if taken == list(labels) else ' '.join(taken) or 'none'}; kernels {' '.join(kernels)}")


@pytest.mark.parametrize("family,code,case", _matrix())
def test_forced_kernel_with_worst_case_operands(qnnp, family, code, case):
    labels = [f"{izp}/{kzp}" for izp, kzp in wc.CORNERS]
    sets = ((f"{corner[0]}/{corner[1]}", regime, wc.operands(case, corner, regime))
            for corner in wc.CORNERS for regime in wc.regimes(case))
    what = f"{case.name} {family} {code}"
    done, ran = sweep(qnnp, family, code, what, _names(family, case, code), sets, dense=code == 31)
    _report(what, ran, labels)
    for regime in wc.regimes(case):
        assert done[regime] > 0, f"{what}: no run of regime {regime} completed ({dict(done)})"
    assert {"A30", "A31", "B"} <= set(done), f"{what}: {dict(done)}"
    if code == 0:
        assert set(ran) == set(labels)


EDGE = {k: FcCase(f"fc_edge_k{k}", 64, k, 64) for k in (16512, 16576)}


@pytest.mark.parametrize("code", [0] + GEMM_CODES)
def test_reduction_length_at_the_classification_edge(qnnp, code):
    """Fully connected, 64 rows x 64 channels, bias in +-10000: K = 16512 is the last reduction length classified b = 30
    (10000 + 65025 * 16512 < 2^30), K = 16576 -- the next multiple of 64 -- is b = 31. Density-1 rows meet density-1
    channels at the outer corners, so the accumulators sit where the classes part."""
    labels = [f"{k}:{izp}/{kzp}" for k in EDGE for izp, kzp in wc.OUTER_CORNERS]
    sets = []
    for k, case in EDGE.items():
        for corner in wc.OUTER_CORNERS:
            ops = wc.operands(case, corner, "E")
            top = int(np.abs(ops.acc.astype(np.int64)).max())
            assert top > (2 ** 30 - 2 ** 17 if k == 16512 else 2 ** 30), (k, corner, top)
            sets.append((f"{k}:{corner[0]}/{corner[1]}", "E", ops))
    what = f"classification edge, gemm_kernel {code}"
    done, ran = sweep(qnnp, "gemm_kernel", code, what, FORCED_NAMES["gemm_kernel"][code] if code else None, sets)
    _report(what, ran, labels)
    if code == 0:
        assert set(ran) == set(labels), f"{what}: ran only {sorted(ran)}"


@pytest.mark.parametrize("code", [0] + DW_CODES)
@pytest.mark.parametrize("name", ["dw3_c32", "dw5_c32"])
def test_depthwise_weight_range_classes(qnnp, name, code):
    """Every tap at w - kzp in {-255, -128, -127, 127, 128, 255} -- the three a kernel zero point reaches, one per block of
    eight channels -- against activations at both extremes, regime B's bias: the int16 weights, the int8 split of the
    matrix-core kernels and the dot4 class choice (pack.h: qnnp_dwconv_weight_range) at their ends."""
    case = _BY_NAME[name]
    labels = [f"{izp}/{kzp}" for izp, kzp in wc.CORNERS]
    sets = ((f"{c[0]}/{c[1]}", "B", wc.weight_range_operands(case, c)) for c in wc.CORNERS)
    what = f"{name} weight-range classes, dwconv_kernel {code}"
    done, ran = sweep(qnnp, "dwconv_kernel", code, what, FORCED_NAMES["dwconv_kernel"][code] if code else None, sets)
    _report(what, ran, labels)
    if code == 0:
        assert set(ran) == set(labels), f"{what}: ran only {sorted(ran)}"
    elif name in ACCEPTS.get(("dwconv_kernel", code), ()):
        assert ran, f"{what}: refused every corner"
