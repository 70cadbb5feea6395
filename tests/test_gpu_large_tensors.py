"""GPU tier: operators on tensors past 2^31 and 2^32 bytes, every output byte against the scalar oracle.

The fast kernels address memory through buffer descriptors (a 32-bit byte count, 32-bit lane offsets) or 32-bit offset
arithmetic, and each one's *_supported / plan_* guard refuses the tensors those cannot cover; the dispatch plans then fall
through to another kernel. A guard off by one, or one that checks the input but not the output, would read zeros, drop
stores or reach another image of the same tensor -- all of it plausible uint8. So the guards below are run on both sides
of their bounds: the largest tensor the guard still accepts (the case names the kernel it is there for) and the smallest
it refuses (another kernel runs, bit-exact). Covered: the 128-row unaligned GEMM (input span, flat-row stores), the wave
kernel's weight-stationary flavours (input and output terms), the patch kernel, the weight-stationary 16-channel kernel
(input and output terms), the 256x256 kernels through the offset table (centred and row-sum images), depthwise kernels
G (input and output terms) and H, the unaligned and the aligned sliding windows, and the four-channel generic kernel's
input term. The first-layer (3-channel) kernels, the long-K / one-wave streaming kernels, the 16x16x64 depthwise walk,
deconvolution, the folded residual add, the fused block at its setup limit, the per-channel kernels and multiply are in
tests/test_large_guards_gpu.py. Not covered in either file: the offset-table term of the first-layer streaming kernel.

At the first refused sizes every forced kernel code must refuse with the output and input untouched or be bit-exact (the
contract of test_gpu_kernel_contract.py). Tensors are periodic with marker units at the 2^31 / 2^32 boundaries
(_large.py); nothing of gigabyte size is copied to the host. The setup limits each operator documents are checked on
small buffers: one past the limit refuses, and a valid setup of the same operator afterwards runs bit-exact."""
import dataclasses
import functools

import numpy as np
import pytest

import _large as lg
import _pooling as pool
import _pointwise as pw
import _x8 as x8
import test_gpu_kernel_contract as contract
from _cases import ConvCase, DeconvCase, FcCase, conv_tensors, deconv_tensors, fc_tensors, seed_for
from _runner import FILL, assert_bytes_equal, conv_expected, deconv_expected, fc_expected
from oracle import o1
from qnnpack_amd import QnnpackError, Status
from test_gpu_kernel_contract import DW_CODES, FORCED_NAMES, GEMM_CODES, MUST_REFUSE

pytestmark = pytest.mark.gpu

P = lg.PERIOD
ROWS = 37           # rows per unit of the row-wise operators: not a tile multiple, so units straddle tiles


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    lg.free_memory()


@pytest.fixture(autouse=True)
def _release_after_each():
    yield
    lg.free_memory()


@dataclasses.dataclass
class Side:
    """one tensor of a problem: span, unit size, the P pattern units and the markers (index -> unit)"""
    span: int
    unit: int
    pattern: np.ndarray
    marks: dict


@dataclasses.dataclass
class Problem:
    name: str
    inputs: list                # [Side]
    output: Side
    create: object              # create(lib) -> op
    setup: object               # setup(lib, op, [d_in...], d_out)

    @property
    def nbytes(self):
        return sum(s.span for s in self.inputs) + self.output.span + 2 * lg.CHUNK


def _ok(status):
    if status != Status.success:
        raise QnnpackError("setup", status)


def _sides(count, spans_units, rng_name):
    """marker indices over all tensors and a random generator for the unique units"""
    return lg.markers(count, spans_units), np.random.default_rng(seed_for(rng_name))


def _split(mk, flat, unit, fill):
    """(pattern, marks) of the oracle's output over the P pattern units followed by the markers"""
    u = lg.units(flat, unit, P + len(mk), fill)
    return u[:P], {i: u[P + j] for j, i in enumerate(mk)}


# ---- convolutions (dense, depthwise) and fully connected ----
@functools.lru_cache(maxsize=None)
def conv_problem(case: ConvCase) -> Problem:
    H, W = case.input_size
    _, kern, bias = conv_tensors(dataclasses.replace(case, batch=1))
    oh, ow = o1.conv_output_hw(o1.conv_shape(1, H, W, case.padding, case.kernel_size, case.subsampling, case.dilation,
                                             case.groups, case.gic, case.goc, case.in_stride))
    cin, cout = case.groups * case.gic, case.groups * case.goc
    iu, ou = H * W * case.in_stride, oh * ow * case.out_stride
    ispan, ospan = (case.batch * H * W - 1) * case.in_stride + cin, (case.batch * oh * ow - 1) * case.out_stride + cout
    mk, rng = _sides(case.batch, [(ispan, iu), (ospan, ou)], case.name)
    n = P + len(mk)
    imgs = rng.integers(0, 256, size=(n, iu), dtype=np.uint8)
    small = dataclasses.replace(case, batch=n)
    out, quant, _ = conv_expected(small, imgs.reshape(-1)[:(n * H * W - 1) * case.in_stride + cin], kern, bias)
    opat, omarks = _split(mk, out, ou, FILL)

    def create(lib):
        return lib.create_convolution2d_nhwc_q8(
            case.padding[0], case.padding[1], case.padding[2], case.padding[3], case.kernel_size[0], case.kernel_size[1],
            case.subsampling[0], case.subsampling[1], case.dilation[0], case.dilation[1], case.groups, case.gic, case.goc,
            case.izp, 1.0, case.kzp, 1.0, kern, bias, quant[1], float(quant[0]), case.qmin, case.qmax, 0)

    def setup(lib, op, d_in, d_out):
        lib.setup_convolution2d_nhwc_q8(op, case.batch, H, W, d_in[0], case.in_stride, d_out, case.out_stride)

    return Problem(case.name, [Side(ispan, iu, imgs[:P], {i: imgs[P + j] for j, i in enumerate(mk)})],
                   Side(ospan, ou, opat, omarks), create, setup)


@functools.lru_cache(maxsize=None)
def fc_problem(case: FcCase) -> Problem:
    _, kern, bias = fc_tensors(dataclasses.replace(case, batch=1))
    K, N, si, so = case.input_channels, case.output_channels, case.in_stride, case.out_stride
    iu, ou = ROWS * si, ROWS * so
    ispan, ospan = (case.batch - 1) * si + K, (case.batch - 1) * so + N
    count = (case.batch + ROWS - 1) // ROWS
    mk, rng = _sides(count, [(ispan, iu), (ospan, ou)], case.name)
    n = P + len(mk)
    blocks = rng.integers(0, 256, size=(n, iu), dtype=np.uint8)
    small = dataclasses.replace(case, batch=n * ROWS)
    out, quant = fc_expected(small, blocks.reshape(-1)[:(n * ROWS - 1) * si + K], kern, bias)
    opat, omarks = _split(mk, out, ou, FILL)

    def create(lib):
        return lib.create_fully_connected_nc_q8(K, N, case.izp, 1.0, case.kzp, 1.0, kern, bias, quant[1], float(quant[0]),
                                                case.qmin, case.qmax, 0)

    def setup(lib, op, d_in, d_out):
        lib.setup_fully_connected_nc_q8(op, case.batch, d_in[0], si, d_out, so)

    return Problem(case.name, [Side(ispan, iu, blocks[:P], {i: blocks[P + j] for j, i in enumerate(mk)})],
                   Side(ospan, ou, opat, omarks), create, setup)


class Placed:
    """a problem's tensors on the device: inputs periodic with their markers, the output FILL"""

    def __init__(self, prob: Problem):
        lg.require_memory(prob.nbytes, prob.name)
        self.prob = prob
        self.inputs = []
        for k, s in enumerate(prob.inputs):
            t = lg.Tensor(s.span, salt=3 + k)
            t.fill_units(s.unit, s.pattern, s.marks)
            self.inputs.append(t)
        self.out = lg.Tensor(prob.output.span, salt=1)

    def run(self, lib, family=None, code=0):
        """(kernel name, None) or (None, status) when setup or run refuses"""
        self.out.fill(FILL)
        if family:
            lib.set_option(family, code)
        op = None
        try:
            op = self.prob.create(lib)
            self.prob.setup(lib, op, [t.view for t in self.inputs], self.out.view)
            lib.run_operator(op)
            return lib.operator_kernel(op), None
        except QnnpackError as e:
            return None, e.status
        finally:
            if op is not None:
                lib.delete_operator(op)
            if family:
                lib.set_option(family, 0)

    def check(self, what):
        o = self.prob.output
        self.out.assert_units(o.unit, o.pattern, o.marks, f"{what}, output")
        for k, (t, s) in enumerate(zip(self.inputs, self.prob.inputs)):
            t.assert_units(s.unit, s.pattern, s.marks, f"{what}: input {k} was written")

    def check_refused(self, what):
        self.out.assert_all(FILL, f"{what} (refused), output")
        for k, (t, s) in enumerate(zip(self.inputs, self.prob.inputs)):
            t.assert_units(s.unit, s.pattern, s.marks, f"{what} (refused): input {k} was written")


def run_auto(lib, prob: Problem, names=None, not_names=None):
    """code 0 on the problem: bit-exact, guards intact; the kernel in `names` / not in `not_names`"""
    placed = Placed(prob)
    got, status = placed.run(lib)
    assert got is not None, f"{prob.name}: the automatic choice refused a valid operator ({status.name})"
    placed.check(f"gfx950 {got} vs oracle [{prob.name}]")
    if names is not None:
        assert got in names, f"{prob.name}: ran {got}, the case is there for {sorted(names)}"
    if not_names is not None:
        assert got not in not_names, f"{prob.name}: ran {got}, which the guard should have refused at this size"
    return got


def run_forced(lib, prob: Problem, family, codes):
    """every forced code: refuses with the output all FILL, or reports one of its kernels and is bit-exact"""
    placed = Placed(prob)
    ran = {}
    for code in [0] + codes:
        what = f"{prob.name} {family} {code}"
        got, status = placed.run(lib, family, code)
        if got is None:
            assert code != 0, f"{what}: the automatic choice refused a valid operator ({status.name})"
            assert status == Status.unsupported_parameter, f"{what}: refused with {status.name}"
            placed.check_refused(what)
            continue
        names = FORCED_NAMES[family][code] if code else None
        assert names is None or got in names, f"{what}: ran {got}, not one of {sorted(names)} -- a forced kernel rerouted"
        assert (family, code) not in MUST_REFUSE, f"{what}: ran {got}; {MUST_REFUSE[(family, code)]}"
        placed.check(f"gfx950 {got} vs oracle [{what}]")
        ran[code] = got
    return ran


def _rows_below(bound, stride, channels):
    """the most rows whose span (rows - 1) * stride + channels stays below `bound`"""
    return (bound - 1 - channels) // stride + 1


U_NAMES = FORCED_NAMES["gemm_kernel"][29]
PW_NAMES = {"q8_pw_stream_mfma"}
WAVE_WS = {"q8_conv_wave_ws_mfma", "q8_conv_wave_ws_c_mfma", "q8_conv_wave_ws_c16_mfma"}
WS16S = FORCED_NAMES["gemm_kernel"][32]
PATCH = FORCED_NAMES["gemm_kernel"][22]
BIG_CENTRED = {"q8_gemm_mfma_256x256_c16", "q8_gemm_mfma_256x256_c", "q8_gemm_mfma_256x256_c_burst"}
BIG_ROWSUM = FORCED_NAMES["gemm_kernel"][28]      # the same kernel on the standard image with its row term (other zero points)
DW_COL = FORCED_NAMES["dwconv_kernel"][6]
DW_COL5 = {"q8_dwconv_col_5x5_dot4"}
B31, B32 = 1 << 31, 1 << 32

# 128-row GEMM (q8gemm128u.hip:gemm128u_supported): input span < 2^31
U_LAST = _rows_below(B31, 24, 24)
U_STRIDED_LAST = _rows_below(B31, 32, 24)
# its flat-row stores: rows * n < 2^32
U_FLAT_LAST = (B32 - 1) // 58
# 3x3 at 56x56 with 64 channels on one side: the weight-stationary wave flavours take inputs and outputs below 2^31 bytes
# (q8convwave.hip:convwave_launch); 64 -> 32 reaches the input term alone, 32 -> 64 the output term alone
C64_LAST = (B31 - 1) // (56 * 56 * 64)
# SqueezeNet's 55x55 fire modules on the weight-stationary 16-channel kernel (q8convws16s.hip:convws16s_supported): input and
# output each below 2^31 -- 16 -> 64 reaches the output term, 64 -> 16 the input term
WS_LAST = (B31 - 1) // (55 * 55 * 64)
# depthwise 3x3, 32 channels at 112x112: kernel G's batch * H * W * stride < 2^31 (q8dwconv.hip:plan_col)
DW32_LAST = (B31 - 1) // (112 * 112 * 32)
# ... and its output term, batch * OH * OW * out_stride < 2^32, with 68-byte output pixels: 5035 images below, 5036 past
DW32_O68_LAST = (B32 - 1) // (112 * 112 * 68)
# depthwise 5x5, 96 channels at 112x112 (MobileNet-style 5x5): kernel H's input term (q8dwconv.hip:plan_col5)
DW5_LAST = (B31 - 1) // (112 * 112 * 96)
# ShuffleNet v2's 58-channel depthwise 3x3 at 28x28, unaligned pixels: the sliding window on unaligned dwords, input < 2^32
# (q8dwconv.hip:plan_row)
DW58_LAST = (B32 - 1) // (28 * 28 * 58)
# ResNet-50's strided 1x1 through the offset table, 28x28 stride 2, 512 -> 1024 (with K = 256 the streaming kernel takes the
# 56x56 one at these row counts): the 256x256 centred kernels' images * image_stride + k_pad < 2^32
# (q8gemm256c.hip:gemm256c_supported, which the headline 16x16x64 kernel shares)
S2_LAST = (B32 - 1 - 512) // (28 * 28 * 512)


def _c33(name, hw, c, n, batch, **kw):
    return ConvCase(name, hw, (3, 3), (1, 1, 1, 1), gic=c, goc=n, batch=batch, **kw)


def _dw(name, hw, c, batch, k=3, **kw):
    return ConvCase(name, hw, (k, k), (k // 2,) * 4, groups=c, gic=1, goc=1, batch=batch, **kw)


def _s2(name, batch, kzp):
    return ConvCase(name, (28, 28), subsampling=(2, 2), gic=512, goc=1024, batch=batch, kzp=kzp)


PAIRS = [
    # (problem factory, case, kernels it must run, kernels it must not run)
    (fc_problem, FcCase("fc64_in_2g", 1 << 25, 64, 64), PW_NAMES, None),                       # input span exactly 2^31
    (fc_problem, FcCase("fc64_in_past_4g", (1 << 26) + 7, 64, 64), PW_NAMES, None),            # both spans past 2^32
    (fc_problem, FcCase("fc16_256_out_past_4g", (1 << 24) + 7, 16, 256), PW_NAMES, None),      # output past 2^32
    (fc_problem, FcCase("u_24_58_flat_last", U_FLAT_LAST, 24, 58), U_NAMES, None),             # flat rows, out < 2^32
    (fc_problem, FcCase("u_24_58_flat_past", U_FLAT_LAST + 1, 24, 58), U_NAMES, None),         # row stores past 2^32
    (fc_problem, FcCase("u_24_58_in_last", U_LAST, 24, 58), U_NAMES, None),
    (fc_problem, FcCase("u_24_58_in_refused", U_LAST + 1, 24, 58), None, U_NAMES),
    (fc_problem, FcCase("u_24_58_s32_in_last", U_STRIDED_LAST, 24, 58, input_stride=32), U_NAMES, None),
    (fc_problem, FcCase("u_24_58_s32_in_refused", U_STRIDED_LAST + 1, 24, 58, input_stride=32), None, U_NAMES),
    (conv_problem, _c33("c33_64_last", (56, 56), 64, 64, C64_LAST), WAVE_WS, None),
    (conv_problem, _c33("c33_64_refused", (56, 56), 64, 64, C64_LAST + 1), {"q8_conv_wave_mfma"}, None),
    (conv_problem, _c33("c33_64_32_in_last", (56, 56), 64, 32, C64_LAST), WAVE_WS, None),
    (conv_problem, _c33("c33_64_32_in_refused", (56, 56), 64, 32, C64_LAST + 1), None, WAVE_WS),
    (conv_problem, _c33("c33_32_64_out_last", (56, 56), 32, 64, C64_LAST), WAVE_WS, None),
    (conv_problem, _c33("c33_32_64_out_refused", (56, 56), 32, 64, C64_LAST + 1), {"q8_conv_wave_mfma"}, None),
    # the patch kernel's output span < 2^31 - 512 (q8convpatch.hip), one 128-byte row either side: 11 x 101 x 15101 =
    # 2^24 - 5 rows end 640 bytes short of 2^31, 17 x 21 x 46995 = 2^24 - 1 rows 128 bytes short (past 2^31 - 512)
    (conv_problem, _c33("c33_128_patch_last", (11, 101), 128, 128, 15101), PATCH, None),
    (conv_problem, _c33("c33_128_patch_refused", (17, 21), 128, 128, 46995), None, PATCH),
    (conv_problem, _c33("ws16s_16_64_out_last", (55, 55), 16, 64, WS_LAST), WS16S, None),
    (conv_problem, _c33("ws16s_16_64_out_refused", (55, 55), 16, 64, WS_LAST + 1), None, WS16S),
    (conv_problem, _c33("ws16s_64_16_in_last", (55, 55), 64, 16, WS_LAST), WS16S, None),
    (conv_problem, _c33("ws16s_64_16_in_refused", (55, 55), 64, 16, WS_LAST + 1), None, WS16S),
    (conv_problem, _s2("s2_512_1024_kzp127_last", S2_LAST, 127), BIG_CENTRED, None),
    (conv_problem, _s2("s2_512_1024_kzp127_refused", S2_LAST + 1, 127), None, BIG_CENTRED | BIG_ROWSUM),
    (conv_problem, _s2("s2_512_1024_kzp126_last", S2_LAST, 126), BIG_ROWSUM, None),
    (conv_problem, _s2("s2_512_1024_kzp126_refused", S2_LAST + 1, 126), None, BIG_CENTRED | BIG_ROWSUM),
    (conv_problem, _dw("dw3_c32_last", (112, 112), 32, DW32_LAST), DW_COL, None),
    (conv_problem, _dw("dw3_c32_refused", (112, 112), 32, DW32_LAST + 1), {"q8_dwconv_mfma_lds_3x3"}, None),
    (conv_problem, _dw("dw3_c32_o64_last", (112, 112), 32, DW32_LAST, output_pixel_stride=64), DW_COL, None),
    (conv_problem, _dw("dw3_c32_o68_last", (112, 112), 32, DW32_O68_LAST, output_pixel_stride=68), DW_COL, None),
    (conv_problem, _dw("dw3_c32_o68_refused", (112, 112), 32, DW32_O68_LAST + 1, output_pixel_stride=68), None, DW_COL),
    (conv_problem, _dw("dw5_c96_last", (112, 112), 96, DW5_LAST, k=5), DW_COL5, None),
    (conv_problem, _dw("dw5_c96_refused", (112, 112), 96, DW5_LAST + 1, k=5), None, DW_COL5),
    (conv_problem, _dw("dw3_c58_last", (28, 28), 58, DW58_LAST), {"q8_dwconv_row_3x3_any"}, None),
    (conv_problem, _dw("dw3_c58_refused", (28, 28), 58, DW58_LAST + 1), None, {"q8_dwconv_row_3x3_any"}),
]


@pytest.mark.parametrize("make,case,names,not_names", PAIRS, ids=[p[1].name for p in PAIRS])
def test_guard_bound(qnnp, make, case, names, not_names):
    run_auto(qnnp, make(case), names, not_names)


# Guards of kernels the automatic choice does not take at these shapes, run through their forced code: (case, family, code,
# the kernels the code reports at the last accepted size; at the first refused size the code must refuse)
FORCED_PAIRS = [
    # the aligned sliding window (kernel C), input < 2^32 (q8dwconv.hip:plan_row)
    (_dw("dw3_c32_row", (112, 112), 32, (B32 - 1) // (112 * 112 * 32)), "dwconv_kernel", 3, {"q8_dwconv_row_3x3"}),
    # the four-channel generic kernel's input term, input + 8 < 2^31 (q8dwconv.hip:direct4_fits)
    (_dw("dw3_c32_direct4", (112, 112), 32, (B31 - 9) // (112 * 112 * 32)), "dwconv_kernel", 9, {"q8_dwconv_direct4"}),
]


@pytest.mark.parametrize("case,family,code,names", FORCED_PAIRS, ids=[f[0].name for f in FORCED_PAIRS])
@pytest.mark.parametrize("side", ["last", "refused"])
def test_forced_guard_bound(qnnp, case, family, code, names, side):
    case = dataclasses.replace(case, name=f"{case.name}_{side}", batch=case.batch + (side == "refused"))
    placed = Placed(conv_problem(case))
    what = f"{case.name} {family} {code}"
    got, status = placed.run(qnnp, family, code)
    if side == "last":
        assert got in names, f"{what}: ran {got} ({status}), the case is there for {sorted(names)}"
        placed.check(f"gfx950 {got} vs oracle [{what}]")
    else:
        assert got is None and status == Status.unsupported_parameter, f"{what}: ran {got} ({status}) past the guard's bound"
        placed.check_refused(what)


FORCED = [
    (fc_problem, FcCase("u_24_58_in_refused", U_LAST + 1, 24, 58), "gemm_kernel", GEMM_CODES),
    (conv_problem, _c33("c33_64_refused", (56, 56), 64, 64, C64_LAST + 1), "gemm_kernel", GEMM_CODES),
    (conv_problem, _dw("dw3_c32_refused", (112, 112), 32, DW32_LAST + 1), "dwconv_kernel", DW_CODES),
]


@pytest.mark.parametrize("make,case,family,codes", FORCED, ids=[f[1].name for f in FORCED])
def test_forced_kernels_at_first_refused_size(qnnp, make, case, family, codes):
    run_forced(qnnp, make(case), family, codes)


# ---- the byte-streaming operators: 64-bit addressing, tensors past 2^32 bytes ----
def _rowwise(name, rows, channels, strides, oracle, create, setup, n_inputs=1):
    """rows of `channels` bytes at the given strides (inputs..., output); `oracle(n_rows, [inputs]) -> output`"""
    units = [ROWS * s for s in strides]
    spans = [(rows - 1) * s + channels for s in strides]
    count = (rows + ROWS - 1) // ROWS
    mk, rng = _sides(count, list(zip(spans, units)), name)
    n = P + len(mk)
    ins = [rng.integers(0, 256, size=(n, units[k]), dtype=np.uint8) for k in range(n_inputs)]
    out = oracle(n * ROWS, [x.reshape(-1)[:(n * ROWS - 1) * strides[k] + channels] for k, x in enumerate(ins)])
    opat, omarks = _split(mk, out, units[-1], FILL)
    sides = [Side(spans[k], units[k], x[:P], {i: x[P + j] for j, i in enumerate(mk)}) for k, x in enumerate(ins)]
    return Problem(name, sides, Side(spans[-1], units[-1], opat, omarks), create, setup)


def add_problem():
    c, strides = 64, (72, 64, 66)
    case = pw.AddCase("add_past_4g", (1 << 26) + 5, c, *strides)

    def oracle(rows, xs):
        return pw.add_expected(dataclasses.replace(case, batch=rows), xs[0], xs[1])
    return _rowwise(case.name, case.batch, c, strides, oracle,
                    lambda lib: lib.create_add_nc_q8(c, case.a_zp, case.a_scale, case.b_zp, case.b_scale, case.y_zp,
                                                     case.y_scale, case.qmin, case.qmax, 0),
                    lambda lib, op, d, y: lib.setup_add_nc_q8(op, case.batch, d[0], strides[0], d[1], strides[1], y, strides[2]),
                    n_inputs=2)


def x8_problem(kind):
    if kind == "shuffle":
        case = x8.X8Case("shuffle", "shuffle_g2_58_past_4g", ((1 << 32) // 116) + 3, groups=2, group_channels=58,
                         out_stride=120)
    else:
        case = x8.X8Case("clamp", "clamp_58_past_4g", ((1 << 32) // 58) + 3, clamp_channels=58, in_stride=61, out_stride=64,
                         qmin=17, qmax=230)

    def oracle(rows, xs):
        return x8.expected_one(dataclasses.replace(case, batch=rows), xs[0], rows)
    return _rowwise(case.name, case.batch, case.channels, case.strides, oracle,
                    lambda lib: x8.create(lib, case)[1],
                    lambda lib, op, d, y: _ok(x8.setup_status(lib, case, op, case.batch, d[0], y)))


def gap_problem():
    case = pw.GapCase("gap_past_4g", 0, 49, 64, in_stride=72, out_stride=67)
    si, so = case.strides
    batch = (1 << 32) // (49 * si) + 3
    iu = case.width * si
    ispan, ospan = (batch * case.width - 1) * si + case.channels, (batch - 1) * so + case.channels
    mk, rng = _sides(batch, [(ispan, iu), (ospan, so)], case.name)
    n = P + len(mk)
    imgs = rng.integers(0, 256, size=(n, iu), dtype=np.uint8)
    out = pw.gap_expected(dataclasses.replace(case, batch=n), imgs.reshape(-1)[:(n * case.width - 1) * si + case.channels])
    opat, omarks = _split(mk, out, so, FILL)
    return Problem(case.name, [Side(ispan, iu, imgs[:P], {i: imgs[P + j] for j, i in enumerate(mk)})], Side(ospan, so, opat, omarks),
                   lambda lib: lib.create_global_average_pooling_nwc_q8(case.channels, case.in_zp, case.in_scale, case.out_zp,
                                                                        case.out_scale, case.qmin, case.qmax, 0),
                   lambda lib, op, d, y: lib.setup_global_average_pooling_nwc_q8(op, batch, case.width, d[0], si, y, so))


def pool_problem(kind):
    if kind == "max":    # ShuffleNet's 3x3 stride-2 max pooling at 112x112x24, input past 2^32
        case = pool.PoolCase("max", "maxpool_past_4g", 0, 112, 112, 24, 3, 3, 1, 1, 1, 1, 2, 2, out_stride=26)
    else:
        case = pool.PoolCase("avg", "avgpool_past_4g", 0, 56, 56, 64, 3, 3, 1, 1, 1, 1, 2, 2, in_stride=72, out_stride=68,
                             in_scale=0.5, out_scale=0.75)
    si, so = case.strides
    H, W, C = case.input_height, case.input_width, case.channels
    oh, ow = case.output_size(H, W)
    iu, ou = H * W * si, oh * ow * so
    batch = (1 << 32) // iu + 3
    ispan, ospan = (batch * H * W - 1) * si + C, (batch * oh * ow - 1) * so + C
    mk, rng = _sides(batch, [(ispan, iu), (ospan, ou)], case.name)
    n = P + len(mk)
    imgs = rng.integers(0, 256, size=(n, iu), dtype=np.uint8)
    small = dataclasses.replace(case, batch=n)
    out = pool.expected(small, imgs.reshape(-1)[:(n * H * W - 1) * si + C])[0]
    opat, omarks = _split(mk, out, ou, FILL)
    big = dataclasses.replace(case, batch=batch)
    return Problem(case.name, [Side(ispan, iu, imgs[:P], {i: imgs[P + j] for j, i in enumerate(mk)})], Side(ospan, ou, opat, omarks),
                   lambda lib: pool.create(lib, big)[1],
                   lambda lib, op, d, y: _ok(pool.setup_status(lib, big, op, batch, H, W, d[0], y)))


STREAMING = {"add": add_problem, "gap": gap_problem, "shuffle": lambda: x8_problem("shuffle"),
             "clamp": lambda: x8_problem("clamp"), "maxpool": lambda: pool_problem("max"), "avgpool": lambda: pool_problem("avg")}


# the kernels of each (all 64-bit addressed): a dispatch change that moved one of these tensors elsewhere must show here
STREAMING_NAMES = {"add": {"q8_vadd_strided"}, "gap": {"q8_gavgpool_x1", "q8_gavgpool_x4"},
                   "shuffle": {"x8_shuffle_g2_x4", "x8_shuffle_g2_x16", "x8_shuffle_gather", "x8_shuffle_lds"},
                   "clamp": {"u8_clamp_rows_x1", "u8_clamp_rows_x4", "u8_clamp_rows_x16"},
                   "maxpool": {"q8_maxpool_x1", "q8_maxpool_x4", "q8_maxpool_x16"},
                   "avgpool": {"q8_avgpool_x1", "q8_avgpool_x4", "q8_avgpool_x16"}}


@pytest.mark.parametrize("which", sorted(STREAMING))
def test_streaming_operator_past_4g(qnnp, which):
    prob = STREAMING[which]()
    assert max(s.span for s in prob.inputs) > (1 << 32), prob.name
    run_auto(qnnp, prob, STREAMING_NAMES[which])


# ---- setup limits: one past refuses, and the operator still runs a valid setup bit-exact afterwards ----
def _small_conv(lib, case):
    inp, kern, bias = conv_tensors(case)
    expected, quant, out_hw = conv_expected(case, inp, kern, bias)
    return inp, kern, bias, expected, quant


def _refuse_then_run(lib, op, refused_setup, valid_setup, inp, expected, what):
    import torch
    d_in = torch.from_numpy(inp.copy()).cuda()
    d_out = torch.full((expected.size,), FILL, dtype=torch.uint8, device="cuda")
    st = refused_setup(d_in, d_out)
    assert st == Status.unsupported_parameter, f"{what}: one past the limit -> {st.name}"
    valid_setup(d_in, d_out)
    lib.run_operator(op)
    torch.cuda.synchronize()
    assert_bytes_equal(d_out.cpu().numpy(), expected, f"gfx950 {lib.operator_kernel(op)} after a refused setup [{what}]")


def _conv_op(lib, case, kern, bias, quant):
    return lib.create_convolution2d_nhwc_q8(
        case.padding[0], case.padding[1], case.padding[2], case.padding[3], case.kernel_size[0], case.kernel_size[1],
        case.subsampling[0], case.subsampling[1], case.dilation[0], case.dilation[1], case.groups, case.gic, case.goc,
        case.izp, 1.0, case.kzp, 1.0, kern, bias, quant[1], float(quant[0]), case.qmin, case.qmax, 0)


@pytest.mark.parametrize("limit", ["output_pixels", "image_bytes"])
def test_convolution_setup_limit(qnnp, limit):
    """convolution.c: batch * output pixels <= 2^31 - 1 and bytes per input image <= 2^31 - 1"""
    case = _c33("limit_conv", (9, 11), 16, 24, 2)
    inp, kern, bias, expected, quant = _small_conv(qnnp, case)
    op = _conv_op(qnnp, case, kern, bias, quant)
    try:
        if limit == "output_pixels":    # 1x1 output pixels per image ... 3x3 / pad 1 keeps H x W: batch (2^31 / 99) + 1
            n, h, w, s = (1 << 31) // 99 + 1, 9, 11, case.in_stride
            assert n * 99 > (1 << 32) // 2 - 1
        else:                           # one image of 2^31 bytes: 1 x 2^27 pixels of 16 bytes
            n, h, w, s = 1, 1, 1 << 27, 16
        _refuse_then_run(
            qnnp, op, lambda i, o: qnnp.setup_convolution2d_nhwc_q8_status(op, n, h, w, i, s, o, case.out_stride),
            lambda i, o: qnnp.setup_convolution2d_nhwc_q8(op, case.batch, 9, 11, i, case.in_stride, o, case.out_stride),
            inp, expected, f"convolution setup, {limit}")
    finally:
        qnnp.delete_operator(op)


def test_fully_connected_setup_limit(qnnp):
    """fully-connected.c: batch <= 2^31 - 1"""
    case = FcCase("limit_fc", 40, 24, 58)
    inp, kern, bias = fc_tensors(case)
    expected, quant = fc_expected(case, inp, kern, bias)
    op = qnnp.create_fully_connected_nc_q8(24, 58, case.izp, 1.0, case.kzp, 1.0, kern, bias, quant[1], float(quant[0]), 0, 255, 0)
    try:
        _refuse_then_run(qnnp, op, lambda i, o: qnnp.setup_fully_connected_nc_q8_status(op, 1 << 31, i, 24, o, 58),
                         lambda i, o: qnnp.setup_fully_connected_nc_q8(op, case.batch, i, 24, o, 58),
                         inp, expected, "fully connected setup")
    finally:
        qnnp.delete_operator(op)


def test_channel_shuffle_and_clamp_setup_limits(qnnp):
    """channel-shuffle.c / clamp.c: batch <= 2^31 - 1"""
    for case in (x8.X8Case("shuffle", "limit_shuffle", 33, groups=2, group_channels=29),
                 x8.X8Case("clamp", "limit_clamp", 33, clamp_channels=58, qmin=9, qmax=201)):
        x = x8.input_tensor(case)
        want = x8.expected_one(case, x, case.batch)
        op = x8.create(qnnp, case)[1]
        try:
            _refuse_then_run(qnnp, op, lambda i, o: x8.setup_status(qnnp, case, op, 1 << 31, i, o),
                             lambda i, o: _ok(x8.setup_status(qnnp, case, op, case.batch, i, o)),
                             x, want, f"{case.kind} setup")
        finally:
            qnnp.delete_operator(op)


# (batch, height, width) one past each limit of max-pooling.c / average-pooling.c for a 3x3 / stride 2 / pad 1 window over
# 24 channels: padded height, padded width, batch, batch x output height, output width x channels
POOL_LIMITS = {"padded_height": (1, 1 << 31, 10), "padded_width": (1, 9, 1 << 31), "batch": (1 << 32, 9, 10),
               "batch_x_output_height": ((1 << 32) // 5 + 1, 9, 10), "output_width_x_channels": (1, 9, 2 * ((1 << 31) // 24 + 1) - 1)}


@pytest.mark.parametrize("limit", sorted(POOL_LIMITS))
@pytest.mark.parametrize("kind", ["max", "avg"])
def test_pooling_setup_limit(qnnp, kind, limit):
    case = pool.PoolCase(kind, f"limit_{kind}pool", 2, 9, 10, 24, 3, 3, 1, 1, 1, 1, 2, 2)
    x = pool.input_tensor(case)
    want = pool.expected(case, x)[0]
    n, h, w = POOL_LIMITS[limit]
    oh, ow = case.output_size(h, w)
    assert case.output_size(9, 10)[0] == 5
    assert limit != "output_width_x_channels" or ow * 24 > (1 << 31) - 1 >= (ow - 1) * 24, ow
    op = pool.create(qnnp, case)[1]
    try:
        _refuse_then_run(qnnp, op, lambda i, o: pool.setup_status(qnnp, case, op, n, h, w, i, o),
                         lambda i, o: _ok(pool.setup_status(qnnp, case, op, 2, 9, 10, i, o)),
                         x, want, f"{kind} pooling setup, {limit}")
    finally:
        qnnp.delete_operator(op)


@pytest.mark.parametrize("limit", ["output_pixels", "image_bytes"])
def test_deconvolution_setup_limit(qnnp, limit):
    """deconvolution.c: batch * output pixels <= 2^31 - 1 and bytes per input image <= 2^31 - 1"""
    case = DeconvCase("limit_deconv", (6, 5), (2, 2), subsampling=(2, 2), gic=16, goc=19, batch=2)
    inp, kern, bias = deconv_tensors(case)
    expected, quant, (oh, ow) = deconv_expected(case, inp, kern, bias)
    op = qnnp.create_deconvolution2d_nhwc_q8(0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 1, 1, 1, 16, 19, case.izp, 1.0, case.kzp, 1.0,
                                             kern, bias, quant[1], float(quant[0]), 0, 255, 0)
    try:
        if limit == "output_pixels":    # 12 x 10 output pixels per 6 x 5 image
            n, h, w = (1 << 31) // (oh * ow) + 1, 6, 5
        else:                           # one image of 2^31 bytes: 1 x 2^27 pixels of 16 bytes
            n, h, w = 1, 1, 1 << 27
        _refuse_then_run(
            qnnp, op, lambda i, o: qnnp.setup_deconvolution2d_nhwc_q8_status(op, n, h, w, i, 16, o, 19),
            lambda i, o: qnnp.setup_deconvolution2d_nhwc_q8(op, case.batch, 6, 5, i, 16, o, 19),
            inp, expected, f"deconvolution setup, {limit}")
    finally:
        qnnp.delete_operator(op)


def test_fused_block_setup_limit(qnnp):
    """fused-block.c: input pixels x input stride <= 2^32 - 1 (and input pixels <= 2^31 - 1, which the first implies here)"""
    inp, stages, expected = contract._block_oracle()
    cin, cout = contract._BLOCK[0].gic, contract._BLOCK[2].goc
    H, W = contract._BLOCK[0].input_size
    ops, op = contract._fused(qnnp, stages)
    try:
        n = ((1 << 32) - 1) // (H * W * cin) + 1
        _refuse_then_run(qnnp, op, lambda i, o: qnnp.setup_fused_block_status(op, n, H, W, i, cin, o, cout),
                         lambda i, o: qnnp.setup_fused_block(op, contract._BLOCK[0].batch, H, W, i, cin, o, cout),
                         inp, expected, "fused block setup")
    finally:
        for h in [op] + ops:
            qnnp.delete_operator(h)
