"""GPU tier: the size guards tests/test_gpu_large_tensors.py leaves out, run on both sides of their bounds, and the operators
added since on tensors past 2^32 bytes -- every output byte against the scalar oracle, with that file's machinery (periodic
tensors with marker units at 2^31 - 1, 2^31, 2^32 - 1 and 2^32, comparison on the device in chunks, require_memory, the
16 GiB budget of one case). The cases and the guards' arithmetic are in tests/_large_guards.py;
tests/test_large_guard_cases_host.py holds them to it on the CPU.

A pair (test_guard_pair) is one term of one guard. At the last accepted size the named kernel runs -- under the automatic
choice where that takes the shape, and under each forced code listed -- bit-exact, guards intact. At the first refused
size code 0 runs another kernel, bit-exact, and every forced code answers unsupported_parameter with output and input
untouched.

Pairs:
  q8convc3.hip conv_c3rows_supported     output, input, units*pairs, units*segs (codes 14 and 30; the two reciprocal-division
                                         shapes are outside the LDS flavour's plan: 14 only)
  q8convc3.hip conv_c3rows32_supported   output (7x7 stride 2), input (7x7 stride 3: at stride 2 sixteen output channels already
                                         write 16 x 16 x 16 = 4096 bytes per 3072-byte image, so the output term binds first;
                                         at stride 3 an image writes 11 x 11 x 16 = 1936)
  q8convc3.hip c3lds_plan                grid (added with this file, after the depthwise finding below: one workgroup per image
                                         and band; 2^24 one-pixel outputs of 1 x 16 x 3 images, which the plan took, answered
                                         unsupported_hardware from the launch under the automatic choice)
  q8pwconv.hip pwstream_gw_plan          input span, by rows (q8_pw_stream_gw_mfma) and by stride (q8_pw_stream_gwk_mfma,
                                         test_gwk_rows_by_stride: sparse rows)
  q8dwmfma16.hip dwmfma16_plan           output, input, (waves+8)*dmax -- reachable inside the other two: 1 x 1 images of 1040
                                         channels are 65 channel groups of one block, (65 batch + 8) * 65 passes 2^32 at
                                         1 016 560 images, 0.98 GiB -- and the grid term this file added: 1 x 1 images of 560
                                         channels first ran at their (waves+8)*dmax bound, 3 506 095 images = 122 713 325 waves
                                         in 30 678 332 workgroups of 256 work-items. The launch counts work-items in 32 bits:
                                         13 901 116 workgroups ran, and every image from number 1 588 698 on kept its fill
                                         bytes. dwmfma16_plan now refuses grids of 2^32 work-items and more (1 917 397 of
                                         those images), and dwmfma16_grid holds both sides of that
  q8deconv.hip qnnp_hip_deconv_s2_run    output, input
Both sides of a condition that is no refusal:
  q8convc3s.hip convstream_c3_plan       input 2^31: the staged flavour below, the unstaged from there, one kernel name
Terms that no tensor reaches:
  q8convc3.hip c3lds_plan wgs*bands      = batch * bands^2 <= batch * pairs^2 <= units*pairs, which conv_c3rows*_supported
                                         holds below 2^32 first (bands <= pairs; asserted per case in the host tier)
  q8pwconv.hip units < 2^31              units are 32 x 32 blocks of the output: 2^31 of them are 2 TiB of output
  q8deconv.hip bases + 32 < 2^31         at least 32 input channels keep the input term's tensor below 2^27 pixels, and
                                         BH <= H + 2, BW <= W + 2 (kernel <= 4, adjustment <= 1): bases <= 9 * 2^27
Left out:
  q8convc3s.hip convstream_c3 table      rows_per_image * taps * 4 reaches 2^31 only with 2^25 output pixels in ONE image
                                         under a 16-tap window: a 2 GiB offset table and an oracle run over 100 MB images
No size term at all:
  q8pwconv.hip long-K, staged plans    hold no size term (LDS bytes, channel and K conditions): q8_pw_stream_longk_mfma is
                                         run with the input past 2^32 and with the output past 2^32 instead
Past 2^32 without a guard (64-bit addressing): q8_conv_stream_c3_mfma's output, q8_pw_stream_d2s_mfma's output, the residual
add folded into a pointwise layer, the fused block at the last batch fused-block.c accepts, the per-channel kernels
q8_igemm_pc_mfma_128x64 and q8_dwconv_pc_w3s1, q8_mul_x16 and q8_mul_x1 over rows 2^31 + 16 / + 17 bytes apart.

Run time, seconds per id (call phase) on an MI355X in one run with tests/test_gpu_large_tensors.py (--durations=0, 106 ids in
23.9 s). Yardstick, the slowest id of that file in the same run: test_forced_kernels_at_first_refused_size[u_24_58_in_refused]
0.76 (then test_streaming_operator_past_4g[shuffle] 0.69). This file: test_fused_block_at_its_setup_limit 0.67,
test_multiply_rows_past_2g_apart[x16] 0.59, test_guard_pair[deconv_s2_input-refused] 0.10 and [-last] 0.08,
[dwmfma16_grid-last], [dwmfma16_waves-last] and [deconv_s2_output-refused] 0.06, test_per_channel_depthwise_past_4g 0.05, every
other id 0.04 or less (tensors are filled and compared on the device; the oracle runs on a dozen units).
"""
import dataclasses
import functools

import numpy as np
import pytest

import _fused as fb
import _large as lg
import _large_guards as G
import _multiply as mul
import _perchannel as pc
import test_gpu_large_tensors as big
from _cases import ConvCase, DeconvCase, FcCase, conv_tensors, deconv_tensors, fc_tensors, seed_for
from _runner import FILL, assert_bytes_equal, conv_expected, deconv_expected, fc_expected
from oracle import o1
from qnnpack_amd import QnnpackError, Status
from test_gpu_large_tensors import Placed, Problem, Side, run_auto

pytestmark = pytest.mark.gpu

P = lg.PERIOD
ROWS = G.ROWS


@pytest.fixture(autouse=True)
def _release_after_each():
    yield
    lg.free_memory()


# ---- problems ----
@functools.lru_cache(maxsize=None)
def deconv_problem(case: DeconvCase) -> Problem:
    H, W = case.input_size
    _, kern, bias = deconv_tensors(dataclasses.replace(case, batch=1))
    oh, ow = G.output_hw(case)
    cin, cout = case.groups * case.gic, case.groups * case.goc
    iu, ou = H * W * case.in_stride, oh * ow * case.out_stride
    ispan, ospan = G.spans(case)
    mk, rng = big._sides(case.batch, [(ispan, iu), (ospan, ou)], case.name)
    n = P + len(mk)
    imgs = rng.integers(0, 256, size=(n, iu), dtype=np.uint8)
    small = dataclasses.replace(case, batch=n)
    out, quant, _ = deconv_expected(small, imgs.reshape(-1)[:(n * H * W - 1) * case.in_stride + cin], kern, bias)
    opat, omarks = big._split(mk, out, ou, FILL)

    def create(lib):
        return lib.create_deconvolution2d_nhwc_q8(
            case.padding[0], case.padding[1], case.padding[2], case.padding[3], case.adjustment[0], case.adjustment[1],
            case.kernel_size[0], case.kernel_size[1], case.subsampling[0], case.subsampling[1], case.dilation[0], case.dilation[1],
            case.groups, case.gic, case.goc, case.izp, 1.0, case.kzp, 1.0, kern, bias, quant[1], float(quant[0]), case.qmin,
            case.qmax, 0)

    def setup(lib, op, d_in, d_out):
        lib.setup_deconvolution2d_nhwc_q8(op, case.batch, H, W, d_in[0], case.in_stride, d_out, case.out_stride)

    return Problem(case.name, [Side(ispan, iu, imgs[:P], {i: imgs[P + j] for j, i in enumerate(mk)})],
                   Side(ospan, ou, opat, omarks), create, setup)


def problem_of(case) -> Problem:
    if isinstance(case, DeconvCase):
        return deconv_problem(case)
    return big.fc_problem(case) if isinstance(case, FcCase) else big.conv_problem(case)


# ---- the pairs ----
@pytest.mark.parametrize("side", ["last", "refused"])
@pytest.mark.parametrize("pair", G.PAIRS, ids=G.PAIR_IDS)
def test_guard_pair(qnnp, pair, side):
    case = pair.case if side == "last" else pair.refused
    placed = Placed(problem_of(case))
    got, status = placed.run(qnnp)
    assert got is not None, f"{case.name}: the automatic choice refused a valid operator ({status.name})"
    placed.check(f"gfx950 {got} vs oracle [{case.name}]")
    if side == "last":
        assert pair.auto is None or got in pair.auto, f"{case.name}: ran {got}, the case is there for {sorted(pair.auto)}"
    else:
        assert got not in pair.names, f"{case.name}: ran {got}, which the guard should have refused at this size"
        assert pair.past is None or got in pair.past, f"{case.name}: ran {got}, not one of {sorted(pair.past)}"
    for code, names in pair.forced.items():
        what = f"{case.name} {pair.family} {code}"
        got, status = placed.run(qnnp, pair.family, code)
        if side == "last":
            assert got in names, f"{what}: ran {got} ({status}), the case is there for {sorted(names)}"
            placed.check(f"gfx950 {got} vs oracle [{what}]")
        else:
            assert got is None and status == Status.unsupported_parameter, f"{what}: ran {got} ({status}) past the guard's bound"
            placed.check_refused(what)


def _forced(lib, case, family, code, names):
    placed = Placed(problem_of(case))
    what = f"{case.name} {family} {code}"
    got, status = placed.run(lib, family, code)
    assert got in names, f"{what}: ran {got} ({status}), the case is there for {sorted(names)}"
    placed.check(f"gfx950 {got} vs oracle [{what}]")


@pytest.mark.parametrize("case", G.STREAM_C3, ids=[c.name for c in G.STREAM_C3])
def test_stream_c3_both_flavours_and_past_4g(qnnp, case):
    _forced(qnnp, case, "gemm_kernel", 7, G.C3_STREAM)


@pytest.mark.parametrize("case", G.LONGK_CASES, ids=[c.name for c in G.LONGK_CASES])
def test_longk_past_4g(qnnp, case):
    ispan, ospan = G.spans(case)
    assert max(ispan, ospan) > G.B32
    _forced(qnnp, case, "gemm_kernel", 9, G.LONGK)


def test_depth_to_space_output_past_4g(qnnp):
    prob = deconv_problem(G.D2S_CASE)
    assert prob.output.span > G.B32
    run_auto(qnnp, prob, G.D2S)


# ---- q8_pw_stream_gwk_mfma: the input span reached by the row stride, rows and their neighbourhoods only ----
BACKGROUND = 0x3C


@pytest.mark.parametrize("side", ["last", "refused"])
def test_gwk_rows_by_stride(qnnp, side):
    case = dataclasses.replace(G.GWK_CASE, batch=G.GWK_CASE.batch + (side == "refused"))
    rows, K, N = case.batch, case.input_channels, case.output_channels
    lg.require_memory(G.spans(case)[0] + rows * N, case.name)
    _, kern, bias = fc_tensors(dataclasses.replace(case, batch=1))
    x = np.random.default_rng(seed_for(case.name)).integers(0, 256, size=(rows, K), dtype=np.uint8)
    want, quant = fc_expected(FcCase(case.name, rows, K, N), x.reshape(-1), kern, bias)
    d_in = lg.SparseRows(rows, case.in_stride, K, salt=3)
    d_in.write(x, BACKGROUND)
    d_out = lg.Tensor(rows * N, salt=1)

    def run(code):
        d_out.fill(FILL)
        qnnp.set_option("gemm_kernel", code)
        op = None
        try:
            op = qnnp.create_fully_connected_nc_q8(K, N, case.izp, 1.0, case.kzp, 1.0, kern, bias, quant[1], float(quant[0]), 0, 255, 0)
            qnnp.setup_fully_connected_nc_q8(op, rows, d_in.view, case.in_stride, d_out.view, N)
            qnnp.run_operator(op)
            return qnnp.operator_kernel(op), None
        except QnnpackError as e:
            return None, e.status
        finally:
            qnnp.set_option("gemm_kernel", 0)
            if op is not None:
                qnnp.delete_operator(op)

    def check(what):
        assert_bytes_equal(d_out.view.cpu().numpy(), want, what)
        d_out.assert_guards(what)
        d_in.assert_rows(x, BACKGROUND, f"{what}: the input was written")

    got, status = run(0)
    assert got is not None, f"{case.name}: the automatic choice refused a valid operator ({status.name})"
    check(f"gfx950 {got} vs oracle [{case.name}]")
    if side == "refused":
        assert got not in G.GW | G.GWK, f"{case.name}: ran {got}, which the guard should have refused at this span"
    got, status = run(6)
    if side == "last":
        assert got in G.GWK, f"{case.name} gemm_kernel 6: ran {got} ({status}), the case is there for q8_pw_stream_gwk_mfma"
        check(f"gfx950 {got} vs oracle [{case.name} gemm_kernel 6]")
    else:
        assert got is None and status == Status.unsupported_parameter, f"{case.name} gemm_kernel 6: ran {got} ({status}) past the bound"
        d_out.assert_all(FILL, f"{case.name} gemm_kernel 6 (refused), output")
        d_in.assert_rows(x, BACKGROUND, f"{case.name} gemm_kernel 6 (refused): the input was written")


# ---- the residual add folded into a pointwise convolution ----
ADD_Q = dict(a_zp=121, a_scale=0.75, b_scale=1.25, y_zp=133, y_scale=0.96875, y_min=3, y_max=250)


def test_folded_residual_add_past_4g(qnnp):
    """1x1 16 -> 64 over 2^26 + 7 one-pixel images with the residual laid out like the output: both past 2^32. Expected: the
    oracle of the two-operator sequence, convolution then add(a = residual, b = convolution output)."""
    name, rows, cin, cout = "residual_16_64_past_4g", G.RESIDUAL_ROWS, 16, 64
    spans = [rows * cin, rows * cout, rows * cout]
    unit = [ROWS * cin, ROWS * cout, ROWS * cout]
    count = (rows + ROWS - 1) // ROWS
    mk, rng = big._sides(count, list(zip(spans, unit)), name)
    n = P + len(mk)
    x = rng.integers(0, 256, size=(n, unit[0]), dtype=np.uint8)
    res = rng.integers(0, 256, size=(n, unit[1]), dtype=np.uint8)
    case = ConvCase(name, (1, 1), gic=cin, goc=cout, batch=n * ROWS, izp=119, kzp=131)
    _, kern, bias = conv_tensors(dataclasses.replace(case, batch=1))
    conv, quant, _ = conv_expected(case, x.reshape(-1), kern, bias)
    y = np.full(n * unit[2], FILL, np.uint8)
    o1.add_q8(n * ROWS, cout, ADD_Q["a_zp"], ADD_Q["a_scale"], int(quant[1]), ADD_Q["b_scale"], ADD_Q["y_zp"], ADD_Q["y_scale"],
              ADD_Q["y_min"], ADD_Q["y_max"], res.reshape(-1), cout, conv, cout, y, cout)
    opat, omarks = big._split(mk, y, unit[2], FILL)

    def create(lib):
        return lib.create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, cin, cout, case.izp, 1.0, case.kzp, 1.0, kern, bias,
                                                int(quant[1]), float(quant[0]), 0, 255, 0)

    def setup(lib, op, d_in, d_out):
        lib.setup_convolution2d_nhwc_q8(op, rows, 1, 1, d_in[0], cin, d_out, cout)
        add = lib.create_add_nc_q8(cout, ADD_Q["a_zp"], ADD_Q["a_scale"], int(quant[1]), ADD_Q["b_scale"], ADD_Q["y_zp"],
                                   ADD_Q["y_scale"], ADD_Q["y_min"], ADD_Q["y_max"], 0)
        try:
            lib.attach_residual_add(op, add, d_in[1], cout)
        finally:
            lib.delete_operator(add)                    # its parameters were copied

    sides = [Side(spans[k], unit[k], t[:P], {i: t[P + j] for j, i in enumerate(mk)}) for k, t in enumerate((x, res))]
    prob = Problem(name, sides, Side(spans[2], unit[2], opat, omarks), create, setup)
    assert prob.output.span > G.B32 and prob.inputs[1].span > G.B32
    placed = Placed(prob)
    placed.out.fill(FILL)
    op = prob.create(qnnp)
    try:
        prob.setup(qnnp, op, [t.view for t in placed.inputs], placed.out.view)
        qnnp.run_operator(op)
        got, carried = qnnp.operator_kernel(op), qnnp.operator_residual_folded(op)
    finally:
        qnnp.delete_operator(op)
    assert carried == 1, f"{name}: {got} reports folded == {carried}: the add did not ride in the convolution's epilogue"
    placed.check(f"gfx950 {got} with the add folded vs oracle [{name}]")


# ---- the fused block at the last batch its setup accepts ----
def test_fused_block_at_its_setup_limit(qnnp):
    """the contract's block (28 x 28, 24 -> 144 -> 24) at batch (2^32 - 1) // (H W cin): the input ends less than one image short of 2^32.
    The oracle chain of tests/_fused.py runs on the pattern images and the markers."""
    import test_gpu_kernel_contract as contract
    cin, hidden, cout = contract._BLOCK[0].gic, contract._BLOCK[0].goc, contract._BLOCK[2].goc
    H, W = contract._BLOCK[0].input_size
    batch = (G.B32 - 1) // (H * W * cin)
    unit_in, unit_out = H * W * cin, H * W * cout
    mk = lg.markers(batch, [(batch * unit_in, unit_in), (batch * unit_out, unit_out)])
    n = P + len(mk)
    block = fb.build_block("fused_block_at_limit", fb.FIXED, cin=cin, hidden=hidden, cout=cout, h=H, w=W, batch=n, residual=False).check()
    imgs = block.inp.reshape(n, unit_in)
    opat, omarks = big._split(mk, block.expected(), unit_out, FILL)
    members = []

    def create(lib):
        members[:] = [st.create(lib) for st in block.stages]
        return lib.create_fused_block(members[0], members[1], members[2], None)

    def setup(lib, op, d_in, d_out):
        lib.setup_fused_block(op, batch, H, W, d_in[0], cin, d_out, cout)

    prob = Problem(block.name, [Side(batch * unit_in, unit_in, imgs[:P], {i: imgs[P + j] for j, i in enumerate(mk)})],
                   Side(batch * unit_out, unit_out, opat, omarks), create, setup)
    try:
        got = run_auto(qnnp, prob, {"q8_fused_strip"})
    finally:
        for h in members:
            qnnp.delete_operator(h)
    assert got == "q8_fused_strip"


# ---- per-channel operators ----
def test_per_channel_fully_connected_past_4g(qnnp):
    name, rows, K, N = "pc_fc_64_40_past_4g", G.PC_FC_ROWS, 64, 40
    spans, unit = [(rows - 1) * K + K, (rows - 1) * N + N], [ROWS * K, ROWS * N]
    mk = lg.markers((rows + ROWS - 1) // ROWS, list(zip(spans, unit)))
    n = P + len(mk)
    small = pc.fc_problem(name, n * ROWS, K, N).check()
    blocks = small.inp.reshape(n, unit[0])
    opat, omarks = big._split(mk, small.expected(N), unit[1], FILL)
    prob = Problem(name, [Side(spans[0], unit[0], blocks[:P], {i: blocks[P + j] for j, i in enumerate(mk)})],
                   Side(spans[1], unit[1], opat, omarks), small.create,
                   lambda lib, op, d_in, d_out: lib.setup_fully_connected_nc_q8(op, rows, d_in[0], K, d_out, N))
    assert spans[0] > G.B32
    run_auto(qnnp, prob, {"q8_igemm_pc_mfma_128x64"})


def test_per_channel_depthwise_past_4g(qnnp):
    name, batch, hw, C = "pc_dw_58_past_4g", G.PC_DW_BATCH, 28, 58
    unit = hw * hw * C
    mk = lg.markers(batch, [(batch * unit, unit)])
    n = P + len(mk)
    small = pc.conv_problem(name, n, (hw, hw), (3, 3), (1, 1, 1, 1), groups=C).check()
    imgs = small.inp.reshape(n, unit)
    opat, omarks = big._split(mk, small.expected(C), unit, FILL)
    prob = Problem(name, [Side(batch * unit, unit, imgs[:P], {i: imgs[P + j] for j, i in enumerate(mk)})],
                   Side(batch * unit, unit, opat, omarks), small.create,
                   lambda lib, op, d_in, d_out: lib.setup_convolution2d_nhwc_q8(op, batch, hw, hw, d_in[0], C, d_out, C))
    assert batch * unit > G.B32
    run_auto(qnnp, prob, {"q8_dwconv_pc_w3s1"})


# ---- multiply: rows more than 2^31 bytes apart in all three tensors ----
@pytest.mark.parametrize("stride,channels,kernel", [(G.MUL_STRIDE_X16, 1024, "q8_mul_x16"), (G.MUL_STRIDE_X1, 1021, "q8_mul_x1")],
                         ids=["x16", "x1"])
def test_multiply_rows_past_2g_apart(qnnp, stride, channels, kernel):
    """three b rows (one a row each); the last row of each tensor starts past 2^32. Only the rows and their neighbourhoods are
    written and compared."""
    rows, q = 3, mul.MID
    span = (rows - 1) * stride + channels
    assert (rows - 1) * stride > G.B32
    lg.require_memory(3 * span, f"multiply {kernel}")
    rng = np.random.default_rng(seed_for(f"mul_far_{kernel}"))
    a, b = (rng.integers(0, 256, size=(rows, channels), dtype=np.uint8) for _ in range(2))
    want = mul.product_rows(q, a, b)
    d_a, d_b, d_y = (lg.SparseRows(rows, stride, channels, salt=s) for s in (3, 4, 1))
    d_a.write(a, BACKGROUND)
    d_b.write(b, BACKGROUND)
    d_y.write(None, FILL)
    assert kernel == mul.kernel_for(mul.Shape(channels, rows, 1, stride, stride, stride), d_a.view.data_ptr(), d_b.view.data_ptr(),
                                    d_y.view.data_ptr())
    op = qnnp.create_multiply_nc_q8(channels, *q.args())
    try:
        qnnp.setup_multiply_nc_q8(op, rows, 1, d_a.view, stride, d_b.view, stride, d_y.view, stride)
        qnnp.run_operator(op)
        got = qnnp.operator_kernel(op)
    finally:
        qnnp.delete_operator(op)
    assert got == kernel, f"ran {got}, the case is there for {kernel}"
    d_y.assert_rows(want, FILL, f"gfx950 {got} vs oracle, rows {stride} bytes apart")
    d_a.assert_rows(a, BACKGROUND, f"{got}: a was written")
    d_b.assert_rows(b, BACKGROUND, f"{got}: b was written")
