"""GPU tier: the 256 x 256 GEMM on v_mfma_i32_16x16x64_i8 (qnnpack_amd/csrc/hip/q8gemm256x.hip) fetches its activations
in pairs of K tiles -- 128 contiguous bytes of a row per eight lanes -- through a ring of three pair slots beside three
weight-tile slots. Against the scalar oracle, byte for byte: every tile count from 8 to 26 (both parities -- an odd count
ends in an unpaired tile fetched as a 64-byte half --, every residue of the ring period of 6, the literal-slot kernel
at 10, 16 and 22 tiles and the run-time-slot kernels at all others), single-row and 255-row tensors, strided rows, a
strided 1x1 convolution, both centring classes and the row-sum flavour ("gemm_kernel" 23 and 28).
(The index maps and the schedule themselves are proven on the host: tests/test_gemm256x_map.py.)
The cases of a group run inside one test, a few seconds for the whole file: the message of a mismatch names the case."""
import pytest

from _cases import ConvCase, FcCase
from _gpu import from_device, to_device
from _runner import assert_bytes_equal, conv_expected, conv_run, fc_expected, fc_run

pytestmark = pytest.mark.gpu

C16 = "q8_gemm_mfma_256x256_c16"
R16 = "q8_gemm_mfma_256x256_r16"


@pytest.fixture
def forced(qnnp):
    def run(code, name, case):
        qnnp.set_option("gemm_kernel", code)
        try:
            if isinstance(case, ConvCase):
                expected, quant, out_hw = conv_expected(case)
                out, kname = conv_run(qnnp, case, quant, out_hw, to_device=to_device, from_device=from_device)
            else:
                expected, quant = fc_expected(case)
                out, kname = fc_run(qnnp, case, quant, to_device=to_device, from_device=from_device)
        finally:
            qnnp.set_option("gemm_kernel", 0)
        assert kname == name, (case.name, kname)
        assert_bytes_equal(out, expected, f"gfx950 {kname} vs oracle [{case.name}]")
    return run


def test_every_tile_count_from_8_to_26(forced):
    for tiles in range(8, 27):
        forced(23, C16, FcCase(f"kp_t{tiles}", 257, 64 * tiles, 256))


def test_short_tensors_and_strided_rows(forced):
    for k in (576, 640):             # an odd and an even tile count
        for m in (1, 255):
            forced(23, C16, FcCase(f"kp_m{m}_k{k}", m, k, 256))
        # a row's 128 bytes may straddle two cache lines: two requests, the same bytes
        forced(23, C16, FcCase(f"kp_strided_k{k}", 300, k, 256, input_stride=k + 16, output_stride=272))


def test_strided_pointwise_convolution(forced):
    forced(23, C16, ConvCase("kp_1x1_s2_576_256", (9, 11), subsampling=(2, 2), gic=576, goc=256, batch=3))


def test_other_kernel_zero_points(forced):
    forced(23, C16, FcCase("kp_kzp128_k704", 257, 704, 256, kzp=128))          # odd tile count
    for k in (704, 768):                                                      # the row-sum flavour, odd and even
        forced(28, R16, FcCase(f"kp_r16_k{k}", 257, k, 256, kzp=126))
