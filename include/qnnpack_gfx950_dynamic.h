/*
 * qnnpack_gfx950_dynamic.h -- a DYNAMICALLY QUANTIZED fully connected operator: float32 in, float32 out, int8 on the
 * matrix cores in between (W8A8 with one activation scale per row -- per token --, one weight scale per output channel).
 * The caller needs no calibrated activation range: every input row is quantized to its own range inside the operator.
 * This is the shape of PyTorch's quantized::linear_dynamic, of transformer and recommender MLPs, LSTM / GRU gates and
 * the classifier head of a float model. No reference counterpart. An operator behind qnnp_run_operator /
 * qnnp_delete_operator like every other one: it records into the library's hipGraph capture (as its two launches), runs
 * on the library stream, and takes host tensors through the device staging.
 *
 * Definition (bit-exact, no tolerance). All arithmetic is float32, every operation rounded once (no fused multiply-add),
 * in this order. Per input row r, with K = input_channels:
 *   lo = min(0, min_k x[r][k]);  hi = max(0, max_k x[r][k])           NaN elements are ignored by the min and the max
 *   scale_r = (hi - lo) / 255.0f                                        an IEEE division
 *   if !(scale_r >= 0x1p-60f && scale_r <= 0x1p60f)  scale_r = 1.0f    all-zero rows, overflowed and denormal ranges
 *   inv = 1.0f / scale_r;  zp_r = (int32) rintf(min(-lo * inv, 255.0f))          ties to even
 *   t = x * inv;  t = isnan(t) ? 0 : t;  t = min(max(t, (float) -zp_r), (float) (255 - zp_r))
 *   q = (int32) rintf(t) + zp_r                                         in [0, 255]
 * Per output (r, c):
 *   acc = sum_k (q[r][k] - zp_r) * kernel[c][k]                         exact in int32
 *   s = scale_r * kernel_scales[c]
 *   y = (float) acc * s;  y = y + bias[c];  y = min(max(y, output_min), output_max)      (float) acc: to nearest even
 * The bytes are THIS definition's, not PyTorch's: quantized::linear_dynamic nudges its zero point differently.
 *
 * No result depends on the denormal mode. Output side: kernel_scales lie in [2^-20, 2^20], a row scale that passes the
 * test above is at least 2^-60 and a bias is zero or a normal number. So s >= 2^-80 is normal, a nonzero product
 * (float) acc * s is at least 2^-80, and a sum y + bias that cancels is zero or a multiple of about 2^-103 (the last
 * place of a product of that size): never a denormal. Input side: a denormal x gives |x * inv| < 2^-126 * 2^60, which
 * rounds to the zero point flushed or not; and a range hi - lo that is denormal or flushed to zero fails the test above
 * either way and takes scale 1.
 *
 * The accumulator cannot wrap: |q - zp_r| <= 255, |kernel| <= 128, K <= 32768 give |acc| <= 255 * 128 * 32768 < 2^31.
 * The kernels compute it as sum_k (q - 128) * kernel[c][k] + (128 - zp_r) * wsum[c] with wsum[c] = sum_k kernel[c][k]:
 * either part is at most 2^29 in magnitude.
 *
 * Create answers, in this order: uninitialized; invalid_parameter for a zero channel count, a NULL kernel or
 * kernel_scales, a scale that is not a normal number above zero, a bias that is NaN, infinite or denormal, an
 * output_min or output_max that is NaN, output_min > output_max; unsupported_parameter for a scale outside
 * [2^-20, 2^20], input_channels > 32768, output_channels >= 2^24; out_of_memory. A refused create writes no handle.
 * kernel, kernel_scales and bias are host memory, read during the call and not kept. bias == NULL means all zero;
 * -INFINITY / +INFINITY as output_min / output_max mean no clamp. `flags` is accepted and ignored.
 *
 * Setup follows qnnpack_gfx950_float.h: both strides count ELEMENTS. batch_size == 0 succeeds and the run does nothing.
 * invalid_parameter: a NULL tensor, a pointer that is not 4-byte aligned, a stride below the channel count of its side,
 * input and output byte spans that share a byte, memory of another GPU, a call inside a graph capture.
 * unsupported_parameter: batch_size >= 2^31. Every check comes before the operator changes: a refused setup leaves the
 * previous one runnable. Setup grows the one device scratch the operator owns (the quantized rows, k_pad = K rounded up
 * to 64 bytes each, and eight bytes per row of scale and zero point); it never shrinks and is freed with the operator.
 *
 * Kernels. A run is two launches, chosen by batch_size and K alone (and the input's alignment for the load width):
 *   rows (hip/f32qd8rows.hip; qnnp_gfx950_dynamic_rows_kernel names it)
 *     f32_qd8_rows_wave      K <= 1024       one wave per row
 *     f32_qd8_rows_block     K <= 16384      one workgroup per row, the row read once and kept in registers
 *     f32_qd8_rows_twopass   K <= 32768      the row is read twice
 *     each with _x4 behind its name where the input base or, with more than one row, the input stride is no multiple of
 *     16 bytes: 4-byte loads
 *   matrix product and float epilogue (hip/qd8f32gemm.hip; qnnp_gfx950_operator_kernel names it)
 *     qd8_f32_gemv_mfma_16        batch_size <= 16
 *     qd8_f32_gemm_mfma_128x128   batch_size > 16
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qnnpack_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8(
    size_t input_channels,
    size_t output_channels,
    const int8_t* kernel,          /* [output_channels][input_channels], symmetric int8, host */
    const float* kernel_scales,    /* [output_channels], host */
    const float* bias,             /* [output_channels] float32, host; NULL means all zero */
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected);

/*
 * The same operator with 4-BIT weights (qd8-f32-qc4w: one scale per output channel, no block-wise scales). Byte k / 2 of
 * row c of `kernel` holds weight (c, k) in bits 4 (k % 2) .. 4 (k % 2) + 3, a two's-complement signed nibble in [-8, 7];
 * with an odd input_channels the high nibble of a row's last byte is ignored, whatever it holds. The definition above
 * holds with kernel[c][k] read as that nibble, and nothing else changes: |acc| <= 255 * 8 * 32768 < 2^31. The kernels
 * feed the matrix cores 16 * kernel[c][k] (the nibble in the top half of an int8), so their loop sums
 * 16 * sum_k (q - 128) * kernel[c][k], at most 128 * 128 * 32768 = 2^29 in magnitude, and shift it right by four: exact.
 *
 * Statuses and their order are those of qnnp_gfx950_create_fully_connected_nc_f32_qd8, the limits
 * input_channels <= 32768 and output_channels < 2^24 included. The handle is set up with
 * qnnp_gfx950_setup_fully_connected_nc_f32_qd8 and is run, captured, named and deleted like the int8 one: the row launch and
 * the scratch are the same, only the weight image (half the bytes, K rounded up to 128) and the second launch differ
 * (hip/qd8f32gemm4.hip; qnnp_gfx950_operator_kernel names it):
 *     qd8_f32_qc4w_gemv_mfma_16        batch_size <= 16
 *     qd8_f32_qc4w_gemm_mfma_128x128   batch_size > 16
 */
enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8_qc4w(
    size_t input_channels,
    size_t output_channels,
    const uint8_t* kernel,         /* [output_channels][(input_channels + 1) / 2], two signed nibbles per byte, host */
    const float* kernel_scales,    /* [output_channels], host */
    const float* bias,             /* [output_channels] float32, host; NULL means all zero */
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected);

enum qnnp_status qnnp_gfx950_setup_fully_connected_nc_f32_qd8(
    qnnp_operator_t fully_connected,
    size_t batch_size,
    const float* input,
    size_t input_stride,
    float* output,
    size_t output_stride);

/* Name of the row kernel the operator's last run launched in front of the kernel qnnp_gfx950_operator_kernel names
 * (static string), or NULL: before the first run, or for a handle of another kind. */
const char* qnnp_gfx950_dynamic_rows_kernel(qnnp_operator_t fully_connected);

#ifdef __cplusplus
}
#endif
