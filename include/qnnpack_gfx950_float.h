/*
 * qnnpack_gfx950_float.h -- the two ends of a quantized network: float32 -> uint8 (quantize) and uint8 -> float32
 * (dequantize), as operators behind qnnp_run_operator / qnnp_delete_operator like every other one, so that they record
 * into the library's hipGraph capture and run on the library stream. No reference counterpart.
 *
 * Each operator type has two setups, and one handle may be set up either way (the last successful setup decides):
 *   rows (NC)   `batch_size` rows of `channels` elements on both sides. The stride of the float tensor is in ELEMENTS,
 *               the stride of the uint8 tensor in bytes.
 *   planar      the float tensor is dense NCHW (PyTorch's layout): element (n, c, p) at float index
 *               (n * channels + c) * pixels + p, with pixels = height * width. The uint8 tensor is NHWC: pixel (n, p) at
 *               byte (n * pixels + p) * pixel_stride, `channels` bytes; the stride may exceed `channels`, so the operator
 *               can write into (read from) a channel slice of a wider tensor. Quantizing while transposing moves 5 bytes
 *               per element, where a permute followed by a quantize moves 13.
 *
 * Arithmetic: float32, every operation rounded once (no fused multiply-add), bit-exact by definition.
 *   quantize    inv = 1.0f / output_scale;  t = x * inv;  t = isnan(t) ? 0.0f : t;
 *               t = min(max(t, (float) (output_min - output_zero_point)), (float) (output_max - output_zero_point));
 *               y = (uint8) ((int32) rintf(t) + output_zero_point), ties to even.
 *               NaN of any payload and +-0 give the clamped zero point; +-inf and huge values saturate.
 *   dequantize  y = (float) ((int32) x - input_zero_point) * input_scale: one multiply, exact in the integer part.
 * A scale has to lie in [2^-118, 2^118]. That keeps `inv` a normal number and 255 * scale finite; a dequantized value is
 * never a denormal; and every denormal input of quantize has |x * inv| < 2^-8, which rounds to the zero point whether
 * the hardware flushes denormals or not. So no result depends on the denormal mode.
 *
 * Create answers, in this order: uninitialized; invalid_parameter for channels == 0, for a scale that is not a normal
 * number above zero, for quantize with output_min >= output_max; unsupported_parameter for channels >= 2^31, for a
 * scale outside [2^-118, 2^118]. `flags` is accepted and ignored.
 *
 * Setup: batch_size == 0 succeeds and the run does nothing. invalid_parameter: a NULL tensor, pixels == 0, a float
 * pointer that is not 4-byte aligned, a stride below `channels`, input and output byte spans that share a byte (there is
 * no in-place form; the float side spans 4 bytes per element), memory of another GPU, a call inside a graph capture.
 * unsupported_parameter: batch_size, batch_size * pixels or channels * pixels at or above 2^31. Every check comes before
 * the operator changes: a refused setup leaves the previous one runnable. Host tensors are staged like any operator's.
 *
 * Kernels (hip/f32q8.hip; qnnp_gfx950_operator_kernel names the one that ran). Rows that are dense on both sides
 * (both strides == channels), or a single row, count as ONE row of batch_size * channels elements. Then the widest
 * piece W of 16, 4, 1 bytes is taken for which the uint8 base address -- and, with more than one row, the uint8 stride --
 * is a multiple of W, and for W = 16 also the float base address is a multiple of 16 bytes and, with more than one row,
 * the float stride a multiple of 4 elements: f32q8_quantize_x16 / _x4 / _x1, f32q8_dequantize_x16 / _x4 / _x1. The channel
 * count does not enter: the last piece of a row may be partial. The planar setups run f32q8_quantize_planar and
 * f32q8_dequantize_planar at any channel count, pixel count and byte-side alignment.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qnnpack_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

enum qnnp_status qnnp_gfx950_create_quantize_nc_f32_q8(
    size_t channels, uint8_t output_zero_point, float output_scale,
    uint8_t output_min, uint8_t output_max, uint32_t flags, qnnp_operator_t* quantize);
enum qnnp_status qnnp_gfx950_setup_quantize_nc_f32_q8(
    qnnp_operator_t quantize, size_t batch_size,
    const float* input, size_t input_stride, uint8_t* output, size_t output_stride);
enum qnnp_status qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(
    qnnp_operator_t quantize, size_t batch_size, size_t pixels,
    const float* input, uint8_t* output, size_t output_pixel_stride);

enum qnnp_status qnnp_gfx950_create_dequantize_nc_q8_f32(
    size_t channels, uint8_t input_zero_point, float input_scale,
    uint32_t flags, qnnp_operator_t* dequantize);
enum qnnp_status qnnp_gfx950_setup_dequantize_nc_q8_f32(
    qnnp_operator_t dequantize, size_t batch_size,
    const uint8_t* input, size_t input_stride, float* output, size_t output_stride);
enum qnnp_status qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(
    qnnp_operator_t dequantize, size_t batch_size, size_t pixels,
    const uint8_t* input, size_t input_pixel_stride, float* output);

#ifdef __cplusplus
}
#endif
