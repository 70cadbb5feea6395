/*
 * leaky-relu.c -- qnnp_create_leaky_relu_nc_q8 / qnnp_setup_leaky_relu_nc_q8 for the gfx950 build.
 *
 * Replaces reference src/leaky-relu.c:20-130 (create) and :132-157 (setup): same checks in the same order, same status
 * codes, and the same table -- the reference's float expressions restated term for term (the scale ratio, the slope
 * on the negative side, two comparisons, lrintf plus the zero point as a long) and compiled by the same host compiler
 * against the same libm, never on the device. The operator that comes out is the table operator of lut.c.
 *
 * Not part of the seam library (oracle/Makefile): there the reference's own leaky ReLU stays on the CPU.
 */
#include <inttypes.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "log.h"
#include "lut.h"
#include "state.h"

enum qnnp_status qnnp_create_leaky_relu_nc_q8(
    size_t channels,
    float negative_slope,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* leaky_relu)
{
  (void) flags;
  /* reference leaky-relu.c:35-38 */
  if (!qnnp_state.initialized) {
    qnnp_log_error("qnnp_create_leaky_relu_nc_q8 called before qnnp_initialize succeeded");
    return qnnp_status_uninitialized;
  }
  /* reference leaky-relu.c:40-77: invalid_parameter */
  if (channels == 0) {
    qnnp_log_error("cannot create leaky ReLU operator with %zu channels: number of channels must be non-zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if (negative_slope <= 0.0f || !isnormal(negative_slope)) {
    qnnp_log_error("cannot create leaky ReLU operator with %.7g negative slope: slope must be finite and positive",
        negative_slope);
    return qnnp_status_invalid_parameter;
  }
  if (negative_slope > 1.0f) {
    qnnp_log_error("cannot create leaky ReLU operator with %.7g negative slope: slope must not exceed 1.0", negative_slope);
    return qnnp_status_invalid_parameter;
  }
  if (input_scale <= 0.0f || !isnormal(input_scale)) {
    qnnp_log_error("cannot create leaky ReLU operator with %.7g input scale: scale must be finite and positive", input_scale);
    return qnnp_status_invalid_parameter;
  }
  if (output_scale <= 0.0f || !isnormal(output_scale)) {
    qnnp_log_error("cannot create leaky ReLU operator with %.7g output scale: scale must be finite and positive", output_scale);
    return qnnp_status_invalid_parameter;
  }
  if (output_min >= output_max) {
    qnnp_log_error("cannot create leaky ReLU operator with [%" PRIu8 ", %" PRIu8 "] output range: range min must be "
        "below range max", output_min, output_max);
    return qnnp_status_invalid_parameter;
  }
  /* reference leaky-relu.c:79-88: unsupported_parameter */
  const float input_output_scale = input_scale / output_scale;
  if (input_output_scale < 0x1.0p-8f || input_output_scale >= 0x1.0p+8f) {
    qnnp_log_error("cannot create leaky ReLU operator with %.7g input-to-output scale ratio: scale ratio must be in "
        "[2**-8, 2**8) range", input_output_scale);
    return qnnp_status_unsupported_parameter;
  }

  /* reference leaky-relu.c:104-117 */
  uint8_t table[256];
  const float scaled_min_less_zero_point = (float) ((int32_t) output_min - (int32_t) output_zero_point);
  const float scaled_max_less_zero_point = (float) ((int32_t) output_max - (int32_t) output_zero_point);
  for (int32_t i = 0; i < 256; i++) {
    const float x = input_output_scale * (float) (i - (int32_t) (uint32_t) input_zero_point);
    float y = x < 0.0f ? x * negative_slope : x;
    if (y < scaled_min_less_zero_point) {
      y = scaled_min_less_zero_point;
    }
    if (y > scaled_max_less_zero_point) {
      y = scaled_max_less_zero_point;
    }
    table[(uint32_t) i] = (uint8_t) (lrintf(y) + (long) output_zero_point);
  }
  return qnnp_create_lut_operator("leaky ReLU", channels, table, leaky_relu);
}

enum qnnp_status qnnp_setup_leaky_relu_nc_q8(
    qnnp_operator_t leaky_relu,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  return qnnp_setup_lut_operator("qnnp_setup_leaky_relu_nc_q8", leaky_relu, batch_size, input, input_stride, output,
                                 output_stride);
}
