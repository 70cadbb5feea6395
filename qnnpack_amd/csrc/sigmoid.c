/*
 * sigmoid.c -- qnnp_create_sigmoid_nc_q8 / qnnp_setup_sigmoid_nc_q8 for the gfx950 build.
 *
 * Replaces reference src/sigmoid.c:20-123 (create) and :125-150 (setup): same checks in the same order, same status
 * codes, and the same table -- the reference's float expressions restated term for term (expf, two comparisons, lrintf)
 * and compiled by the same host compiler against the same libm, never on the device. The operator that comes out is
 * the table operator of lut.c.
 *
 * Not part of the seam library (oracle/Makefile): there the reference's own sigmoid stays on the CPU.
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

enum qnnp_status qnnp_create_sigmoid_nc_q8(
    size_t channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* sigmoid)
{
  (void) flags;
  /* reference sigmoid.c:34-37 */
  if (!qnnp_state.initialized) {
    qnnp_log_error("qnnp_create_sigmoid_nc_q8 called before qnnp_initialize succeeded");
    return qnnp_status_uninitialized;
  }
  /* reference sigmoid.c:39-64: invalid_parameter */
  if (channels == 0) {
    qnnp_log_error("cannot create sigmoid operator with %zu channels: number of channels must be non-zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if (input_scale <= 0.0f || !isnormal(input_scale)) {
    qnnp_log_error("cannot create sigmoid operator with %.7g input scale: scale must be finite and positive", input_scale);
    return qnnp_status_invalid_parameter;
  }
  if (output_scale <= 0.0f || !isnormal(output_scale)) {
    qnnp_log_error("cannot create sigmoid operator with %.7g output scale: scale must be finite and positive", output_scale);
    return qnnp_status_invalid_parameter;
  }
  if (output_min >= output_max) {
    qnnp_log_error("cannot create sigmoid operator with [%" PRIu8 ", %" PRIu8 "] output range: range min must be below "
        "range max", output_min, output_max);
    return qnnp_status_invalid_parameter;
  }
  /* reference sigmoid.c:66-80: unsupported_parameter */
  if (output_scale != 0x1.0p-8f) {
    qnnp_log_error("cannot create sigmoid operator with %.7g output scale: only output scale of 1/256 is supported",
        output_scale);
    return qnnp_status_unsupported_parameter;
  }
  if (output_zero_point != 0) {
    qnnp_log_error("cannot create sigmoid operator with %" PRIu8 " output zero point: only output zero point of 0 is "
        "supported", output_zero_point);
    return qnnp_status_unsupported_parameter;
  }

  /* reference sigmoid.c:96-110 */
  uint8_t table[256];
  const float scaled_min = (float) (int32_t) output_min;
  const float scaled_max = (float) (int32_t) output_max;
  for (int32_t i = 0; i < 256; i++) {
    const float x = input_scale * (float) (i - (int32_t) (uint32_t) input_zero_point);
    /* sigmoid(x) / output scale, the output scale being 1 / 256 */
    float scaled_sigmoid_x = 256.0f / (1.0f + expf(-x));
    if (scaled_sigmoid_x < scaled_min) {
      scaled_sigmoid_x = scaled_min;
    }
    if (scaled_sigmoid_x > scaled_max) {
      scaled_sigmoid_x = scaled_max;
    }
    table[(uint32_t) i] = (uint8_t) lrintf(scaled_sigmoid_x);
  }
  return qnnp_create_lut_operator("sigmoid", channels, table, sigmoid);
}

enum qnnp_status qnnp_setup_sigmoid_nc_q8(
    qnnp_operator_t sigmoid,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  return qnnp_setup_lut_operator("qnnp_setup_sigmoid_nc_q8", sigmoid, batch_size, input, input_stride, output, output_stride);
}
