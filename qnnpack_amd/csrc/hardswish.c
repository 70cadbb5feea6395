/*
 * hardswish.c -- qnnp_gfx950_create_hardswish_nc_q8: x * relu6(x + 3) / 6 as a 256-byte table on the table operator of lut.c.
 *
 * No reference counterpart (PyTorch's later fork of QNNPACK has the operator; this is written from the definition in
 * include/qnnpack_gfx950.h). The checks and their order are sigmoid.c's. The table is built on the host at create, in
 * float32 with every operation rounded once: each step below is its own statement, and the
 * Makefile compiles this file with -ffp-contract=off so that no multiply and add fuse. lrintf rounds to nearest even.
 * Setup, run and delete are the table operator's (qnnp_gfx950_setup_lut_nc_x8).
 *
 * Not part of the seam library (oracle/Makefile).
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

enum qnnp_status qnnp_gfx950_create_hardswish_nc_q8(
    size_t channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* hardswish)
{
  (void) flags;
  if (!qnnp_state.initialized) {
    qnnp_log_error("qnnp_gfx950_create_hardswish_nc_q8 called before qnnp_initialize succeeded");
    return qnnp_status_uninitialized;
  }
  if (channels == 0) {
    qnnp_log_error("cannot create hardswish operator with %zu channels: number of channels must be non-zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if (input_scale <= 0.0f || !isnormal(input_scale)) {
    qnnp_log_error("cannot create hardswish operator with %.7g input scale: scale must be finite and positive", input_scale);
    return qnnp_status_invalid_parameter;
  }
  if (output_scale <= 0.0f || !isnormal(output_scale)) {
    qnnp_log_error("cannot create hardswish operator with %.7g output scale: scale must be finite and positive", output_scale);
    return qnnp_status_invalid_parameter;
  }
  if (output_min >= output_max) {
    qnnp_log_error("cannot create hardswish operator with [%" PRIu8 ", %" PRIu8 "] output range: range min must be below "
        "range max", output_min, output_max);
    return qnnp_status_invalid_parameter;
  }

  uint8_t table[256];
  const float scaled_min = (float) (int32_t) output_min;
  const float scaled_max = (float) (int32_t) output_max;
  const float inv_output_scale = 1.0f / output_scale;
  const float zero_point = (float) (int32_t) output_zero_point;
  for (int32_t i = 0; i < 256; i++) {
    const float x = input_scale * (float) (i - (int32_t) (uint32_t) input_zero_point);
    /* relu6(x + 3) */
    float h = x + 3.0f;
    if (h < 0.0f) {
      h = 0.0f;
    }
    if (h > 6.0f) {
      h = 6.0f;
    }
    /* x * relu6(x + 3) / 6, in the output's units */
    const float xh = x * h;
    const float hardswish_x = xh / 6.0f;
    const float scaled = inv_output_scale * hardswish_x;
    float y = scaled + zero_point;
    if (!(y >= scaled_min)) {   /* (a NaN too: an input scale so large that x overflows) */
      y = scaled_min;
    }
    if (y > scaled_max) {
      y = scaled_max;
    }
    table[(uint32_t) i] = (uint8_t) lrintf(y);
  }
  return qnnp_create_lut_operator("hardswish", channels, table, hardswish);
}
