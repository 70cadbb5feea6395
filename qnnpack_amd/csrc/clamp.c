/*
 * clamp.c -- qnnp_create_clamp_nc_u8 / qnnp_setup_clamp_nc_u8 for the gfx950 build.
 *
 * Replaces reference src/clamp.c:20-70 (create) and :72-97 (setup): same checks in the same order, same status codes.
 * The reference's clamping parameters (qnnp_compute_u8_clamping_params) reduce to the two bounds kept in
 * op->output_min / op->output_max. The run is the kernel of hip/x8shuffle.hip, reached through op->launch.
 *
 * Where the reference checks nothing and would go out of range, this build answers instead:
 *   - invalid_parameter: NULL tensors, pixel strides below the channel count, and input and output byte spans that
 *     overlap other than exactly in place (input == output with equal strides, which is supported);
 *   - unsupported_parameter: sizes beyond the kernels' index range (channels >= 2^31, batch >= 2^31).
 *
 * Not part of the seam library (oracle/Makefile): there the reference's own clamp stays on the CPU.
 */
#include <inttypes.h>
#include <stddef.h>
#include <stdint.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"

static int launch_clamp(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  /* reference operator-run.c:1054-1089 */
  const struct qnnp_hip_x8_args args = {
    .input = (const uint8_t*) input,
    .output = (uint8_t*) output,
    .pixels = (uint32_t) op->batch_size,
    .channels = (uint32_t) op->channels,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
    .output_min = op->output_min,
    .output_max = op->output_max,
  };
  return qnnp_hip_clamp_run(&args, &op->kernel_name);
}

static enum qnnp_status create_clamp(
    size_t channels,
    uint8_t output_min,
    uint8_t output_max,
    qnnp_operator_t* clamp_out)
{
  /* reference clamp.c:35-48 */
  if (channels == 0) {
    qnnp_log_error("cannot create clamp operator with %zu channels: number of channels must be non-zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if (output_min > output_max) {
    qnnp_log_error("cannot create clamp operator with [%" PRIu8 ", %" PRIu8 "] output range: range min must be below "
        "range max", output_min, output_max);
    return qnnp_status_invalid_parameter;
  }
  if (channels > (size_t) INT32_MAX) {
    qnnp_log_error("cannot create clamp operator: %zu channels exceed the device kernel's index range", channels);
    return qnnp_status_unsupported_parameter;
  }

  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_clamp, launch_clamp);
  if (op == NULL) {
    return qnnp_status_out_of_memory;
  }
  op->channels = channels;
  op->output_min = output_min;
  op->output_max = output_max;
  *clamp_out = op;
  return qnnp_status_success;
}

enum qnnp_status qnnp_create_clamp_nc_u8(
    size_t channels,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* clamp)
{
  (void) flags;
  int token;
  /* reference clamp.c:30-33 */
  const enum qnnp_status status = qnnp_enter_create("qnnp_create_clamp_nc_u8", &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token, create_clamp(channels, output_min, output_max, clamp));
}

enum qnnp_status qnnp_setup_clamp_nc_u8(
    qnnp_operator_t clamp,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  int token;
  /* reference clamp.c:80-83 */
  enum qnnp_status status = qnnp_enter_setup("qnnp_setup_clamp_nc_u8", clamp, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  /* reference clamp.c:85-97 */
  status = clamp->ukernel_type != qnnp_ukernel_type_clamp ? qnnp_status_invalid_parameter :
      qnnp_setup_nc(clamp, "qnnp_setup_clamp_nc_u8", 1, batch_size, input, input_stride, output, output_stride);
  return qnnp_leave_setup(clamp, token, status);
}
