/*
 * softargmax.c -- qnnp_create_softargmax_nc_q8 / qnnp_setup_softargmax_nc_q8 for the gfx950 build.
 *
 * Replaces reference src/softargmax.c:20-104 (create) and :106-131 (setup): same checks in the same order, same status
 * codes, and the same table of 256 uint32_t -- the reference's double expressions restated term for term (fmin, exp,
 * lrint) and compiled by the same host compiler against the same libm, never on the device. The table is uploaded once
 * at create, to the create's device, and kept in op->d_weights (freed by qnnp_delete_operator); the run is the kernels
 * of hip/q8softargmax.hip, reached through op->launch.
 *
 * The reference's setup checks nothing but the initialization. Where it would go out of range, this build answers
 * instead, as lut.c does:
 *   - invalid_parameter: NULL tensors, row strides below the channel count, and input and output byte spans that
 *     overlap other than exactly in place (input == output with equal strides, which is supported, as the reference's
 *     byte-serial kernel supports it);
 *   - unsupported_parameter: sizes beyond the kernels' index range (channels >= 2^31 at create, batch >= 2^31).
 *
 * Not part of the seam library (oracle/Makefile): there the reference's own softargmax stays on the CPU.
 */
#include <inttypes.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "upload.h"

static int launch_softargmax(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  /* reference operator-run.c:1091-1108 */
  const struct qnnp_hip_softargmax_args args = {
    .input = (const uint8_t*) input,
    .output = (uint8_t*) output,
    .table = (const uint32_t*) op->d_weights,
    .rows = (uint32_t) op->batch_size,
    .channels = (uint32_t) op->channels,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
  };
  return qnnp_hip_softargmax_run(&args, &op->kernel_name);
}

enum qnnp_status qnnp_create_softargmax_nc_q8(
    size_t channels,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint32_t flags,
    qnnp_operator_t* softargmax)
{
  (void) flags;
  /* reference softargmax.c:31-34 */
  const enum qnnp_status initialized = qnnp_check_initialized("qnnp_create_softargmax_nc_q8");
  if (initialized != qnnp_status_success) {
    return initialized;
  }
  /* reference softargmax.c:36-54: invalid_parameter */
  if (channels == 0) {
    qnnp_log_error("cannot create softargmax operator with %zu channels: number of channels must be non-zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if (input_scale <= 0.0f || !isnormal(input_scale)) {
    qnnp_log_error("cannot create softargmax operator with %.7g input scale: scale must be finite and positive", input_scale);
    return qnnp_status_invalid_parameter;
  }
  if (output_scale <= 0.0f || !isnormal(output_scale)) {
    qnnp_log_error("cannot create softargmax operator with %.7g output scale: scale must be finite and positive", output_scale);
    return qnnp_status_invalid_parameter;
  }
  /* reference softargmax.c:56-70: unsupported_parameter */
  if (output_scale != 0x1.0p-8f) {
    qnnp_log_error("cannot create softargmax operator with %.7g output scale: only output scale of 1/256 is supported",
        output_scale);
    return qnnp_status_unsupported_parameter;
  }
  if (output_zero_point != 0) {
    qnnp_log_error("cannot create softargmax operator with %" PRIu8 " output zero point: only output zero point of 0 is "
        "supported", output_zero_point);
    return qnnp_status_unsupported_parameter;
  }
  /* the product's own limit, as in lut.c */
  if (channels > (size_t) INT32_MAX) {
    qnnp_log_error("cannot create softargmax operator: %zu channels exceed the device kernel's index range", channels);
    return qnnp_status_unsupported_parameter;
  }

  /* reference softargmax.c:86-91 */
  uint32_t table[256];
  const double qscale = fmin(((double) UINT32_MAX) / (double) channels, 8388607.0);
  for (int32_t i = 0; i < 256; i++) {
    const double scaled_exp_xi = qscale * exp((double) (i - 255) * (double) input_scale);
    table[(uint32_t) i] = (uint32_t) lrint(scaled_exp_xi);
  }

  int token;
  enum qnnp_status status = qnnp_enter_for_update(qnnp_hip_device(), qnnp_status_unsupported_hardware, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  status = qnnp_status_out_of_memory;
  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_softargmax, launch_softargmax);
  if (op != NULL) {
    op->d_weights = qnnp_upload(table, sizeof(table));
    if (op->d_weights == NULL) {
      qnnp_log_error("failed to place the %zu-byte table of the softargmax operator on the device", sizeof(table));
      free(op);
    } else {
      op->channels = channels;
      op->input_scale = input_scale;
      *softargmax = op;
      status = qnnp_status_success;
    }
  }
  return qnnp_leave_create(token, status);
}

enum qnnp_status qnnp_setup_softargmax_nc_q8(
    qnnp_operator_t softargmax,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  int token;
  /* reference softargmax.c:114-117 */
  enum qnnp_status status = qnnp_enter_setup("qnnp_setup_softargmax_nc_q8", softargmax, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  /* reference softargmax.c:119-131 */
  status = softargmax->ukernel_type != qnnp_ukernel_type_softargmax ? qnnp_status_invalid_parameter :
      qnnp_setup_nc(softargmax, "qnnp_setup_softargmax_nc_q8", 1, batch_size, input, input_stride, output, output_stride);
  return qnnp_leave_setup(softargmax, token, status);
}
