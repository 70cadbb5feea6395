/*
 * softargmax.c -- qnnp_create_softargmax_nc_q8 / qnnp_setup_softargmax_nc_q8 for the gfx950 build.
 *
 * Replaces reference src/softargmax.c:20-104 (create) and :106-131 (setup): same checks in the same order, same status
 * codes, and the same table of 256 uint32_t -- the reference's double expressions restated term for term (fmin, exp,
 * lrint) and compiled by the same host compiler against the same libm, never on the device. The table is uploaded once
 * at create, to the create's device, and kept in op->d_weights (freed by qnnp_delete_operator); the run is the kernels
 * of hip/q8softargmax.hip, reached through op->launch_hook.
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
#include "log.h"
#include "operator.h"
#include "state.h"
#include "upload.h"

static int launch_softargmax(struct qnnp_operator* op, const void* input, void* output)
{
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
  if (!qnnp_state.initialized) {
    qnnp_log_error("qnnp_create_softargmax_nc_q8 called before qnnp_initialize succeeded");
    return qnnp_status_uninitialized;
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
  qnnp_operator_t op = calloc(1, sizeof(struct qnnp_operator));
  if (op == NULL) {
    qnnp_log_error("out of host memory: %zu bytes for qnnp_operator structure", sizeof(struct qnnp_operator));
  } else {
    op->device = qnnp_hip_device();   /* the context this create runs in */
    op->d_weights = qnnp_upload(table, sizeof(table));
    if (op->d_weights == NULL) {
      qnnp_log_error("failed to place the %zu-byte table of the softargmax operator on the device", sizeof(table));
      free(op);
    } else {
      op->channels = channels;
      op->input_scale = input_scale;
      op->ukernel_type = qnnp_ukernel_type_softargmax;
      op->launch_hook = launch_softargmax;
      *softargmax = op;
      status = qnnp_status_success;
    }
  }
  qnnp_hip_leave(token);
  return status;
}

static enum qnnp_status setup_softargmax(qnnp_operator_t op, size_t batch_size, const uint8_t* input, size_t input_stride,
                                         uint8_t* output, size_t output_stride)
{
  /* reference softargmax.c:119-122 */
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (input == NULL || output == NULL || input_stride < channels || output_stride < channels) {
    qnnp_log_error("qnnp_setup_softargmax_nc_q8: NULL tensor or row stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  if (batch_size > (size_t) INT32_MAX) {
    qnnp_log_error("qnnp_setup_softargmax_nc_q8 with batch %zu: outside the device kernel's index range", batch_size);
    return qnnp_status_unsupported_parameter;
  }
  const size_t input_span = (batch_size - 1) * input_stride + channels;
  const size_t output_span = (batch_size - 1) * output_stride + channels;
  const int in_place = (const void*) input == (const void*) output && input_stride == output_stride;
  if (!in_place && qnnp_spans_overlap(input, input_span, output, output_span)) {
    qnnp_log_error("qnnp_setup_softargmax_nc_q8: the input and output tensors overlap without being the same tensor");
    return qnnp_status_invalid_parameter;
  }

  op->setup_valid = 0;   /* until every check and allocation below has succeeded */
  op->batch_size = batch_size;
  op->input = input;
  op->input_pixel_stride = input_stride;
  op->output = output;
  op->output_pixel_stride = output_stride;
  op->input_span = input_span;
  op->output_span = output_span;
  enum qnnp_status bound = qnnp_bind_endpoint(input, op->input_span, &op->input_on_device, &op->d_stage_in, &op->stage_in_capacity);
  if (bound == qnnp_status_success) bound = qnnp_bind_endpoint(output, op->output_span, &op->output_on_device, &op->d_stage_out, &op->stage_out_capacity);
  if (bound != qnnp_status_success) {
    qnnp_log_error("qnnp_setup_softargmax_nc_q8: failed to bind the tensors: device staging for host memory could not be "
        "allocated, or a tensor lives on a different device than the operator");
  }
  return bound;
}

enum qnnp_status qnnp_setup_softargmax_nc_q8(
    qnnp_operator_t softargmax,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  if (!qnnp_state.initialized) {
    qnnp_log_error("qnnp_setup_softargmax_nc_q8 called before qnnp_initialize succeeded");
    return qnnp_status_uninitialized;
  }
  if (softargmax == NULL || softargmax->ukernel_type != qnnp_ukernel_type_softargmax) {
    return qnnp_status_invalid_parameter;
  }
  int token;
  enum qnnp_status status = qnnp_enter_for_update(softargmax->device, qnnp_status_invalid_parameter, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  status = setup_softargmax(softargmax, batch_size, input, input_stride, output, output_stride);
  /* a failed setup leaves the operator unrunnable instead of half updated (run answers invalid_parameter) */
  if (status == qnnp_status_success) {
    softargmax->setup_valid = 1;
  }
  qnnp_hip_leave(token);
  return status;
}
