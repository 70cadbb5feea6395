/*
 * lut.c -- the byte lookup-table operator: qnnp_gfx950_create_lut_nc_x8 / qnnp_gfx950_setup_lut_nc_x8, and the create
 * and setup that qnnp_*_sigmoid_nc_q8 (sigmoid.c) and qnnp_*_leaky_relu_nc_q8 (leaky-relu.c) end in.
 *
 * The reference has one operator type under sigmoid and leaky ReLU (qnnp_ukernel_type_lut: a 256-byte table made at
 * create, src/sigmoid.c:96-110, src/leaky-relu.c:104-117) and runs y[i] = table[x[i]] (src/operator-run.c:1017-1052).
 * Here the table is uploaded once at create, to the create's device, and kept in op->d_weights (freed by
 * qnnp_delete_operator); the run is the kernel of hip/x8lut.hip, reached through op->launch_hook.
 *
 * The reference's setups (sigmoid.c:125-150, leaky-relu.c:132-157) check nothing but the initialization. Where they
 * would go out of range, this build answers instead:
 *   - invalid_parameter: NULL tensors, pixel strides below the channel count, and input and output byte spans that
 *     overlap other than exactly in place (input == output with equal strides, which is supported, as the reference's
 *     byte-serial kernel supports it);
 *   - unsupported_parameter: sizes beyond the kernels' index range (channels >= 2^31, batch >= 2^31).
 *
 * Not part of the seam library (oracle/Makefile): there the reference's own sigmoid and leaky ReLU stay on the CPU.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"
#include "log.h"
#include "lut.h"
#include "operator.h"
#include "state.h"
#include "upload.h"

static int launch_lut(struct qnnp_operator* op, const void* input, void* output)
{
  /* reference operator-run.c:1017-1052 */
  const struct qnnp_hip_lut_args args = {
    .input = (const uint8_t*) input,
    .output = (uint8_t*) output,
    .table = (const uint8_t*) op->d_weights,
    .pixels = (uint32_t) op->batch_size,
    .channels = (uint32_t) op->channels,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
  };
  return qnnp_hip_lut_run(&args, &op->kernel_name);
}

enum qnnp_status qnnp_create_lut_operator(const char* what, size_t channels, const uint8_t table[256],
                                          qnnp_operator_t* lut_out)
{
  if (channels > (size_t) INT32_MAX) {
    qnnp_log_error("cannot create %s operator: %zu channels exceed the device kernel's index range", what, channels);
    return qnnp_status_unsupported_parameter;
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
    op->d_weights = qnnp_upload(table, 256);
    if (op->d_weights == NULL) {
      qnnp_log_error("failed to place the 256-byte table of the %s operator on the device", what);
      free(op);
    } else {
      op->channels = channels;
      op->ukernel_type = qnnp_ukernel_type_lut;
      op->launch_hook = launch_lut;
      *lut_out = op;
      status = qnnp_status_success;
    }
  }
  qnnp_hip_leave(token);
  return status;
}

static enum qnnp_status setup_lut(const char* what, qnnp_operator_t op, size_t batch_size, const uint8_t* input,
                                  size_t input_stride, uint8_t* output, size_t output_stride)
{
  /* reference sigmoid.c:138-141, leaky-relu.c:145-148 */
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (input == NULL || output == NULL || input_stride < channels || output_stride < channels) {
    qnnp_log_error("%s: NULL tensor or pixel stride smaller than the channel count", what);
    return qnnp_status_invalid_parameter;
  }
  if (batch_size > (size_t) INT32_MAX) {
    qnnp_log_error("%s with batch %zu: outside the device kernel's index range", what, batch_size);
    return qnnp_status_unsupported_parameter;
  }
  const size_t input_span = (batch_size - 1) * input_stride + channels;
  const size_t output_span = (batch_size - 1) * output_stride + channels;
  const int in_place = (const void*) input == (const void*) output && input_stride == output_stride;
  if (!in_place && qnnp_spans_overlap(input, input_span, output, output_span)) {
    qnnp_log_error("%s: the input and output tensors overlap without being the same tensor", what);
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
    qnnp_log_error("%s: failed to bind the tensors: device staging for host memory could not be allocated, or a tensor "
        "lives on a different device than the operator", what);
  }
  return bound;
}

enum qnnp_status qnnp_setup_lut_operator(const char* what, qnnp_operator_t lut, size_t batch_size, const uint8_t* input,
                                         size_t input_stride, uint8_t* output, size_t output_stride)
{
  if (!qnnp_state.initialized) {
    qnnp_log_error("%s called before qnnp_initialize succeeded", what);
    return qnnp_status_uninitialized;
  }
  if (lut == NULL || lut->ukernel_type != qnnp_ukernel_type_lut) {
    return qnnp_status_invalid_parameter;
  }
  int token;
  enum qnnp_status status = qnnp_enter_for_update(lut->device, qnnp_status_invalid_parameter, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  status = setup_lut(what, lut, batch_size, input, input_stride, output, output_stride);
  /* a failed setup leaves the operator unrunnable instead of half updated (run answers invalid_parameter) */
  if (status == qnnp_status_success) {
    lut->setup_valid = 1;
  }
  qnnp_hip_leave(token);
  return status;
}

/* ---- the generic operator: any 256-byte table ---- */

enum qnnp_status qnnp_gfx950_create_lut_nc_x8(size_t channels, const uint8_t table[256], uint32_t flags, qnnp_operator_t* lut)
{
  (void) flags;
  if (!qnnp_state.initialized) {
    qnnp_log_error("qnnp_gfx950_create_lut_nc_x8 called before qnnp_initialize succeeded");
    return qnnp_status_uninitialized;
  }
  if (channels == 0) {
    qnnp_log_error("cannot create lookup table operator with %zu channels: number of channels must be non-zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if (table == NULL) {
    qnnp_log_error("cannot create lookup table operator without a table");
    return qnnp_status_invalid_parameter;
  }
  return qnnp_create_lut_operator("lookup table", channels, table, lut);
}

enum qnnp_status qnnp_gfx950_setup_lut_nc_x8(qnnp_operator_t lut, size_t batch_size, const uint8_t* input,
                                             size_t input_stride, uint8_t* output, size_t output_stride)
{
  return qnnp_setup_lut_operator("qnnp_gfx950_setup_lut_nc_x8", lut, batch_size, input, input_stride, output, output_stride);
}
