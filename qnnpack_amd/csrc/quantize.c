/*
 * quantize.c -- qnnp_gfx950_create_quantize_nc_f32_q8 and its two setups, qnnp_gfx950_setup_quantize_nc_f32_q8 (rows) and
 * qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8 (planar float in, NHWC bytes out): the float32 -> uint8 end of a network
 * (include/qnnpack_gfx950_float.h has the arithmetic and the statuses).
 *
 * No reference counterpart. Create and setup follow multiply.c: validation in the documented order, every setup check
 * before the operator changes, so a refused setup leaves the previous one runnable. The kernels are hip/f32q8.hip, reached
 * through op->launch. The float tensor is op->input: its byte span is 4 bytes per element, and in the rows setup
 * op->input_pixel_stride counts elements.
 *
 * Not part of the seam library (oracle/Makefile).
 */
#include <inttypes.h>
#include <math.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#include <qnnpack.h>
#include <qnnpack_gfx950_float.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"

static int launch_quantize(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  const struct qnnp_hip_quantize_args args = {
    .input = (const float*) input,
    .output = (uint8_t*) output,
    .planar = (uint32_t) op->f32_planar,
    .rows = (uint32_t) op->batch_size,
    .pixels = (uint32_t) op->f32_pixels,
    .channels = (uint32_t) op->channels,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
    .inv_scale = op->f32_inv_scale,
    .clamp_lo = (float) ((int32_t) op->output_min - (int32_t) op->output_zero_point),
    .clamp_hi = (float) ((int32_t) op->output_max - (int32_t) op->output_zero_point),
    .zero_point = (int32_t) op->output_zero_point,
    .streaming_mode = op->streaming_mode,
  };
  return qnnp_hip_quantize_run(&args, &op->kernel_name);
}

enum qnnp_status qnnp_gfx950_create_quantize_nc_f32_q8(
    size_t channels,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* quantize)
{
  (void) flags;
  enum qnnp_status status = qnnp_check_initialized("qnnp_gfx950_create_quantize_nc_f32_q8");
  if (status != qnnp_status_success) {
    return status;
  }
  if (channels == 0) {
    qnnp_log_error("cannot create quantize operator with %zu channels: number of channels may not be zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if (!(output_scale > 0.0f && isnormal(output_scale))) {
    qnnp_log_error("cannot create quantize operator with %.7g output scale: a scale has to be a finite number above zero",
        output_scale);
    return qnnp_status_invalid_parameter;
  }
  if (output_min >= output_max) {
    qnnp_log_error("cannot create quantize operator with [%" PRIu8 ", %" PRIu8 "] output range: range min must be below "
        "range max", output_min, output_max);
    return qnnp_status_invalid_parameter;
  }
  if (channels > (size_t) INT32_MAX) {
    qnnp_log_error("cannot create quantize operator: %zu channels exceed the device kernels' index range", channels);
    return qnnp_status_unsupported_parameter;
  }
  if (!(output_scale >= 0x1.0p-118f && output_scale <= 0x1.0p+118f)) {
    qnnp_log_error("cannot create quantize operator with %.7g output scale: scale must be in [2**-118, 2**118] range",
        output_scale);
    return qnnp_status_unsupported_parameter;
  }

  int token;
  status = qnnp_enter_for_update(qnnp_hip_device(), qnnp_status_unsupported_hardware, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_quantize, launch_quantize);
  if (op == NULL) {
    status = qnnp_status_out_of_memory;
  } else {
    op->channels = channels;
    op->output_zero_point = output_zero_point;
    op->output_scale = output_scale;
    op->output_min = output_min;
    op->output_max = output_max;
    op->f32_inv_scale = 1.0f / output_scale;   /* normal: the scale is within [2^-118, 2^118] */
    *quantize = op;
  }
  return qnnp_leave_create(token, status);
}

/* what both setups store once every check has passed */
static enum qnnp_status bind_quantize(
    qnnp_operator_t op, const char* what, int planar, size_t batch_size, size_t pixels, const float* input,
    size_t input_stride, size_t input_span, uint8_t* output, size_t output_stride, size_t output_span)
{
  op->setup_valid = 0;   /* until every allocation below has succeeded */
  op->batch_size = batch_size;
  op->f32_planar = planar;
  op->f32_pixels = pixels;
  op->input = input;
  op->input_pixel_stride = input_stride;
  op->output = output;
  op->output_pixel_stride = output_stride;
  op->input_span = input_span;
  op->output_span = output_span;
  return qnnp_bind_tensors(op, what);
}

static enum qnnp_status setup_quantize_nc(
    qnnp_operator_t op, size_t batch_size, const float* input, size_t input_stride, uint8_t* output, size_t output_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_quantize) {
    return qnnp_status_invalid_parameter;
  }
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (input == NULL || output == NULL) {
    qnnp_log_error("cannot set up quantize operator: NULL tensor");
    return qnnp_status_invalid_parameter;
  }
  if ((uintptr_t) input % sizeof(float) != 0) {
    qnnp_log_error("cannot set up quantize operator: the float tensor is not 4-byte aligned");
    return qnnp_status_invalid_parameter;
  }
  if (input_stride < channels || output_stride < channels) {
    qnnp_log_error("cannot set up quantize operator: row stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  if (batch_size > (size_t) INT32_MAX) {
    qnnp_log_error("cannot set up quantize operator with batch %zu: outside the device kernels' index range", batch_size);
    return qnnp_status_unsupported_parameter;
  }
  const size_t input_span = ((batch_size - 1) * input_stride + channels) * sizeof(float);
  const size_t output_span = (batch_size - 1) * output_stride + channels;
  if (qnnp_spans_overlap(input, input_span, output, output_span)) {
    qnnp_log_error("cannot set up quantize operator: the input and output tensors overlap");
    return qnnp_status_invalid_parameter;
  }
  return bind_quantize(op, "qnnp_gfx950_setup_quantize_nc_f32_q8", 0, batch_size, 0, input, input_stride, input_span,
      output, output_stride, output_span);
}

static enum qnnp_status setup_quantize_planar(
    qnnp_operator_t op, size_t batch_size, size_t pixels, const float* input, uint8_t* output, size_t output_pixel_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_quantize) {
    return qnnp_status_invalid_parameter;
  }
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (input == NULL || output == NULL) {
    qnnp_log_error("cannot set up quantize operator: NULL tensor");
    return qnnp_status_invalid_parameter;
  }
  if (pixels == 0) {
    qnnp_log_error("cannot set up quantize operator: number of pixels may not be zero");
    return qnnp_status_invalid_parameter;
  }
  if ((uintptr_t) input % sizeof(float) != 0) {
    qnnp_log_error("cannot set up quantize operator: the float tensor is not 4-byte aligned");
    return qnnp_status_invalid_parameter;
  }
  if (output_pixel_stride < channels) {
    qnnp_log_error("cannot set up quantize operator: pixel stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  /* each factor is checked first, so the products below cannot wrap */
  if (batch_size > (size_t) INT32_MAX || pixels > (size_t) INT32_MAX ||
      (uint64_t) batch_size * (uint64_t) pixels > (uint64_t) INT32_MAX ||
      (uint64_t) channels * (uint64_t) pixels > (uint64_t) INT32_MAX) {
    qnnp_log_error("cannot set up quantize operator with batch %zu of %zu pixels x %zu channels: outside the device "
        "kernels' index range", batch_size, pixels, channels);
    return qnnp_status_unsupported_parameter;
  }
  const size_t input_span = batch_size * pixels * channels * sizeof(float);
  const size_t output_span = (batch_size * pixels - 1) * output_pixel_stride + channels;
  if (qnnp_spans_overlap(input, input_span, output, output_span)) {
    qnnp_log_error("cannot set up quantize operator: the input and output tensors overlap");
    return qnnp_status_invalid_parameter;
  }
  return bind_quantize(op, "qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8", 1, batch_size, pixels, input, channels,
      input_span, output, output_pixel_stride, output_span);
}

enum qnnp_status qnnp_gfx950_setup_quantize_nc_f32_q8(
    qnnp_operator_t quantize,
    size_t batch_size,
    const float* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_gfx950_setup_quantize_nc_f32_q8", quantize, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(quantize, token,
      setup_quantize_nc(quantize, batch_size, input, input_stride, output, output_stride));
}

enum qnnp_status qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(
    qnnp_operator_t quantize,
    size_t batch_size,
    size_t pixels,
    const float* input,
    uint8_t* output,
    size_t output_pixel_stride)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8", quantize, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(quantize, token,
      setup_quantize_planar(quantize, batch_size, pixels, input, output, output_pixel_stride));
}
