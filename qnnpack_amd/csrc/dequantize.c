/*
 * dequantize.c -- qnnp_gfx950_create_dequantize_nc_q8_f32 and its two setups, qnnp_gfx950_setup_dequantize_nc_q8_f32
 * (rows) and qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32 (NHWC bytes in, planar float out): the uint8 -> float32 end of
 * a network (include/qnnpack_gfx950_float.h has the arithmetic and the statuses).
 *
 * No reference counterpart; the mirror of quantize.c. The float tensor is op->output: its byte span is 4 bytes per
 * element, and in the rows setup op->output_pixel_stride counts elements. In the planar setup the output is dense, and
 * op->output_pixel_stride is the channel count (what qnnp_run_operator takes for "no bytes between the elements" when it
 * stages a host tensor).
 *
 * Not part of the seam library (oracle/Makefile).
 */
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

static int launch_dequantize(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  const struct qnnp_hip_dequantize_args args = {
    .input = (const uint8_t*) input,
    .output = (float*) output,
    .planar = (uint32_t) op->f32_planar,
    .rows = (uint32_t) op->batch_size,
    .pixels = (uint32_t) op->f32_pixels,
    .channels = (uint32_t) op->channels,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
    .scale = op->input_scale,
    .zero_point = (int32_t) op->input_zero_point,
    .streaming_mode = op->streaming_mode,
  };
  return qnnp_hip_dequantize_run(&args, &op->kernel_name);
}

enum qnnp_status qnnp_gfx950_create_dequantize_nc_q8_f32(
    size_t channels,
    uint8_t input_zero_point,
    float input_scale,
    uint32_t flags,
    qnnp_operator_t* dequantize)
{
  (void) flags;
  enum qnnp_status status = qnnp_check_initialized("qnnp_gfx950_create_dequantize_nc_q8_f32");
  if (status != qnnp_status_success) {
    return status;
  }
  if (channels == 0) {
    qnnp_log_error("cannot create dequantize operator with %zu channels: number of channels may not be zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if (!(input_scale > 0.0f && isnormal(input_scale))) {
    qnnp_log_error("cannot create dequantize operator with %.7g input scale: a scale has to be a finite number above zero",
        input_scale);
    return qnnp_status_invalid_parameter;
  }
  if (channels > (size_t) INT32_MAX) {
    qnnp_log_error("cannot create dequantize operator: %zu channels exceed the device kernels' index range", channels);
    return qnnp_status_unsupported_parameter;
  }
  if (!(input_scale >= 0x1.0p-118f && input_scale <= 0x1.0p+118f)) {
    qnnp_log_error("cannot create dequantize operator with %.7g input scale: scale must be in [2**-118, 2**118] range",
        input_scale);
    return qnnp_status_unsupported_parameter;
  }

  int token;
  status = qnnp_enter_for_update(qnnp_hip_device(), qnnp_status_unsupported_hardware, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_dequantize, launch_dequantize);
  if (op == NULL) {
    status = qnnp_status_out_of_memory;
  } else {
    op->channels = channels;
    op->input_zero_point = input_zero_point;
    op->input_scale = input_scale;
    *dequantize = op;
  }
  return qnnp_leave_create(token, status);
}

/* what both setups store once every check has passed */
static enum qnnp_status bind_dequantize(
    qnnp_operator_t op, const char* what, int planar, size_t batch_size, size_t pixels, const uint8_t* input,
    size_t input_stride, size_t input_span, float* output, size_t output_stride, size_t output_span)
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

static enum qnnp_status setup_dequantize_nc(
    qnnp_operator_t op, size_t batch_size, const uint8_t* input, size_t input_stride, float* output, size_t output_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_dequantize) {
    return qnnp_status_invalid_parameter;
  }
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (input == NULL || output == NULL) {
    qnnp_log_error("cannot set up dequantize operator: NULL tensor");
    return qnnp_status_invalid_parameter;
  }
  if ((uintptr_t) output % sizeof(float) != 0) {
    qnnp_log_error("cannot set up dequantize operator: the float tensor is not 4-byte aligned");
    return qnnp_status_invalid_parameter;
  }
  if (input_stride < channels || output_stride < channels) {
    qnnp_log_error("cannot set up dequantize operator: row stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  if (batch_size > (size_t) INT32_MAX) {
    qnnp_log_error("cannot set up dequantize operator with batch %zu: outside the device kernels' index range", batch_size);
    return qnnp_status_unsupported_parameter;
  }
  const size_t input_span = (batch_size - 1) * input_stride + channels;
  const size_t output_span = ((batch_size - 1) * output_stride + channels) * sizeof(float);
  if (qnnp_spans_overlap(input, input_span, output, output_span)) {
    qnnp_log_error("cannot set up dequantize operator: the input and output tensors overlap");
    return qnnp_status_invalid_parameter;
  }
  return bind_dequantize(op, "qnnp_gfx950_setup_dequantize_nc_q8_f32", 0, batch_size, 0, input, input_stride, input_span,
      output, output_stride, output_span);
}

static enum qnnp_status setup_dequantize_planar(
    qnnp_operator_t op, size_t batch_size, size_t pixels, const uint8_t* input, size_t input_pixel_stride, float* output)
{
  if (op->ukernel_type != qnnp_ukernel_type_dequantize) {
    return qnnp_status_invalid_parameter;
  }
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (input == NULL || output == NULL) {
    qnnp_log_error("cannot set up dequantize operator: NULL tensor");
    return qnnp_status_invalid_parameter;
  }
  if (pixels == 0) {
    qnnp_log_error("cannot set up dequantize operator: number of pixels may not be zero");
    return qnnp_status_invalid_parameter;
  }
  if ((uintptr_t) output % sizeof(float) != 0) {
    qnnp_log_error("cannot set up dequantize operator: the float tensor is not 4-byte aligned");
    return qnnp_status_invalid_parameter;
  }
  if (input_pixel_stride < channels) {
    qnnp_log_error("cannot set up dequantize operator: pixel stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  /* each factor is checked first, so the products below cannot wrap */
  if (batch_size > (size_t) INT32_MAX || pixels > (size_t) INT32_MAX ||
      (uint64_t) batch_size * (uint64_t) pixels > (uint64_t) INT32_MAX ||
      (uint64_t) channels * (uint64_t) pixels > (uint64_t) INT32_MAX) {
    qnnp_log_error("cannot set up dequantize operator with batch %zu of %zu pixels x %zu channels: outside the device "
        "kernels' index range", batch_size, pixels, channels);
    return qnnp_status_unsupported_parameter;
  }
  const size_t input_span = (batch_size * pixels - 1) * input_pixel_stride + channels;
  const size_t output_span = batch_size * pixels * channels * sizeof(float);
  if (qnnp_spans_overlap(input, input_span, output, output_span)) {
    qnnp_log_error("cannot set up dequantize operator: the input and output tensors overlap");
    return qnnp_status_invalid_parameter;
  }
  return bind_dequantize(op, "qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32", 1, batch_size, pixels, input,
      input_pixel_stride, input_span, output, channels, output_span);
}

enum qnnp_status qnnp_gfx950_setup_dequantize_nc_q8_f32(
    qnnp_operator_t dequantize,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    float* output,
    size_t output_stride)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_gfx950_setup_dequantize_nc_q8_f32", dequantize, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(dequantize, token,
      setup_dequantize_nc(dequantize, batch_size, input, input_stride, output, output_stride));
}

enum qnnp_status qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(
    qnnp_operator_t dequantize,
    size_t batch_size,
    size_t pixels,
    const uint8_t* input,
    size_t input_pixel_stride,
    float* output)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32", dequantize, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(dequantize, token,
      setup_dequantize_planar(dequantize, batch_size, pixels, input, input_pixel_stride, output));
}
