/*
 * global-average-pooling.c -- qnnp_create_global_average_pooling_nwc_q8 /
 * qnnp_setup_global_average_pooling_nwc_q8 for the gfx950 build (the pooling in
 * front of MobileNetV2's classifier).
 *
 * Replaces reference src/global-average-pooling.c:20-107 (create) and :109-148 (setup): same validation
 * order and status codes. The quantization parameters are the scalar member of
 * qnnp_compute_avgpool_quantization_params (reference src/qnnpack/requantization.h:200-222, :252-265; requantization.h),
 * recomputed at every setup from the pooled width exactly as the reference does (:138-145). The
 * reference's zero buffer (:79-85) has no equivalent: the device kernel never reads beyond `width` pixels.
 */
#include <math.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <qnnpack.h>

#include "gavgpool-params.h"
#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "requantization.h"

static inline bool scale_is_valid(float scale)
{
  return scale > 0.0f && isnormal(scale);
}

/* reference operator-run.c:981-1016 */
static int launch_global_average_pooling(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  const struct qnnp_hip_gavgpool_args args = {
    .input = (const uint8_t*) input,
    .output = (uint8_t*) output,
    .batch = op->batch_size,
    .width = op->input_width,
    .channels = (uint32_t) op->channels,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
    .params = op->avgpool_params,
  };
  return qnnp_hip_gavgpool_run(&args, &op->kernel_name);
}

static enum qnnp_status qnnp_create_global_average_pooling_nwc_q8_impl(
    size_t channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* global_average_pooling_out)
{
  (void) flags;
  /* reference global-average-pooling.c:39-59 */
  if (channels == 0) {
    qnnp_log_error("cannot create global average pooling operator with %zu channels: number of channels may not be zero",
        channels);
    return qnnp_status_invalid_parameter;
  }
  if (!scale_is_valid(input_scale)) {
    qnnp_log_error("cannot create global average pooling operator with %.7g input scale: a scale has to be a finite number above zero",
        input_scale);
    return qnnp_status_invalid_parameter;
  }
  if (!scale_is_valid(output_scale)) {
    qnnp_log_error("cannot create global average pooling operator with %.7g output scale: a scale has to be a finite number above zero",
        output_scale);
    return qnnp_status_invalid_parameter;
  }
  /* reference global-average-pooling.c:61-70 */
  const float input_output_scale = input_scale / output_scale;
  if (input_output_scale < 0x1.0p-8f || input_output_scale >= 0x1.0p+8f) {
    qnnp_log_error("cannot create global average pooling operator with %.7g input-to-output scale ratio: "
        "scale ratio must be in [2**-8, 2**8) range", input_output_scale);
    return qnnp_status_unsupported_parameter;
  }
  if (channels > (size_t) UINT32_MAX / 4) {
    qnnp_log_error("cannot create global average pooling operator: %zu channels exceed the device kernels' index range",
        channels);
    return qnnp_status_unsupported_parameter;
  }

  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_global_average_pooling, launch_global_average_pooling);
  if (op == NULL) {
    return qnnp_status_out_of_memory;
  }
  op->channels = channels;
  op->input_zero_point = input_zero_point;
  op->output_zero_point = output_zero_point;
  op->input_scale = input_scale;
  op->output_scale = output_scale;
  op->output_min = output_min;
  op->output_max = output_max;
  *global_average_pooling_out = op;
  return qnnp_status_success;
}

static enum qnnp_status qnnp_setup_global_average_pooling_nwc_q8_impl(
    qnnp_operator_t op,
    size_t batch_size,
    size_t width,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_global_average_pooling) {
    return qnnp_status_invalid_parameter;
  }
  /* reference global-average-pooling.c:123-126 */
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  /* reference global-average-pooling.c:128-131 */
  if (width == 0) {
    qnnp_log_error("cannot set up global average pooling operator with width %zu: width may not be zero", width);
    return qnnp_status_invalid_parameter;
  }
  const size_t channels = op->channels;
  if (input == NULL || output == NULL || input_stride < channels || output_stride < channels) {
    qnnp_log_error("cannot set up global average pooling operator: NULL tensor or stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  /* the width's range check and quantization parameters: gavgpool-params.h */
  struct qnnp_hip_avgpool_params params;
  if (!qnnp_gavgpool_params_for_width(op, width, &params)) {
    qnnp_log_error("cannot set up global average pooling operator with width %zu: outside the supported range", width);
    return qnnp_status_unsupported_parameter;
  }

  /* reference global-average-pooling.c:133-145 */
  op->setup_valid = 0;   /* until every check, allocation and upload below has succeeded */
  op->batch_size = batch_size;
  op->input_width = width;
  op->input = input;
  op->input_pixel_stride = input_stride;
  op->output = output;
  op->output_pixel_stride = output_stride;
  op->avgpool_params = params;

  op->input_span = (batch_size * width - 1) * input_stride + channels;
  op->output_span = (batch_size - 1) * output_stride + channels;
  return qnnp_bind_tensors(op, "qnnp_setup_global_average_pooling_nwc_q8");
}

/* ---- public entry points: the implementations above inside the device guards of lifecycle.h ---- */

enum qnnp_status qnnp_create_global_average_pooling_nwc_q8(
    size_t channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* global_average_pooling_out)
{
  int token;
  const enum qnnp_status status = qnnp_enter_create("qnnp_create_global_average_pooling_nwc_q8", &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token,
      qnnp_create_global_average_pooling_nwc_q8_impl(channels, input_zero_point, input_scale, output_zero_point,
          output_scale, output_min, output_max, flags, global_average_pooling_out));
}

enum qnnp_status qnnp_setup_global_average_pooling_nwc_q8(
    qnnp_operator_t op,
    size_t batch_size,
    size_t width,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_setup_global_average_pooling_nwc_q8", op, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(op, token,
      qnnp_setup_global_average_pooling_nwc_q8_impl(op, batch_size, width, input, input_stride, output,
          output_stride));
}
