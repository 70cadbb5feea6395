/*
 * add.c -- qnnp_create_add_nc_q8 / qnnp_setup_add_nc_q8 for the gfx950 build (SURVEY.md section 8f, row 4:
 * the residual add between MobileNetV2's convolutions).
 *
 * Replaces reference src/add.c:20-116 (create) and :118-149 (setup): same validation order and status
 * codes; the quantization parameters are the scalar member of qnnp_compute_add_quantization_params
 * (reference src/qnnpack/requantization.h:327-360, :400-413), built by qnnp_compute_add_params (requantization.h) and
 * consumed on the device by q8pointwise.hip. Where both scale ratios are below 2^-10 the reference's parameters are
 * undefined; here every output is then clamp(sum_zero_point), the correctly rounded sum (requantization.h).
 */
#include <math.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <qnnpack.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "requantization.h"

static inline bool scale_is_valid(float scale)
{
  return scale > 0.0f && isnormal(scale);
}

/* reference operator-run.c, case qnnp_ukernel_type_add (q8vadd over rows of `channels` bytes) */
static int launch_add(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  const struct qnnp_hip_vadd_args args = qnnp_vadd_args(op, input, op->input_pixel_stride, input2, op->input2_pixel_stride,
      output, op->output_pixel_stride, op->batch_size, op->channels, &op->add_params);
  return qnnp_hip_vadd_run(&args, &op->kernel_name);
}

static enum qnnp_status qnnp_create_add_nc_q8_impl(
    size_t channels,
    uint8_t a_zero_point,
    float a_scale,
    uint8_t b_zero_point,
    float b_scale,
    uint8_t sum_zero_point,
    float sum_scale,
    uint8_t sum_min,
    uint8_t sum_max,
    uint32_t flags,
    qnnp_operator_t* add_out)
{
  (void) flags;
  /* reference add.c:41-71 */
  if (channels == 0) {
    qnnp_log_error("cannot create add operator with %zu channels: number of channels may not be zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if (!scale_is_valid(a_scale)) {
    qnnp_log_error("cannot create add operator with %.7g A scale: a scale has to be a finite number above zero", a_scale);
    return qnnp_status_invalid_parameter;
  }
  if (!scale_is_valid(b_scale)) {
    qnnp_log_error("cannot create add operator with %.7g B scale: a scale has to be a finite number above zero", b_scale);
    return qnnp_status_invalid_parameter;
  }
  if (!scale_is_valid(sum_scale)) {
    qnnp_log_error("cannot create add operator with %.7g output scale: a scale has to be a finite number above zero", sum_scale);
    return qnnp_status_invalid_parameter;
  }
  if (sum_min >= sum_max) {
    qnnp_log_error("cannot create add operator with [%" PRIu8 ", %" PRIu8 "] output range: range min must be below range max",
        sum_min, sum_max);
    return qnnp_status_invalid_parameter;
  }
  if (channels > (size_t) UINT32_MAX / 4) {
    qnnp_log_error("cannot create add operator: %zu channels exceed the device kernels' index range", channels);
    return qnnp_status_unsupported_parameter;
  }
  /* reference add.c:73-89 */
  const float a_output_scale = a_scale / sum_scale;
  if (a_output_scale < 0x1.0p-14f || a_output_scale >= 0x1.0p+8f) {
    qnnp_log_error("cannot create add operator with %.7g A-to-output scale ratio: scale ratio must be in [2**-14, 2**8) range",
        a_output_scale);
    return qnnp_status_unsupported_parameter;
  }
  const float b_output_scale = b_scale / sum_scale;
  if (b_output_scale < 0x1.0p-14f || b_output_scale >= 0x1.0p+8f) {
    qnnp_log_error("cannot create add operator with %.7g B-to-output scale ratio: scale ratio must be in [2**-14, 2**8) range",
        b_output_scale);
    return qnnp_status_unsupported_parameter;
  }

  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_add, launch_add);
  if (op == NULL) {
    return qnnp_status_out_of_memory;
  }
  op->channels = channels;
  op->add_params = qnnp_compute_add_params(a_zero_point, b_zero_point, sum_zero_point,
      a_output_scale, b_output_scale, sum_min, sum_max);
  *add_out = op;
  return qnnp_status_success;
}

static enum qnnp_status qnnp_setup_add_nc_q8_impl(
    qnnp_operator_t op,
    size_t batch_size,
    const uint8_t* a,
    size_t a_stride,
    const uint8_t* b,
    size_t b_stride,
    uint8_t* sum,
    size_t sum_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_add) {
    return qnnp_status_invalid_parameter;
  }
  /* reference add.c:133-136 */
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (a == NULL || b == NULL || sum == NULL || a_stride < channels || b_stride < channels || sum_stride < channels) {
    qnnp_log_error("cannot set up add operator: NULL tensor or stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }

  /* reference add.c:138-146 */
  op->setup_valid = 0;   /* until every check, allocation and upload below has succeeded */
  op->batch_size = batch_size;
  op->input = a;
  op->input_pixel_stride = a_stride;
  op->input2 = b;
  op->input2_pixel_stride = b_stride;
  op->output = sum;
  op->output_pixel_stride = sum_stride;

  op->input_span = (batch_size - 1) * a_stride + channels;
  op->input2_span = (batch_size - 1) * b_stride + channels;
  op->output_span = (batch_size - 1) * sum_stride + channels;
  return qnnp_bind_tensors(op, "qnnp_setup_add_nc_q8");
}

/* ---- public entry points: the implementations above inside the device guards of lifecycle.h ---- */

enum qnnp_status qnnp_create_add_nc_q8(
    size_t channels,
    uint8_t a_zero_point,
    float a_scale,
    uint8_t b_zero_point,
    float b_scale,
    uint8_t sum_zero_point,
    float sum_scale,
    uint8_t sum_min,
    uint8_t sum_max,
    uint32_t flags,
    qnnp_operator_t* add_out)
{
  int token;
  const enum qnnp_status status = qnnp_enter_create("qnnp_create_add_nc_q8", &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token,
      qnnp_create_add_nc_q8_impl(channels, a_zero_point, a_scale, b_zero_point, b_scale, sum_zero_point, sum_scale,
          sum_min, sum_max, flags, add_out));
}

enum qnnp_status qnnp_setup_add_nc_q8(
    qnnp_operator_t op,
    size_t batch_size,
    const uint8_t* a,
    size_t a_stride,
    const uint8_t* b,
    size_t b_stride,
    uint8_t* sum,
    size_t sum_stride)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_setup_add_nc_q8", op, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(op, token,
      qnnp_setup_add_nc_q8_impl(op, batch_size, a, a_stride, b, b_stride, sum, sum_stride));
}
