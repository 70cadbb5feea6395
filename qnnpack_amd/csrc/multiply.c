/*
 * multiply.c -- qnnp_gfx950_create_multiply_nc_q8 / qnnp_gfx950_setup_multiply_nc_q8: the quantized product of two
 * tensors, element-wise or with the second operand broadcast over groups of rows (the x * s that ends a
 * squeeze-and-excite block: s has one row per image, x one row per pixel).
 *
 * No reference counterpart. The create is modelled on add.c (same validation order and status codes), the setup on
 * lut.c (every check comes before the operator changes, so a refused setup leaves the previous one runnable). The
 * arithmetic is the convolutions' own down-convert: acc = (a - a_zero_point) * (b - b_zero_point), requantized by
 * qnnp_q31_requantize with the scale a_scale * b_scale / product_scale (requantization.h builds the parameters,
 * hip/requant.hip.h consumes them). |acc| <= 255 * 255, which is the accumulator bound of ONE product and no bias.
 *
 * The kernels are hip/q8mul.hip, reached through op->launch; `b` is the operator's second input (op->input2, staged by
 * qnnp_run_operator when it is host memory), which the launch receives as `input2`.
 *
 * Not part of the seam library (oracle/Makefile).
 */
#include <inttypes.h>
#include <math.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "requantization.h"

static inline bool scale_is_valid(float scale)
{
  return scale > 0.0f && isnormal(scale);
}

static int launch_multiply(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  const struct qnnp_hip_mul_args args = {
    .a = (const uint8_t*) input,
    .b = (const uint8_t*) input2,
    .product = (uint8_t*) output,
    .b_rows = (uint32_t) op->mul_b_rows,
    .a_rows_per_b_row = (uint32_t) op->mul_a_rows_per_b_row,
    .channels = (uint32_t) op->channels,
    .a_stride = op->input_pixel_stride,
    .b_stride = op->input2_pixel_stride,
    .product_stride = op->output_pixel_stride,
    .a_zero_point = (int32_t) (uint32_t) op->mul_a_zero_point,
    .b_zero_point = (int32_t) (uint32_t) op->mul_b_zero_point,
    .rq = op->requant,
    .streaming_mode = op->streaming_mode,
  };
  return qnnp_hip_mul_run(&args, &op->kernel_name);
}

enum qnnp_status qnnp_gfx950_create_multiply_nc_q8(
    size_t channels,
    uint8_t a_zero_point,
    float a_scale,
    uint8_t b_zero_point,
    float b_scale,
    uint8_t product_zero_point,
    float product_scale,
    uint8_t product_min,
    uint8_t product_max,
    uint32_t flags,
    qnnp_operator_t* multiply)
{
  (void) flags;
  enum qnnp_status status = qnnp_check_initialized("qnnp_gfx950_create_multiply_nc_q8");
  if (status != qnnp_status_success) {
    return status;
  }
  if (channels == 0) {
    qnnp_log_error("cannot create multiply operator with %zu channels: number of channels may not be zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if (!scale_is_valid(a_scale)) {
    qnnp_log_error("cannot create multiply operator with %.7g A scale: a scale has to be a finite number above zero", a_scale);
    return qnnp_status_invalid_parameter;
  }
  if (!scale_is_valid(b_scale)) {
    qnnp_log_error("cannot create multiply operator with %.7g B scale: a scale has to be a finite number above zero", b_scale);
    return qnnp_status_invalid_parameter;
  }
  if (!scale_is_valid(product_scale)) {
    qnnp_log_error("cannot create multiply operator with %.7g output scale: a scale has to be a finite number above zero",
        product_scale);
    return qnnp_status_invalid_parameter;
  }
  if (product_min >= product_max) {
    qnnp_log_error("cannot create multiply operator with [%" PRIu8 ", %" PRIu8 "] output range: range min must be below "
        "range max", product_min, product_max);
    return qnnp_status_invalid_parameter;
  }
  if (channels > (size_t) INT32_MAX) {
    qnnp_log_error("cannot create multiply operator: %zu channels exceed the device kernels' index range", channels);
    return qnnp_status_unsupported_parameter;
  }
  /* float32, left to right: one rounding after the product, one after the quotient */
  const float ab_scale = a_scale * b_scale;
  const float ratio = ab_scale / product_scale;
  if (!(ratio >= 0x1.0p-32f && ratio < 1.0f)) {
    qnnp_log_error("cannot create multiply operator with %.7g scale ratio: a_scale * b_scale / product_scale must be in "
        "[2**-32, 1) range", ratio);
    return qnnp_status_unsupported_parameter;
  }

  int token;
  status = qnnp_enter_for_update(qnnp_hip_device(), qnnp_status_unsupported_hardware, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_multiply, launch_multiply);
  if (op == NULL) {
    status = qnnp_status_out_of_memory;
  } else {
    op->channels = channels;
    op->mul_a_zero_point = a_zero_point;
    op->mul_b_zero_point = b_zero_point;
    op->requant = qnnp_compute_requant(ratio, product_zero_point, product_min, product_max);
    /* one product, no bias: |acc| <= 65025 < 2^16 */
    op->requant.accumulator_bits = qnnp_accumulator_bits(NULL, 0, 1);
    *multiply = op;
  }
  return qnnp_leave_create(token, status);
}

static enum qnnp_status setup_multiply(
    qnnp_operator_t op, size_t b_rows, size_t a_rows_per_b_row, const uint8_t* a, size_t a_stride,
    const uint8_t* b, size_t b_stride, uint8_t* product, size_t product_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_multiply) {
    return qnnp_status_invalid_parameter;
  }
  if (b_rows == 0 || a_rows_per_b_row == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (a == NULL || b == NULL || product == NULL) {
    qnnp_log_error("cannot set up multiply operator: NULL tensor");
    return qnnp_status_invalid_parameter;
  }
  if (a_stride < channels || b_stride < channels || product_stride < channels) {
    qnnp_log_error("cannot set up multiply operator: row stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  /* each factor is checked first, so the product below cannot wrap */
  if (b_rows > (size_t) INT32_MAX || a_rows_per_b_row > (size_t) INT32_MAX ||
      (uint64_t) b_rows * (uint64_t) a_rows_per_b_row > (uint64_t) INT32_MAX) {
    qnnp_log_error("cannot set up multiply operator with %zu x %zu rows: outside the device kernels' index range",
        b_rows, a_rows_per_b_row);
    return qnnp_status_unsupported_parameter;
  }
  const size_t rows = b_rows * a_rows_per_b_row;
  const size_t a_span = (rows - 1) * a_stride + channels;
  const size_t b_span = (b_rows - 1) * b_stride + channels;
  const size_t product_span = (rows - 1) * product_stride + channels;
  /* a lane reads its own piece of a and of b before it writes that piece of the product: the product may BE a, and may
   * be b where b is not broadcast; a and b are only read and may overlap freely (a == b is the square) */
  const int on_a = (const void*) product == (const void*) a && product_stride == a_stride;
  const int on_b = (const void*) product == (const void*) b && product_stride == b_stride && a_rows_per_b_row == 1;
  if ((!on_a && qnnp_spans_overlap(a, a_span, product, product_span)) ||
      (!on_b && qnnp_spans_overlap(b, b_span, product, product_span))) {
    qnnp_log_error("cannot set up multiply operator: the product overlaps an input without being that tensor");
    return qnnp_status_invalid_parameter;
  }

  op->setup_valid = 0;   /* until every check and allocation below has succeeded */
  op->batch_size = rows;
  op->mul_b_rows = b_rows;
  op->mul_a_rows_per_b_row = a_rows_per_b_row;
  op->input = a;
  op->input_pixel_stride = a_stride;
  op->input2 = b;
  op->input2_pixel_stride = b_stride;
  op->output = product;
  op->output_pixel_stride = product_stride;
  op->input_span = a_span;
  op->input2_span = b_span;
  op->output_span = product_span;
  return qnnp_bind_tensors(op, "qnnp_gfx950_setup_multiply_nc_q8");
}

enum qnnp_status qnnp_gfx950_setup_multiply_nc_q8(
    qnnp_operator_t multiply,
    size_t b_rows,
    size_t a_rows_per_b_row,
    const uint8_t* a,
    size_t a_stride,
    const uint8_t* b,
    size_t b_stride,
    uint8_t* product,
    size_t product_stride)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_gfx950_setup_multiply_nc_q8", multiply, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(multiply, token,
      setup_multiply(multiply, b_rows, a_rows_per_b_row, a, a_stride, b, b_stride, product, product_stride));
}
