/*
 * max-pooling.c -- qnnp_create_max_pooling2d_nhwc_u8 / qnnp_setup_max_pooling2d_nhwc_u8 for the gfx950 build.
 *
 * Replaces reference src/max-pooling.c:36-135 (create) and :137-223 (setup): same checks in the same order, same
 * status codes. The reference's indirection buffer (src/indirection.c:192-230) has no equivalent: the kernel
 * (hip/q8pool.hip) computes each window's clamped coordinates itself, so the operator owns no device state beyond the
 * host-pointer staging buffers.
 *
 * Where the reference checks nothing and would read out of range, this build answers instead:
 *   - invalid_parameter: NULL tensors, pixel strides below the channel count (as every other operator of this build),
 *     and a padded input smaller than the dilated window (the reference's output size then wraps around);
 *   - unsupported_parameter: tensors beyond the kernel's index range (padded extent >= 2^31, channels or the
 *     pixels of one output row times channels >= 2^31, batch * output height >= 2^32).
 *
 * Not part of the seam library (oracle/Makefile): there the reference's own max pooling stays on the CPU.
 */
#include <inttypes.h>
#include <stddef.h>
#include <stdint.h>

#include <qnnpack.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"

static int launch_max_pooling(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  /* reference operator-run.c:899-940 */
  const struct qnnp_hip_pool_args args = {
    .input = (const uint8_t*) input,
    .output = (uint8_t*) output,
    .batch = (uint32_t) op->batch_size,
    .input_height = (uint32_t) op->input_height,
    .input_width = (uint32_t) op->input_width,
    .output_height = (uint32_t) op->output_height,
    .output_width = (uint32_t) op->output_width,
    .channels = (uint32_t) op->channels,
    .kernel_height = op->kernel_height,
    .kernel_width = op->kernel_width,
    .stride_height = op->stride_height,
    .stride_width = op->stride_width,
    .dilation_height = op->dilation_height,
    .dilation_width = op->dilation_width,
    .pad_top = op->input_padding_top,
    .pad_left = op->input_padding_left,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
    .output_min = op->output_min,
    .output_max = op->output_max,
  };
  return qnnp_hip_maxpool_run(&args, &op->kernel_name);
}

static enum qnnp_status qnnp_create_max_pooling2d_nhwc_u8_impl(
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t pooling_height,
    uint32_t pooling_width,
    uint32_t stride_height,
    uint32_t stride_width,
    uint32_t dilation_height,
    uint32_t dilation_width,
    size_t channels,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* max_pooling_out)
{
  (void) flags;
  /* reference max-pooling.c:61-103 (the pooling size is a 32-bit product there too) */
  const uint32_t pooling_size = pooling_height * pooling_width;
  if (pooling_size == 0) {
    qnnp_log_error("cannot create max pooling operator with %" PRIu32 "x%" PRIu32 " pooling size: "
        "pooling size dimensions must be non-zero", pooling_width, pooling_height);
    return qnnp_status_invalid_parameter;
  }
  if (pooling_size == 1) {
    qnnp_log_error("cannot create max pooling operator with 1 pooling element: 1x1 pooling is meaningless");
    return qnnp_status_invalid_parameter;
  }
  if (stride_height == 0 || stride_width == 0) {
    qnnp_log_error("cannot create max pooling operator with %" PRIu32 "x%" PRIu32 " stride: "
        "stride dimensions must be non-zero", stride_width, stride_height);
    return qnnp_status_invalid_parameter;
  }
  if (dilation_height == 0 || dilation_width == 0) {
    qnnp_log_error("cannot create max pooling operator with %" PRIu32 "x%" PRIu32 " dilation: "
        "dilation dimensions must be non-zero", dilation_width, dilation_height);
    return qnnp_status_invalid_parameter;
  }
  if (channels == 0) {
    qnnp_log_error("cannot create max pooling operator with %zu channels: number of channels must be non-zero",
        channels);
    return qnnp_status_invalid_parameter;
  }
  if (channels > (size_t) INT32_MAX) {
    qnnp_log_error("cannot create max pooling operator: %zu channels exceed the device kernel's index range", channels);
    return qnnp_status_unsupported_parameter;
  }

  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_max_pooling, launch_max_pooling);
  if (op == NULL) {
    return qnnp_status_out_of_memory;
  }
  op->input_padding_top = input_padding_top;
  op->input_padding_right = input_padding_right;
  op->input_padding_bottom = input_padding_bottom;
  op->input_padding_left = input_padding_left;
  op->kernel_height = pooling_height;
  op->kernel_width = pooling_width;
  op->stride_height = stride_height;
  op->stride_width = stride_width;
  op->dilation_height = dilation_height;
  op->dilation_width = dilation_width;
  op->channels = channels;
  op->output_min = output_min;
  op->output_max = output_max;
  *max_pooling_out = op;
  return qnnp_status_success;
}

static enum qnnp_status qnnp_setup_max_pooling2d_nhwc_u8_impl(
    qnnp_operator_t op,
    size_t batch_size,
    size_t input_height,
    size_t input_width,
    const uint8_t* input,
    size_t input_pixel_stride,
    uint8_t* output,
    size_t output_pixel_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_max_pooling) {
    return qnnp_status_invalid_parameter;
  }
  /* reference max-pooling.c:153-156 */
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  /* reference max-pooling.c:158-163 */
  if (input_width == 0 || input_height == 0) {
    qnnp_log_error("cannot set up max pooling operator with %zux%zu input: input dimensions must be non-zero",
        input_width, input_height);
    return qnnp_status_invalid_parameter;
  }
  const size_t channels = op->channels;
  if (input == NULL || output == NULL || input_pixel_stride < channels || output_pixel_stride < channels) {
    qnnp_log_error("cannot set up max pooling operator: NULL tensor or pixel stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  /* reference max-pooling.c:171-180 computes (padded - effective window) / stride + 1 in size_t: a padded input
   * smaller than the dilated window wraps around there */
  const uint64_t padded_height = (uint64_t) op->input_padding_top + input_height + op->input_padding_bottom;
  const uint64_t padded_width = (uint64_t) op->input_padding_left + input_width + op->input_padding_right;
  const uint64_t window_height = (uint64_t) (op->kernel_height - 1) * op->dilation_height + 1;
  const uint64_t window_width = (uint64_t) (op->kernel_width - 1) * op->dilation_width + 1;
  if (padded_height < window_height || padded_width < window_width) {
    qnnp_log_error("cannot set up max pooling operator with %zux%zu input: the padded input is smaller than the "
        "%" PRIu64 "x%" PRIu64 " dilated pooling window", input_width, input_height, window_width, window_height);
    return qnnp_status_invalid_parameter;
  }
  const uint64_t output_height = (padded_height - window_height) / op->stride_height + 1;
  const uint64_t output_width = (padded_width - window_width) / op->stride_width + 1;
  if (padded_height > (uint64_t) INT32_MAX || padded_width > (uint64_t) INT32_MAX || batch_size > UINT32_MAX ||
      (uint64_t) batch_size * output_height > UINT32_MAX || output_width * channels > (uint64_t) INT32_MAX) {
    qnnp_log_error("cannot set up max pooling operator with %zu x %zux%zu input: outside the device kernel's index range",
        batch_size, input_width, input_height);
    return qnnp_status_unsupported_parameter;
  }

  op->setup_valid = 0;   /* until every check, allocation and upload below has succeeded */
  op->batch_size = batch_size;
  op->input_height = input_height;
  op->input_width = input_width;
  op->input = input;
  op->input_pixel_stride = input_pixel_stride;
  op->output_height = (size_t) output_height;
  op->output_width = (size_t) output_width;
  op->output = output;
  op->output_pixel_stride = output_pixel_stride;

  op->input_span = (batch_size * input_height * input_width - 1) * input_pixel_stride + channels;
  op->output_span = (batch_size * op->output_height * op->output_width - 1) * output_pixel_stride + channels;
  return qnnp_bind_tensors(op, "qnnp_setup_max_pooling2d_nhwc_u8");
}

/* ---- public entry points: the implementations above inside the device guards of lifecycle.h ---- */

enum qnnp_status qnnp_create_max_pooling2d_nhwc_u8(
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t pooling_height,
    uint32_t pooling_width,
    uint32_t stride_height,
    uint32_t stride_width,
    uint32_t dilation_height,
    uint32_t dilation_width,
    size_t channels,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* max_pooling)
{
  int token;
  const enum qnnp_status status = qnnp_enter_create("qnnp_create_max_pooling2d_nhwc_u8", &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token,
      qnnp_create_max_pooling2d_nhwc_u8_impl(input_padding_top, input_padding_right, input_padding_bottom,
          input_padding_left, pooling_height, pooling_width, stride_height, stride_width, dilation_height,
          dilation_width, channels, output_min, output_max, flags, max_pooling));
}

enum qnnp_status qnnp_setup_max_pooling2d_nhwc_u8(
    qnnp_operator_t max_pooling,
    size_t batch_size,
    size_t input_height,
    size_t input_width,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride,
    pthreadpool_t threadpool)
{
  (void) threadpool;
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_setup_max_pooling2d_nhwc_u8", max_pooling, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(max_pooling, token,
      qnnp_setup_max_pooling2d_nhwc_u8_impl(max_pooling, batch_size, input_height, input_width, input, input_stride,
          output, output_stride));
}
