/*
 * average-pooling.c -- qnnp_create_average_pooling2d_nhwc_q8 / qnnp_setup_average_pooling2d_nhwc_q8 for the gfx950
 * build.
 *
 * Replaces reference src/average-pooling.c:34-190 (create) and :192-275 (setup): same checks in the same order, same
 * status codes. The reference's zero buffer and indirection buffer (src/average-pooling.c:139-150,
 * src/indirection.c) have no equivalent: the kernel (hip/q8pool.hip) skips the taps in padding -- the reference
 * points them at the input zero point, which adds 0 to sum (x - izp) -- so the operator owns no device state beyond
 * the host-pointer staging buffers. The quantization parameters are those of the reference (:175-179, the scale over
 * the WHOLE window), built by qnnp_compute_avgpool_params (requantization.h) as for global average pooling. The
 * reference's SSE2 kernels clamp with min(., output_max) first and max(., output_min) last
 * (src/q8avgpool/up8x9-sse2.c:141-142), so with output_min > output_max every output is output_min: the parameters
 * carry max(output_min, output_max) as the upper bound to give the same bytes.
 *
 * Where the reference checks nothing and would read out of range, this build answers instead:
 *   - invalid_parameter: NULL tensors, pixel strides below the channel count (as every other operator of this build),
 *     and a padded input smaller than the window (the reference's output size then wraps around);
 *   - unsupported_parameter: tensors beyond the kernel's index range (padded extent >= 2^31, channels or the
 *     pixels of one output row times channels >= 2^31, batch * output height >= 2^32).
 *
 * Not part of the seam library (oracle/Makefile): there the reference's own average pooling stays on the CPU.
 */
#include <inttypes.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <qnnpack.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "requantization.h"

static int launch_average_pooling(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  /* reference operator-run.c:845-898 */
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
    .dilation_height = 1,
    .dilation_width = 1,
    .pad_top = op->input_padding_top,
    .pad_left = op->input_padding_left,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
    .input_zero_point = op->input_zero_point,
    .params = op->avgpool_params,
  };
  return qnnp_hip_avgpool_run(&args, &op->kernel_name);
}

static enum qnnp_status qnnp_create_average_pooling2d_nhwc_q8_impl(
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t pooling_height,
    uint32_t pooling_width,
    uint32_t stride_height,
    uint32_t stride_width,
    size_t channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* average_pooling_out)
{
  (void) flags;
  /* reference average-pooling.c:61-110 (the pooling size is a 32-bit product there too) */
  const uint32_t pooling_size = pooling_height * pooling_width;
  if (pooling_size == 0) {
    qnnp_log_error("cannot create average pooling operator with %" PRIu32 "x%" PRIu32 " pooling size: "
        "pooling size dimensions must be non-zero", pooling_width, pooling_height);
    return qnnp_status_invalid_parameter;
  }
  if (pooling_size == 1) {
    qnnp_log_error("cannot create average pooling operator with 1 pooling element: 1x1 pooling is meaningless");
    return qnnp_status_invalid_parameter;
  }
  if (stride_height == 0 || stride_width == 0) {
    qnnp_log_error("cannot create average pooling operator with %" PRIu32 "x%" PRIu32 " stride: "
        "stride dimensions must be non-zero", stride_width, stride_height);
    return qnnp_status_invalid_parameter;
  }
  if (channels == 0) {
    qnnp_log_error("cannot create average pooling operator with %zu channels: number of channels must be non-zero",
        channels);
    return qnnp_status_invalid_parameter;
  }
  if (!(input_scale > 0.0f) || !isnormal(input_scale)) {
    qnnp_log_error("cannot create average pooling operator with %.7g input scale: scale must be finite and positive",
        input_scale);
    return qnnp_status_invalid_parameter;
  }
  if (!(output_scale > 0.0f) || !isnormal(output_scale)) {
    qnnp_log_error("cannot create average pooling operator with %.7g output scale: scale must be finite and positive",
        output_scale);
    return qnnp_status_invalid_parameter;
  }
  /* reference average-pooling.c:112-129 */
  const float input_output_scale = input_scale / output_scale;
  if (input_output_scale < 0x1.0p-8f || input_output_scale >= 0x1.0p+8f) {
    qnnp_log_error("cannot create average pooling operator with %.7g input-to-output scale ratio: "
        "scale ratio must be in [2**-8, 2**8) range", input_output_scale);
    return qnnp_status_unsupported_parameter;
  }
  if (pooling_size >= UINT32_C(16777216)) {
    qnnp_log_error("cannot create average pooling operator with %" PRIu32 " pooling elements: "
        "the number of elements in the pooling area must be below 2**24", pooling_size);
    return qnnp_status_unsupported_parameter;
  }
  if (channels > (size_t) INT32_MAX) {
    qnnp_log_error("cannot create average pooling operator: %zu channels exceed the device kernel's index range", channels);
    return qnnp_status_unsupported_parameter;
  }

  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_average_pooling, launch_average_pooling);
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
  op->dilation_height = 1;
  op->dilation_width = 1;
  op->channels = channels;
  op->input_zero_point = input_zero_point;
  op->output_zero_point = output_zero_point;
  op->input_scale = input_scale;
  op->output_scale = output_scale;
  op->output_min = output_min;
  op->output_max = output_max;
  /* reference average-pooling.c:175-179; the bias is per output pixel here (its in-image taps), see the kernel */
  op->avgpool_params = qnnp_compute_avgpool_params(0, input_scale / (output_scale * (float) pooling_size),
      output_zero_point, output_min, output_max < output_min ? output_min : output_max);
  *average_pooling_out = op;
  return qnnp_status_success;
}

static enum qnnp_status qnnp_setup_average_pooling2d_nhwc_q8_impl(
    qnnp_operator_t op,
    size_t batch_size,
    size_t input_height,
    size_t input_width,
    const uint8_t* input,
    size_t input_pixel_stride,
    uint8_t* output,
    size_t output_pixel_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_average_pooling) {
    return qnnp_status_invalid_parameter;
  }
  /* reference average-pooling.c:208-211 */
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  /* reference average-pooling.c:213-218 */
  if (input_width == 0 || input_height == 0) {
    qnnp_log_error("cannot set up average pooling operator with %zux%zu input: input dimensions must be non-zero",
        input_width, input_height);
    return qnnp_status_invalid_parameter;
  }
  const size_t channels = op->channels;
  if (input == NULL || output == NULL || input_pixel_stride < channels || output_pixel_stride < channels) {
    qnnp_log_error("cannot set up average pooling operator: NULL tensor or pixel stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  /* reference average-pooling.c:226-233 computes (padded - window) / stride + 1 in size_t: a padded input smaller
   * than the window wraps around there */
  const uint64_t padded_height = (uint64_t) op->input_padding_top + input_height + op->input_padding_bottom;
  const uint64_t padded_width = (uint64_t) op->input_padding_left + input_width + op->input_padding_right;
  const uint64_t window_height = op->kernel_height;
  const uint64_t window_width = op->kernel_width;
  if (padded_height < window_height || padded_width < window_width) {
    qnnp_log_error("cannot set up average pooling operator with %zux%zu input: the padded input is smaller than the "
        "%" PRIu64 "x%" PRIu64 " pooling window", input_width, input_height, window_width, window_height);
    return qnnp_status_invalid_parameter;
  }
  const uint64_t output_height = (padded_height - window_height) / op->stride_height + 1;
  const uint64_t output_width = (padded_width - window_width) / op->stride_width + 1;
  if (padded_height > (uint64_t) INT32_MAX || padded_width > (uint64_t) INT32_MAX || batch_size > UINT32_MAX ||
      (uint64_t) batch_size * output_height > UINT32_MAX || output_width * channels > (uint64_t) INT32_MAX) {
    qnnp_log_error("cannot set up average pooling operator with %zu x %zux%zu input: outside the device kernel's index range",
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
  return qnnp_bind_tensors(op, "qnnp_setup_average_pooling2d_nhwc_q8");
}

/* ---- public entry points: the implementations above inside the device guards of lifecycle.h ---- */

enum qnnp_status qnnp_create_average_pooling2d_nhwc_q8(
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t pooling_height,
    uint32_t pooling_width,
    uint32_t stride_height,
    uint32_t stride_width,
    size_t channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* average_pooling)
{
  int token;
  const enum qnnp_status status = qnnp_enter_create("qnnp_create_average_pooling2d_nhwc_q8", &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token,
      qnnp_create_average_pooling2d_nhwc_q8_impl(input_padding_top, input_padding_right, input_padding_bottom,
          input_padding_left, pooling_height, pooling_width, stride_height, stride_width, channels, input_zero_point,
          input_scale, output_zero_point, output_scale, output_min, output_max, flags, average_pooling));
}

enum qnnp_status qnnp_setup_average_pooling2d_nhwc_q8(
    qnnp_operator_t average_pooling,
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
  const enum qnnp_status status = qnnp_enter_setup("qnnp_setup_average_pooling2d_nhwc_q8", average_pooling, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(average_pooling, token,
      qnnp_setup_average_pooling2d_nhwc_q8_impl(average_pooling, batch_size, input_height, input_width, input,
          input_stride, output, output_stride));
}
