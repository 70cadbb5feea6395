/*
 * channel-shuffle.c -- qnnp_create_channel_shuffle_nc_x8 / qnnp_setup_channel_shuffle_nc_x8 for the gfx950 build.
 *
 * Replaces reference src/channel-shuffle.c:21-71 (create) and :73-98 (setup): same checks in the same order, same
 * status codes. The run is the kernel of hip/x8shuffle.hip, reached through op->launch_hook.
 *
 * Where the reference checks nothing and would go out of range, this build answers instead:
 *   - invalid_parameter: NULL tensors, pixel strides below groups * group_channels, and input and output byte spans
 *     that overlap (the reference's result then depends on the order inside its microkernel);
 *   - unsupported_parameter: sizes beyond the kernels' index range (groups * group_channels >= 2^31, batch >= 2^31).
 *
 * Not part of the seam library (oracle/Makefile): there the reference's own channel shuffle stays on the CPU.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"
#include "log.h"
#include "operator.h"
#include "state.h"

static int launch_channel_shuffle(struct qnnp_operator* op, const void* input, void* output)
{
  /* reference operator-run.c:1109-1147 */
  const struct qnnp_hip_x8_args args = {
    .input = (const uint8_t*) input,
    .output = (uint8_t*) output,
    .pixels = (uint32_t) op->batch_size,
    .groups = op->groups,
    .group_channels = (uint32_t) op->group_input_channels,
    .channels = (uint32_t) op->channels,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
  };
  return qnnp_hip_channel_shuffle_run(&args, &op->kernel_name);
}

static enum qnnp_status qnnp_create_channel_shuffle_nc_x8_impl(
    size_t groups,
    size_t group_channels,
    uint32_t flags,
    qnnp_operator_t* channel_shuffle_out)
{
  (void) flags;
  /* reference channel-shuffle.c:30-33 */
  if (!qnnp_state.initialized) {
    qnnp_log_error("qnnp_create_channel_shuffle_nc_x8 called before qnnp_initialize succeeded");
    return qnnp_status_uninitialized;
  }
  /* reference channel-shuffle.c:35-49 */
  if (groups <= 1) {
    qnnp_log_error("cannot create channel shuffle operator with %zu groups: at least two groups required", groups);
    return qnnp_status_invalid_parameter;
  }
  if (group_channels == 0) {
    qnnp_log_error("cannot create channel shuffle operator with %zu group channels: number of group channels must be "
        "non-zero", group_channels);
    return qnnp_status_invalid_parameter;
  }
  if (groups > (size_t) INT32_MAX || group_channels > (size_t) INT32_MAX / groups) {
    qnnp_log_error("cannot create channel shuffle operator: %zu groups of %zu channels exceed the device kernel's index "
        "range", groups, group_channels);
    return qnnp_status_unsupported_parameter;
  }

  qnnp_operator_t op = calloc(1, sizeof(struct qnnp_operator));
  if (op == NULL) {
    qnnp_log_error("out of host memory: %zu bytes for qnnp_operator structure", sizeof(struct qnnp_operator));
    return qnnp_status_out_of_memory;
  }
  op->device = qnnp_hip_device();   /* the context this create runs in (entry point below) */
  op->groups = (uint32_t) groups;
  op->group_input_channels = group_channels;
  op->group_output_channels = group_channels;
  op->channels = groups * group_channels;
  op->ukernel_type = qnnp_ukernel_type_channel_shuffle;
  op->launch_hook = launch_channel_shuffle;
  *channel_shuffle_out = op;
  return qnnp_status_success;
}

static enum qnnp_status qnnp_setup_channel_shuffle_nc_x8_impl(
    qnnp_operator_t op,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  /* reference channel-shuffle.c:81-84 */
  if (!qnnp_state.initialized) {
    qnnp_log_error("qnnp_setup_channel_shuffle_nc_x8 called before qnnp_initialize succeeded");
    return qnnp_status_uninitialized;
  }
  if (op == NULL || op->ukernel_type != qnnp_ukernel_type_channel_shuffle) {
    return qnnp_status_invalid_parameter;
  }
  /* reference channel-shuffle.c:86-89 */
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (input == NULL || output == NULL || input_stride < channels || output_stride < channels) {
    qnnp_log_error("cannot set up channel shuffle operator: NULL tensor or pixel stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  if (batch_size > (size_t) INT32_MAX) {
    qnnp_log_error("cannot set up channel shuffle operator with batch %zu: outside the device kernel's index range",
        batch_size);
    return qnnp_status_unsupported_parameter;
  }
  const size_t input_span = (batch_size - 1) * input_stride + channels;
  const size_t output_span = (batch_size - 1) * output_stride + channels;
  if (qnnp_spans_overlap(input, input_span, output, output_span)) {
    qnnp_log_error("cannot set up channel shuffle operator: the input and output tensors overlap");
    return qnnp_status_invalid_parameter;
  }

  op->setup_valid = 0;   /* until every check, allocation and upload below has succeeded */
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
    qnnp_log_error("failed to bind the tensors: device staging for host memory could not be allocated, or a tensor "
        "lives on a different device than the operator");
  }
  return bound;
}

/* ---- public entry points: run the implementation inside the right device context (as max-pooling.c) ---- */

enum qnnp_status qnnp_create_channel_shuffle_nc_x8(
    size_t groups,
    size_t group_channels,
    uint32_t flags,
    qnnp_operator_t* channel_shuffle)
{
  if (!qnnp_state.initialized) {
    /* logs and answers qnnp_status_uninitialized */
    return qnnp_create_channel_shuffle_nc_x8_impl(groups, group_channels, flags, channel_shuffle);
  }
  int token;
  enum qnnp_status status = qnnp_enter_for_update(qnnp_hip_device(), qnnp_status_unsupported_hardware, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  status = qnnp_create_channel_shuffle_nc_x8_impl(groups, group_channels, flags, channel_shuffle);
  qnnp_hip_leave(token);
  return status;
}

enum qnnp_status qnnp_setup_channel_shuffle_nc_x8(
    qnnp_operator_t channel_shuffle,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  if (!qnnp_state.initialized || channel_shuffle == NULL) {
    /* answers qnnp_status_uninitialized / invalid_parameter */
    return qnnp_setup_channel_shuffle_nc_x8_impl(channel_shuffle, batch_size, input, input_stride, output, output_stride);
  }
  int token;
  enum qnnp_status status = qnnp_enter_for_update(channel_shuffle->device, qnnp_status_invalid_parameter, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  status = qnnp_setup_channel_shuffle_nc_x8_impl(channel_shuffle, batch_size, input, input_stride, output, output_stride);
  /* a failed setup leaves the operator unrunnable instead of half updated (run answers invalid_parameter) */
  if (status == qnnp_status_success) {
    channel_shuffle->setup_valid = 1;
  }
  qnnp_hip_leave(token);
  return status;
}
