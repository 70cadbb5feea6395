/*
 * channel-shuffle.c -- qnnp_create_channel_shuffle_nc_x8 / qnnp_setup_channel_shuffle_nc_x8 for the gfx950 build.
 *
 * Replaces reference src/channel-shuffle.c:21-71 (create) and :73-98 (setup): same checks in the same order, same
 * status codes. The run is the kernel of hip/x8shuffle.hip, reached through op->launch.
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

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"

static int launch_channel_shuffle(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
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

static enum qnnp_status create_channel_shuffle(size_t groups, size_t group_channels, qnnp_operator_t* channel_shuffle_out)
{
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

  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_channel_shuffle, launch_channel_shuffle);
  if (op == NULL) {
    return qnnp_status_out_of_memory;
  }
  op->groups = (uint32_t) groups;
  op->group_input_channels = group_channels;
  op->group_output_channels = group_channels;
  op->channels = groups * group_channels;
  *channel_shuffle_out = op;
  return qnnp_status_success;
}

enum qnnp_status qnnp_create_channel_shuffle_nc_x8(
    size_t groups,
    size_t group_channels,
    uint32_t flags,
    qnnp_operator_t* channel_shuffle)
{
  (void) flags;
  int token;
  /* reference channel-shuffle.c:30-33 */
  const enum qnnp_status status = qnnp_enter_create("qnnp_create_channel_shuffle_nc_x8", &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token, create_channel_shuffle(groups, group_channels, channel_shuffle));
}

enum qnnp_status qnnp_setup_channel_shuffle_nc_x8(
    qnnp_operator_t channel_shuffle,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  int token;
  /* reference channel-shuffle.c:81-84 */
  enum qnnp_status status = qnnp_enter_setup("qnnp_setup_channel_shuffle_nc_x8", channel_shuffle, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  /* reference channel-shuffle.c:86-98; no in-place form */
  status = channel_shuffle->ukernel_type != qnnp_ukernel_type_channel_shuffle ? qnnp_status_invalid_parameter :
      qnnp_setup_nc(channel_shuffle, "qnnp_setup_channel_shuffle_nc_x8", 0, batch_size, input, input_stride, output,
          output_stride);
  return qnnp_leave_setup(channel_shuffle, token, status);
}
