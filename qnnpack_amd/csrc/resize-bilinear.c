/*
 * resize-bilinear.c -- qnnp_gfx950_create_resize_bilinear2d_nhwc_u8 / qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8: the
 * bilinear resize of a uint8 NHWC tensor to another height and width, quantization unchanged (the bilinear upsampling that
 * ends a segmentation head, the resize in front of a network's first convolution).
 *
 * No reference counterpart. The definition is integers only (include/qnnpack_gfx950.h, resize-table.h): setup builds one
 * table per axis on the host -- for every output row / column the two input rows / columns it blends and a Q11 weight --
 * and uploads both into ONE grow-only device allocation the operator owns (rows first, then columns; freed by
 * qnnp_delete_operator). The kernels are hip/u8resize.hip, reached through op->launch.
 *
 * Setup follows lut.c / multiply.c: every check comes before the operator changes, so a refused setup leaves the previous
 * one runnable. What can still fail afterwards is an allocation or a copy (the tables, the staging of host tensors); the
 * operator is then not runnable until the next successful setup.
 *
 * Not part of the seam library (oracle/Makefile).
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "resize-table.h"
#include "upload.h"

static int launch_resize(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  const struct qnnp_hip_resize_args args = {
    .input = (const uint8_t*) input,
    .output = (uint8_t*) output,
    .table = op->d_resize_table,
    .batch = (uint32_t) op->batch_size,
    .input_height = (uint32_t) op->input_height,
    .input_width = (uint32_t) op->input_width,
    .output_height = (uint32_t) op->output_height,
    .output_width = (uint32_t) op->output_width,
    .channels = (uint32_t) op->channels,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
    .streaming_mode = op->streaming_mode,
  };
  return qnnp_hip_resize_run(&args, &op->kernel_name);
}

enum qnnp_status qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(size_t channels, uint32_t flags, qnnp_operator_t* resize)
{
  enum qnnp_status status = qnnp_check_initialized("qnnp_gfx950_create_resize_bilinear2d_nhwc_u8");
  if (status != qnnp_status_success) {
    return status;
  }
  if (channels == 0) {
    qnnp_log_error("cannot create resize operator with %zu channels: number of channels may not be zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if ((flags & ~QNNP_GFX950_RESIZE_ALIGN_CORNERS) != 0) {
    qnnp_log_error("cannot create resize operator with flags 0x%08x: unknown flag bits", (unsigned) flags);
    return qnnp_status_invalid_parameter;
  }
  if (channels > (size_t) INT32_MAX) {
    qnnp_log_error("cannot create resize operator: %zu channels exceed the device kernels' index range", channels);
    return qnnp_status_unsupported_parameter;
  }

  int token;
  status = qnnp_enter_for_update(qnnp_hip_device(), qnnp_status_unsupported_hardware, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_resize_bilinear, launch_resize);
  if (op == NULL) {
    status = qnnp_status_out_of_memory;
  } else {
    op->channels = channels;
    op->resize_align_corners = (flags & QNNP_GFX950_RESIZE_ALIGN_CORNERS) != 0;
    *resize = op;
  }
  return qnnp_leave_create(token, status);
}

static enum qnnp_status setup_resize(
    qnnp_operator_t op, size_t batch_size, size_t input_height, size_t input_width, size_t output_height,
    size_t output_width, const uint8_t* input, size_t input_stride, uint8_t* output, size_t output_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_resize_bilinear) {
    return qnnp_status_invalid_parameter;
  }
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (input_height == 0 || input_width == 0 || output_height == 0 || output_width == 0) {
    qnnp_log_error("cannot set up resize operator with %zux%zu input and %zux%zu output: sizes may not be zero",
        input_height, input_width, output_height, output_width);
    return qnnp_status_invalid_parameter;
  }
  if (input == NULL || output == NULL) {
    qnnp_log_error("cannot set up resize operator: NULL tensor");
    return qnnp_status_invalid_parameter;
  }
  if (input_stride < channels || output_stride < channels) {
    qnnp_log_error("cannot set up resize operator: pixel stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  /* each factor is checked first, so the products below cannot wrap: sizes below 2^24, then batch against 2^31 */
  if (input_height >= QNNP_RESIZE_SIZE_LIMIT || input_width >= QNNP_RESIZE_SIZE_LIMIT ||
      output_height >= QNNP_RESIZE_SIZE_LIMIT || output_width >= QNNP_RESIZE_SIZE_LIMIT) {
    qnnp_log_error("cannot set up resize operator with %zux%zu input and %zux%zu output: sizes of 2^24 and more are not "
        "supported", input_height, input_width, output_height, output_width);
    return qnnp_status_unsupported_parameter;
  }
  const uint64_t input_image = (uint64_t) input_height * input_width, output_image = (uint64_t) output_height * output_width;
  if (batch_size > (size_t) INT32_MAX || (uint64_t) batch_size * input_image > (uint64_t) INT32_MAX ||
      (uint64_t) batch_size * output_image > (uint64_t) INT32_MAX) {
    qnnp_log_error("cannot set up resize operator with batch %zu of %zux%zu input and %zux%zu output: outside the device "
        "kernels' index range", batch_size, input_height, input_width, output_height, output_width);
    return qnnp_status_unsupported_parameter;
  }
  const size_t input_span = ((size_t) (batch_size * input_image) - 1) * input_stride + channels;
  const size_t output_span = ((size_t) (batch_size * output_image) - 1) * output_stride + channels;
  /* no in-place form: an output pixel reads up to four input pixels, which other lanes' stores could have hit */
  if (qnnp_spans_overlap(input, input_span, output, output_span)) {
    qnnp_log_error("cannot set up resize operator: the input and output tensors overlap");
    return qnnp_status_invalid_parameter;
  }
  if (qnnp_hip_is_device_pointer(input) < 0 || qnnp_hip_is_device_pointer(output) < 0) {
    qnnp_log_error("cannot set up resize operator: a tensor lives on a different device than the operator");
    return qnnp_status_invalid_parameter;
  }
  const size_t entries = output_height + output_width;
  struct qnnp_resize_entry* table = (struct qnnp_resize_entry*) malloc(entries * sizeof(struct qnnp_resize_entry));
  if (table == NULL) {
    qnnp_log_error("out of host memory: %zu bytes for the resize tables", entries * sizeof(struct qnnp_resize_entry));
    return qnnp_status_out_of_memory;
  }
  qnnp_resize_axis_table(input_height, output_height, op->resize_align_corners, table);
  qnnp_resize_axis_table(input_width, output_width, op->resize_align_corners, table + output_height);

  op->setup_valid = 0;   /* from here on the operator changes: until every allocation and copy below has succeeded */
  const int uploaded = qnnp_upload_table(&op->d_resize_table, &op->resize_table_capacity, entries,
      entries * sizeof(struct qnnp_resize_entry), table, entries * sizeof(struct qnnp_resize_entry));
  free(table);
  if (!uploaded) {
    qnnp_log_error("failed to place the resize tables (%zu entries) on the device", entries);
    return qnnp_status_out_of_memory;
  }
  op->batch_size = batch_size;
  op->input_height = input_height;
  op->input_width = input_width;
  op->output_height = output_height;
  op->output_width = output_width;
  op->input = input;
  op->input_pixel_stride = input_stride;
  op->output = output;
  op->output_pixel_stride = output_stride;
  op->input_span = input_span;
  op->output_span = output_span;
  return qnnp_bind_tensors(op, "qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8");
}

enum qnnp_status qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(
    qnnp_operator_t resize,
    size_t batch_size,
    size_t input_height,
    size_t input_width,
    size_t output_height,
    size_t output_width,
    const uint8_t* input,
    size_t input_pixel_stride,
    uint8_t* output,
    size_t output_pixel_stride)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8", resize, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(resize, token, setup_resize(resize, batch_size, input_height, input_width, output_height,
      output_width, input, input_pixel_stride, output, output_pixel_stride));
}
