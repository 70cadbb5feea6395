/*
 * lut.c -- the byte lookup-table operator: qnnp_gfx950_create_lut_nc_x8 / qnnp_gfx950_setup_lut_nc_x8, and the create
 * and setup that qnnp_*_sigmoid_nc_q8 (sigmoid.c) and qnnp_*_leaky_relu_nc_q8 (leaky-relu.c) end in.
 *
 * The reference has one operator type under sigmoid and leaky ReLU (qnnp_ukernel_type_lut: a 256-byte table made at
 * create, src/sigmoid.c:96-110, src/leaky-relu.c:104-117) and runs y[i] = table[x[i]] (src/operator-run.c:1017-1052).
 * Here the table is uploaded once at create, to the create's device, and kept in op->d_weights (freed by
 * qnnp_delete_operator); the run is the kernel of hip/x8lut.hip, reached through op->launch.
 *
 * The reference's setups (sigmoid.c:125-150, leaky-relu.c:132-157) check nothing but the initialization. Where they
 * would go out of range, this build answers instead:
 *   - invalid_parameter: NULL tensors, pixel strides below the channel count, and input and output byte spans that
 *     overlap other than exactly in place (input == output with equal strides, which is supported, as the reference's
 *     byte-serial kernel supports it);
 *   - unsupported_parameter: sizes beyond the kernels' index range (channels >= 2^31, batch >= 2^31).
 *
 * Not part of the seam library (oracle/Makefile): there the reference's own sigmoid and leaky ReLU stay on the CPU.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "lut.h"
#include "operator.h"
#include "upload.h"

static int launch_lut(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  /* reference operator-run.c:1017-1052 */
  const struct qnnp_hip_lut_args args = {
    .input = (const uint8_t*) input,
    .output = (uint8_t*) output,
    .table = (const uint8_t*) op->d_weights,
    .pixels = (uint32_t) op->batch_size,
    .channels = (uint32_t) op->channels,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
  };
  return qnnp_hip_lut_run(&args, &op->kernel_name);
}

enum qnnp_status qnnp_create_lut_operator(const char* what, size_t channels, const uint8_t table[256],
                                          qnnp_operator_t* lut_out)
{
  if (channels > (size_t) INT32_MAX) {
    qnnp_log_error("cannot create %s operator: %zu channels exceed the device kernel's index range", what, channels);
    return qnnp_status_unsupported_parameter;
  }
  int token;
  enum qnnp_status status = qnnp_enter_for_update(qnnp_hip_device(), qnnp_status_unsupported_hardware, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  status = qnnp_status_out_of_memory;
  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_lut, launch_lut);
  if (op != NULL) {
    op->d_weights = qnnp_upload(table, 256);
    if (op->d_weights == NULL) {
      qnnp_log_error("failed to place the 256-byte table of the %s operator on the device", what);
      free(op);
    } else {
      op->channels = channels;
      *lut_out = op;
      status = qnnp_status_success;
    }
  }
  return qnnp_leave_create(token, status);
}

enum qnnp_status qnnp_setup_lut_operator(const char* what, qnnp_operator_t lut, size_t batch_size, const uint8_t* input,
                                         size_t input_stride, uint8_t* output, size_t output_stride)
{
  int token;
  /* reference sigmoid.c:133-136, leaky-relu.c:140-143 */
  enum qnnp_status status = qnnp_enter_setup(what, lut, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  /* reference sigmoid.c:138-150, leaky-relu.c:145-157 */
  status = lut->ukernel_type != qnnp_ukernel_type_lut ? qnnp_status_invalid_parameter :
      qnnp_setup_nc(lut, what, 1, batch_size, input, input_stride, output, output_stride);
  return qnnp_leave_setup(lut, token, status);
}

/* ---- the generic operator: any 256-byte table ---- */

enum qnnp_status qnnp_gfx950_create_lut_nc_x8(size_t channels, const uint8_t table[256], uint32_t flags, qnnp_operator_t* lut)
{
  (void) flags;
  const enum qnnp_status status = qnnp_check_initialized("qnnp_gfx950_create_lut_nc_x8");
  if (status != qnnp_status_success) {
    return status;
  }
  if (channels == 0) {
    qnnp_log_error("cannot create lookup table operator with %zu channels: number of channels must be non-zero", channels);
    return qnnp_status_invalid_parameter;
  }
  if (table == NULL) {
    qnnp_log_error("cannot create lookup table operator without a table");
    return qnnp_status_invalid_parameter;
  }
  return qnnp_create_lut_operator("lookup table", channels, table, lut);
}

enum qnnp_status qnnp_gfx950_setup_lut_nc_x8(qnnp_operator_t lut, size_t batch_size, const uint8_t* input,
                                             size_t input_stride, uint8_t* output, size_t output_stride)
{
  return qnnp_setup_lut_operator("qnnp_gfx950_setup_lut_nc_x8", lut, batch_size, input, input_stride, output, output_stride);
}
