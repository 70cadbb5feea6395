/*
 * fully-connected.c -- qnnp_create_fully_connected_nc_q8 / qnnp_setup_fully_connected_nc_q8.
 *
 * Replaces reference src/fully-connected.c:25-129 (create) and :131-161 (setup).
 * As there, a fully connected layer is a single-group GEMM operator whose rows
 * are the batch (setup maps batch -> rows, :149-158). The weights go to the
 * device as MFMA operand fragments (pack.h) instead of the 4x4c2 CPU panels of
 * pack_q8gemm_w (src/qnnpack/pack.h:12-49).
 */
#include <math.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <qnnpack.h>
#include <qnnpack_gfx950_perchannel.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "bias-pair.h"
#include "pack.h"
#include "per-channel.h"
#include "requantization.h"
#include "state.h"

static inline bool scale_is_valid(float scale)
{
  return scale > 0.0f && isnormal(scale);
}

/* kernel_scales == NULL: the per-tensor create with `kernel_scale`. Else the per-channel one: `per_channel` is set,
 * `kernel_scale` is unused and kernel_scales holds output_channels floats (convolution.c has the same pair). */
static enum qnnp_status qnnp_create_fully_connected_nc_q8_impl(
    int per_channel,
    const float* kernel_scales,
    size_t input_channels,
    size_t output_channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t kernel_zero_point,
    float kernel_scale,
    const uint8_t* kernel,
    const int32_t* bias,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected_out)
{
  (void) flags; /* ignored, reference fully-connected.c:38 */
  qnnp_operator_t op = NULL;
  int8_t* host_weights = NULL;
  int32_t* host_bias = NULL;

  /* reference fully-connected.c:49-67 (:44-47, the initialization, is the entry point's guard) */
  enum qnnp_status status = qnnp_status_invalid_parameter;
  if (!scale_is_valid(input_scale)) {
    qnnp_log_error("cannot create fully connected operator with %.7g input scale: a scale has to be a finite number above zero", input_scale);
    goto error;
  }
  if (per_channel ? kernel_scales == NULL : !scale_is_valid(kernel_scale)) {
    if (per_channel) {
      qnnp_log_error("cannot create fully connected operator: the array of kernel scales may not be NULL");
    } else {
      qnnp_log_error("cannot create fully connected operator with %.7g kernel scale: a scale has to be a finite number above zero", kernel_scale);
    }
    goto error;
  }
  if (!scale_is_valid(output_scale)) {
    qnnp_log_error("cannot create fully connected operator with %.7g output scale: a scale has to be a finite number above zero", output_scale);
    goto error;
  }
  if (input_channels == 0 || output_channels == 0 || kernel == NULL || bias == NULL) {
    qnnp_log_error("cannot create fully connected operator: channel counts, kernel and bias may not be zero");
    goto error;
  }
  if (per_channel) {
    const size_t bad = qnnp_per_channel_first_invalid(kernel_scales, output_channels);
    if (bad != output_channels) {
      qnnp_log_error("cannot create fully connected operator with %.7g kernel scale of channel %zu: a scale has to be a "
          "finite number above zero", kernel_scales[bad], bad);
      goto error;
    }
  }

  /* reference fully-connected.c:69-78 */
  status = qnnp_status_unsupported_parameter;
  float requantization_scale = 0.0f;
  if (per_channel) {
    const size_t bad = qnnp_per_channel_first_unsupported(input_scale, kernel_scales, output_scale, output_channels);
    if (bad != output_channels) {
      qnnp_log_error(
          "cannot create fully connected operator with %.7g input scale, %.7g kernel scale of channel %zu, and %.7g output "
          "scale: requantization scale %.7g is outside [2**-32, 1.0)",
          input_scale, kernel_scales[bad], bad, output_scale,
          qnnp_per_channel_scale(input_scale, kernel_scales[bad], output_scale));
      goto error;
    }
    /* (what op->requant carries beside the zero point and the clamp: the largest channel scale) */
    for (size_t c = 0; c < output_channels; c++) {
      const float scale = qnnp_per_channel_scale(input_scale, kernel_scales[c], output_scale);
      if (scale > requantization_scale) requantization_scale = scale;
    }
  } else {
    requantization_scale = input_scale * kernel_scale / output_scale;
  }
  if (requantization_scale >= 1.0f) {
    qnnp_log_error(
        "cannot create fully connected operator with %.7g input scale, %.7g kernel scale, and %.7g output scale: "
        "requantization scale %.7g is greater or equal to 1.0",
        input_scale, kernel_scale, output_scale, requantization_scale);
    goto error;
  }
  if (!(requantization_scale >= 0x1.0p-32f)) {
    qnnp_log_error("cannot create fully connected operator: requantization scale %.7g is below 2**-32", requantization_scale);
    goto error;
  }
  if (input_channels > (size_t) UINT32_MAX / 4 || output_channels > (size_t) UINT32_MAX / 4) {
    qnnp_log_error("cannot create fully connected operator: channel counts exceed the device kernels' 32-bit index range");
    goto error;
  }

  status = qnnp_status_out_of_memory;
  op = qnnp_allocate_operator(qnnp_ukernel_type_gemm, qnnp_igemm_launch);   /* convolution.c */
  if (op == NULL) {
    goto error;
  }

  const uint32_t n_pad = qnnp_round_up_u32((uint32_t) output_channels, 32);
  const uint32_t k_pad = qnnp_round_up_u32((uint32_t) input_channels, 64);
  const size_t w_bytes = qnnp_igemm_packed_weights_size(1, n_pad, k_pad);
  const size_t b_bytes = sizeof(int32_t) * n_pad;
  host_weights = (int8_t*) malloc(w_bytes);
  host_bias = (int32_t*) malloc(b_bytes);
  if (host_weights == NULL || host_bias == NULL) {
    qnnp_log_error("out of host memory: %zu bytes for packed weights", w_bytes + b_bytes);
    goto error;
  }
  qnnp_pack_igemm_w(1, (uint32_t) output_channels, (uint32_t) input_channels, n_pad, k_pad,
      input_zero_point, kernel_zero_point, kernel, bias, host_weights, host_bias);
  op->n_pad = n_pad;
  op->k_pad = k_pad;
  op->kc_slot = (uint32_t) input_channels;
  op->d_weights = qnnp_upload(host_weights, w_bytes);
  op->d_bias = qnnp_upload_bias_pair(host_bias, n_pad);      /* bias-pair.h */
  if (op->d_weights == NULL || op->d_bias == NULL) {
    qnnp_log_error("device allocation or upload failed: %zu bytes of packed weights on the device", w_bytes + 2 * b_bytes);
    goto error;
  }
  /* The big GEMM kernel's zero-point-centred image (pack.h, hip/q8gemm256c.hip): kernel zero point 128 IS the
   * standard image; 127 (the reference benchmarks' value, bench/q8gemm.cc:60-64) gets its own, for the shapes that
   * kernel takes (no K padding, channel blocks of 256, MFMA-bound sizes). */
  if (per_channel) {
    /* the per-channel flavour of the generic kernel reads the standard image and this table, nothing else */
    op->per_channel = 1;
    op->d_requant_pc = qnnp_per_channel_upload_table(1, output_channels, n_pad, input_scale, kernel_scales, output_scale);
    if (op->d_requant_pc == NULL) {
      goto error;
    }
  } else if (kernel_zero_point == 128) {
    op->centre_flip = 0x80;
  } else if (kernel_zero_point == 127 && k_pad == input_channels &&
             /* (the 256-wide tiling's shapes, or the 128-wide one's: hip/q8gemm128x.hip takes any K % 64 == 0) */
             ((n_pad % 256 == 0 && input_channels >= 512) || (input_channels % 64 == 0 && output_channels % 16 == 0))) {
    qnnp_pack_igemm_w_centred127((uint32_t) output_channels, (uint32_t) input_channels, (uint32_t) input_channels, n_pad,
        input_zero_point, kernel, bias, host_weights, host_bias);
    op->d_weights_centred = qnnp_upload(host_weights, w_bytes);
    op->d_bias_centred = qnnp_upload_bias_pair(host_bias, n_pad);
    if (op->d_weights_centred == NULL || op->d_bias_centred == NULL) {
      /* the centred image is an optimisation, not a requirement: without it the operator runs on the standard image
       * (the lean kernel with its row term) -- drop what was placed and carry on */
      qnnp_log_warning("no room for %zu bytes of centred weights on the device: the operator keeps the standard image", w_bytes + 2 * b_bytes);
      qnnp_hip_free(op->d_weights_centred);
      qnnp_hip_free(op->d_bias_centred);
      op->d_weights_centred = NULL;
      op->d_bias_centred = NULL;
    } else {
      op->centre_flip = 0x7F;
    }
  }
  free(host_weights);
  free(host_bias);
  host_weights = NULL;
  host_bias = NULL;

  /* reference fully-connected.c:109-121 */
  op->kernel_height = 1;
  op->kernel_width = 1;
  op->stride_height = 1;
  op->stride_width = 1;
  op->dilation_height = 1;
  op->dilation_width = 1;
  op->groups = 1;
  op->group_input_channels = input_channels;
  op->group_output_channels = output_channels;
  op->input_zero_point = input_zero_point;
  op->kernel_zero_point = kernel_zero_point;
  op->requant = qnnp_compute_requant(requantization_scale, output_zero_point, output_min, output_max);
  op->requant.accumulator_bits = qnnp_accumulator_bits(bias, output_channels, input_channels);

  *fully_connected_out = op;
  return qnnp_status_success;

error:
  free(host_weights);
  free(host_bias);
  qnnp_delete_operator(op);
  return status;
}

static enum qnnp_status qnnp_setup_fully_connected_nc_q8_impl(
    qnnp_operator_t op,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_gemm || op->transposed || op->group_input_channels == 0) {
    return qnnp_status_invalid_parameter;   /* not a handle from a fully connected / 1x1 create */
  }

  /* reference fully-connected.c:144-147 */
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  if (input == NULL || output == NULL ||
      input_stride < op->group_input_channels || output_stride < op->group_output_channels) {
    qnnp_log_error("cannot set up fully connected operator: NULL tensor or stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  if (batch_size > (size_t) UINT32_MAX / 2) {
    qnnp_log_error("cannot set up fully connected operator: batch %zu exceeds the device kernels' index range", batch_size);
    return qnnp_status_unsupported_parameter;
  }

  /* reference fully-connected.c:149-158: the batch becomes the row dimension */
  op->setup_valid = 0;   /* until every check, allocation and upload below has succeeded */
  op->residual = NULL;   /* an attached residual add belongs to the previous binding (residual.c), as in convolution.c */
  op->residual_folded = 0;
  op->batch_size = 1;
  op->input_height = batch_size;
  op->input_width = 1;
  op->input = input;
  op->input_pixel_stride = input_stride;
  op->output_height = batch_size;
  op->output_width = 1;
  op->output = output;
  op->output_pixel_stride = output_stride;

  op->input_span = (batch_size - 1) * input_stride + op->group_input_channels;
  op->output_span = (batch_size - 1) * output_stride + op->group_output_channels;
  const enum qnnp_status bound = qnnp_bind_tensors(op, "qnnp_setup_fully_connected_nc_q8");
  if (bound != qnnp_status_success) {
    return bound;
  }
  op->variant = qnnp_state.opt_gemm_kernel;
  return qnnp_status_success;
}

/* ---- public entry points: the implementations above inside the device guards of lifecycle.h ---- */

enum qnnp_status qnnp_create_fully_connected_nc_q8(
    size_t input_channels,
    size_t output_channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t kernel_zero_point,
    float kernel_scale,
    const uint8_t* kernel,
    const int32_t* bias,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected_out)
{
  int token;
  const enum qnnp_status status = qnnp_enter_create("qnnp_create_fully_connected_nc_q8", &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token,
      qnnp_create_fully_connected_nc_q8_impl(0, NULL, input_channels, output_channels, input_zero_point, input_scale,
          kernel_zero_point, kernel_scale, kernel, bias, output_zero_point, output_scale, output_min, output_max,
          flags, fully_connected_out));
}

enum qnnp_status qnnp_gfx950_create_fully_connected_nc_q8_per_channel(
    size_t input_channels,
    size_t output_channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t kernel_zero_point,
    const float* kernel_scales,
    const uint8_t* kernel,
    const int32_t* bias,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected_out)
{
  int token;
  const enum qnnp_status status = qnnp_enter_create("qnnp_gfx950_create_fully_connected_nc_q8_per_channel", &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token,
      qnnp_create_fully_connected_nc_q8_impl(1, kernel_scales, input_channels, output_channels, input_zero_point,
          input_scale, kernel_zero_point, 0.0f, kernel, bias, output_zero_point, output_scale, output_min, output_max,
          flags, fully_connected_out));
}

enum qnnp_status qnnp_setup_fully_connected_nc_q8(
    qnnp_operator_t op,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_setup_fully_connected_nc_q8", op, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(op, token,
      qnnp_setup_fully_connected_nc_q8_impl(op, batch_size, input, input_stride, output, output_stride));
}
