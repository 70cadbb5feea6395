/*
 * deconvolution.c -- qnnp_create_deconvolution2d_nhwc_q8 / qnnp_setup_deconvolution2d_nhwc_q8
 * for the gfx950 build ("next" row 3).
 *
 * Replaces reference src/deconvolution.c:39-211 (create) and :213-277 (setup). A transposed convolution is
 * an implicit GEMM like any other once the (output pixel, tap) -> input pixel map is a table: output pixel
 * (oy, ox) takes tap (ky, kx) from input pixel ((oy + pad_top - ky*dil) / stride, ...) when the division is
 * exact and the pixel exists, and the input zero point otherwise (reference src/indirection.c:171-182). So
 *   create: the kernel arrives as [g][ic][ky][kx][oc] (reference pack.h:93-133 reads
 *           k[((ic * ks + ki) * n + oc]); it is transposed on the host to the convolution order
 *           [g][oc][ky][kx][ic] and goes through the SAME MFMA-fragment packer and bias folding as a
 *           convolution (pack.h; the reference's pack_q8deconv_w folds the bias exactly like pack_q8conv_w:
 *           b + ks*kc*izp*kzp - izp * sum(k), pack.h:105,123);
 *   setup : output extent per reference deconvolution.c:25-37; the batch-invariant int32 offset table of
 *           indirection.c (deconvolution flavour);
 *   run   : the generic offset-table MFMA implicit-GEMM kernel (q8igemm.hip) -- the geometry-derived
 *           convolution kernels do not apply, the operator pins "gemm_kernel" = 1.
 * STRIDED deconvolutions are split by output phase: all output pixels with the same
 * ((oy + pad_top) % stride_h, (ox + pad_left) % stride_w) see the same taps -- those with
 * ky*dil_h = phase_y (mod stride_h), likewise in x -- so each of the stride_h*stride_w phases is a dense
 * implicit GEMM over its own sub-kernel, offset table and output-pixel list (the kernel scatters GEMM rows
 * through that list). One table over all taps would spend (stride_h*stride_w - 1)/(stride_h*stride_w) of the
 * MFMA work and of the operand gathers on taps that are padding by construction (3/4 at stride 2).
 * Status codes and their order follow the reference (deconvolution.c:69-129, :225-243).
 */
#include <math.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>

#include "hip/qnnp_hip.h"
#include "indirection.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "bias-pair.h"
#include "pack.h"
#include "requantization.h"
#include "state.h"
#include "upload.h"

/* reference src/deconvolution.c:25-37 */
static inline size_t compute_output_dimension(
    size_t input, size_t padding, size_t adjustment, size_t kernel, size_t dilation, size_t stride)
{
  const size_t effective_kernel = (kernel - 1) * dilation + 1;
  return stride * (input - 1) + adjustment + effective_kernel - padding;
}

static inline bool scale_is_valid(float scale)
{
  return scale > 0.0f && isnormal(scale);
}

/* One packed sub-kernel per output phase (conv_order: the kernel in convolution order, [g][oc][tap][ic]). */
static enum qnnp_status pack_phases(struct qnnp_operator* op, const uint8_t* conv_order, const int32_t* bias)
{
  const uint32_t kh = op->kernel_height, kw = op->kernel_width, sh = op->stride_height, sw = op->stride_width;
  const size_t groups = op->groups, gic = op->group_input_channels, goc = op->group_output_channels;
  const size_t kernel_size = (size_t) kh * kw, group_weights = goc * kernel_size * gic;
  const size_t b_bytes = sizeof(int32_t) * groups * op->n_pad;
  uint8_t* sub = (uint8_t*) malloc(group_weights * groups + gic * goc * groups);
  int32_t* host_bias = (int32_t*) malloc(b_bytes);
  enum qnnp_status status = qnnp_status_out_of_memory;
  if (sub == NULL || host_bias == NULL) {
    qnnp_log_error("out of host memory: %zu bytes for the phase kernels", group_weights * groups);
    goto done;
  }
  for (uint32_t py = 0; py < sh; py++) {
    for (uint32_t px = 0; px < sw; px++) {
      struct qnnp_deconv_phase* ph = &op->phase[py * sw + px];
      uint32_t taps = 0;
      for (uint32_t ky = 0; ky < kh; ky++) {
        if ((ky * op->dilation_height) % sh != py) continue;
        for (uint32_t kx = 0; kx < kw; kx++) {
          if ((kx * op->dilation_width) % sw != px) continue;
          ph->tap_ky[taps] = (uint8_t) ky;
          ph->tap_kx[taps] = (uint8_t) kx;
          taps++;
        }
      }
      const int empty = taps == 0;
      if (empty) {
        /* no tap ever reaches this phase: one tap of weight == kernel zero point, always padding (255 = no tap) */
        ph->tap_ky[0] = ph->tap_kx[0] = 255;
        taps = 1;
      }
      ph->taps = taps;
      for (size_t g = 0; g < groups; g++) {
        for (size_t oc = 0; oc < goc; oc++) {
          for (uint32_t t = 0; t < taps; t++) {
            uint8_t* dst = sub + ((g * goc + oc) * taps + t) * gic;
            if (empty) {
              memset(dst, op->kernel_zero_point, gic);
            } else {
              const size_t tap = (size_t) ph->tap_ky[t] * kw + ph->tap_kx[t];
              memcpy(dst, conv_order + g * group_weights + (oc * kernel_size + tap) * gic, gic);
            }
          }
        }
      }
      ph->k_pad = qnnp_round_up_u32(taps * op->kc_slot, 64);
      const size_t w_bytes = qnnp_igemm_packed_weights_size((uint32_t) groups, op->n_pad, ph->k_pad);
      int8_t* packed = (int8_t*) malloc(w_bytes);
      if (packed != NULL) {
        qnnp_pack_igemm_w_slots((uint32_t) groups, (uint32_t) goc, taps, (uint32_t) gic, op->kc_slot, op->n_pad, ph->k_pad,
            op->input_zero_point, op->kernel_zero_point, sub, bias, packed, host_bias);
        ph->d_weights = qnnp_upload(packed, w_bytes);
        ph->d_bias = qnnp_upload_bias_pair(host_bias, groups * op->n_pad);   /* bias-pair.h */
        free(packed);
      }
      op->deconv_phases = py * sw + px + 1;   /* so that delete frees what exists so far */
      if (ph->d_weights == NULL || ph->d_bias == NULL) {
        qnnp_log_error("device allocation or upload failed: %zu bytes of packed phase weights on the device", w_bytes + b_bytes);
        goto done;
      }
    }
  }
  status = qnnp_status_success;
done:
  free(sub);
  free(host_bias);
  return status;
}

/* Kernel == stride (the usual 2x upsampling): every output pixel has exactly one tap and every input pixel
 * feeds stride_h*stride_w output pixels, so the whole operator is ONE pointwise GEMM over the input pixels with
 * phases * n_pad columns (phase-major) whose 32-channel blocks are stored depth-to-space (q8pwstream.hip).
 * Packed beside the phase kernels; the run falls back to those if the streaming kernel cannot take the tensors. */
static enum qnnp_status pack_depth_to_space(struct qnnp_operator* op, const uint8_t* conv_order, const int32_t* bias)
{
  const uint32_t phases = op->stride_height * op->stride_width, n_pad = op->n_pad;
  const size_t gic = op->group_input_channels, goc = op->group_output_channels;
  const size_t kernel_size = (size_t) op->kernel_height * op->kernel_width;
  const uint32_t d2s_cols = phases * n_pad;
  const uint32_t d2s_k_pad = qnnp_round_up_u32((uint32_t) gic, 64);
  const bool any_padding =
      (op->input_padding_top | op->input_padding_right | op->input_padding_bottom | op->input_padding_left) != 0;
  if (!(op->groups == 1 && op->kernel_height == op->stride_height && op->kernel_width == op->stride_width &&
        op->dilation_height == 1 && op->dilation_width == 1 && !any_padding &&
        op->adjustment_height == 0 && op->adjustment_width == 0 && gic <= 256 && gic % 16 == 0 &&
        (size_t) d2s_cols * ((gic + 31) / 32 * 32) + (size_t) d2s_cols * 4 + 1024 <= 64 * 1024)) {
    return qnnp_status_success;   /* the phase kernels only */
  }
  uint8_t* mat = (uint8_t*) malloc((size_t) d2s_cols * gic);
  int32_t* cols_bias = (int32_t*) calloc(d2s_cols, sizeof(int32_t));
  const size_t dw_bytes = qnnp_igemm_packed_weights_size(1, d2s_cols, d2s_k_pad);
  const size_t db_bytes = sizeof(int32_t) * d2s_cols;
  int8_t* packed = (int8_t*) malloc(dw_bytes);
  int32_t* packed_bias = (int32_t*) malloc(db_bytes);
  if (mat != NULL && cols_bias != NULL && packed != NULL && packed_bias != NULL) {
    memset(mat, op->kernel_zero_point, (size_t) d2s_cols * gic);     /* padding columns: w - kzp == 0 */
    for (uint32_t ph = 0; ph < phases; ph++) {
      const size_t tap = (size_t) (ph / op->stride_width) * op->kernel_width + ph % op->stride_width;   /* (ky, kx) = (py, px) */
      for (size_t oc = 0; oc < goc; oc++) {
        memcpy(mat + ((size_t) ph * n_pad + oc) * gic, conv_order + (oc * kernel_size + tap) * gic, gic);
        cols_bias[(size_t) ph * n_pad + oc] = bias[oc];
      }
    }
    qnnp_pack_igemm_w_slots(1, d2s_cols, 1, (uint32_t) gic, op->kc_slot, d2s_cols, d2s_k_pad,
        op->input_zero_point, op->kernel_zero_point, mat, cols_bias, packed, packed_bias);
    op->d_weights = qnnp_upload(packed, dw_bytes);
    op->d_bias = qnnp_upload_bias_pair(packed_bias, d2s_cols);   /* bias-pair.h */
  }
  free(mat);
  free(cols_bias);
  free(packed);
  free(packed_bias);
  if (op->d_weights == NULL || op->d_bias == NULL) {
    qnnp_log_error("device allocation or upload failed: %zu bytes of packed depth-to-space weights on the device", dw_bytes + db_bytes);
    return qnnp_status_out_of_memory;
  }
  op->k_pad = d2s_k_pad;
  op->deconv_d2s = 1;
  return qnnp_status_success;
}

/* stride 1, or too many phases / taps to split: one packed kernel over all taps */
static enum qnnp_status pack_whole(struct qnnp_operator* op, const uint8_t* conv_order, const int32_t* bias)
{
  const uint32_t groups = op->groups;
  const size_t kernel_size = (size_t) op->kernel_height * op->kernel_width;
  const uint32_t k_pad = qnnp_round_up_u32((uint32_t) (kernel_size * op->kc_slot), 64);
  const size_t w_bytes = qnnp_igemm_packed_weights_size(groups, op->n_pad, k_pad);
  const size_t b_bytes = sizeof(int32_t) * (size_t) groups * op->n_pad;
  int8_t* host_weights = (int8_t*) malloc(w_bytes);
  int32_t* host_bias = (int32_t*) malloc(b_bytes);
  if (host_weights == NULL || host_bias == NULL) {
    free(host_weights);
    free(host_bias);
    qnnp_log_error("out of host memory: %zu bytes for packed weights", w_bytes + b_bytes);
    return qnnp_status_out_of_memory;
  }
  qnnp_pack_igemm_w_slots(groups, (uint32_t) op->group_output_channels, (uint32_t) kernel_size,
      (uint32_t) op->group_input_channels, op->kc_slot, op->n_pad, k_pad, op->input_zero_point, op->kernel_zero_point,
      conv_order, bias, host_weights, host_bias);
  op->k_pad = k_pad;
  op->d_weights = qnnp_upload(host_weights, w_bytes);
  op->d_bias = qnnp_upload_bias_pair(host_bias, (size_t) groups * op->n_pad);   /* bias-pair.h */
  free(host_weights);
  free(host_bias);
  if (op->d_weights == NULL || op->d_bias == NULL) {
    qnnp_log_error("device allocation or upload failed: %zu bytes of packed weights on the device", w_bytes + b_bytes);
    return qnnp_status_out_of_memory;
  }
  return qnnp_status_success;
}

/* The device images: the kernel in convolution order goes through the packer of the phase kernels (+ the depth-to-space
 * GEMM) of a strided deconvolution, else through the one of a single kernel over all taps. */
static enum qnnp_status pack_deconvolution(struct qnnp_operator* op, const uint8_t* kernel, const int32_t* bias)
{
  const size_t groups = op->groups, kernel_size = (size_t) op->kernel_height * op->kernel_width;
  /* [g][ic][tap][oc] -> [g][oc][tap][ic] */
  const size_t gic = op->group_input_channels, goc = op->group_output_channels;
  const size_t group_weights = goc * kernel_size * gic;
  uint8_t* conv_order = (uint8_t*) malloc(group_weights * groups);
  if (conv_order == NULL) {
    qnnp_log_error("out of host memory: %zu bytes for the transposed kernel", group_weights * groups);
    return qnnp_status_out_of_memory;
  }
  for (size_t g = 0; g < groups; g++) {
    for (size_t ic = 0; ic < gic; ic++) {
      for (size_t tap = 0; tap < kernel_size; tap++) {
        const uint8_t* row = kernel + g * group_weights + (ic * kernel_size + tap) * goc;
        for (size_t oc = 0; oc < goc; oc++) {
          conv_order[g * group_weights + (oc * kernel_size + tap) * gic + ic] = row[oc];
        }
      }
    }
  }
  op->kc_slot = (uint32_t) gic;
  op->n_pad = qnnp_round_up_u32((uint32_t) goc, 32);
  const uint32_t phases = op->stride_height * op->stride_width;
  enum qnnp_status status;
  if (phases > 1 && phases <= QNNP_MAX_DECONV_PHASES && kernel_size <= 64) {
    status = pack_phases(op, conv_order, bias);
    if (status == qnnp_status_success) {
      status = pack_depth_to_space(op, conv_order, bias);
    }
  } else {
    status = pack_whole(op, conv_order, bias);
  }
  free(conv_order);
  return status;
}

/* The launch: the depth-to-space GEMM where the create packed one, then the stride-2 streaming kernel, then the phase
 * GEMMs, each falling through to the next when the kernel answers that it cannot take these tensors (QNNP_HIP_EINVAL:
 * alignment is part of the choice, so it is made per launch); the one-table form runs like a convolution. */
static int launch_deconvolution(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  if (op->deconv_d2s) {
    /* kernel == stride: one pointwise GEMM over the input pixels, stored depth-to-space (pack_depth_to_space) */
    struct qnnp_hip_igemm_args dargs = qnnp_igemm_args(op, input, output);
    dargs.packed_w = (const int8_t*) op->d_weights;
    dargs.bias2 = op->d_bias;
    dargs.bias2_pair = 1;
    dargs.rows = (uint32_t) (op->batch_size * op->input_height * op->input_width);
    dargs.rows_per_image = (uint32_t) (op->input_height * op->input_width);
    dargs.image_stride = 0;
    dargs.groups = 1;
    dargs.n_pad = op->n_pad * op->stride_height * op->stride_width;
    dargs.k_pad = op->k_pad;
    dargs.variant = 5;
    dargs.d2s_stride_h = op->stride_height;
    dargs.d2s_stride_w = op->stride_width;
    dargs.d2s_input_h = (uint32_t) op->input_height;
    dargs.d2s_input_w = (uint32_t) op->input_width;
    const int rc_d2s = qnnp_hip_igemm_run(&dargs, &op->kernel_name);
    if (rc_d2s != QNNP_HIP_EINVAL) {
      return rc_d2s;
    }
    /* the streaming kernel cannot take these tensors (alignment): the phase GEMMs below can */
  }
  if (op->deconv_phases == 4 && op->deconv_stream != 1 && op->groups == 1 &&
      op->stride_height == 2 && op->stride_width == 2 && op->dilation_height == 1 && op->dilation_width == 1 &&
      op->kernel_height == op->kernel_width && (op->kernel_height == 3 || op->kernel_height == 4)) {
    /* stride 2, 3x3 / 4x4: one streaming kernel over the input pixels, all four phases (q8deconv.hip) */
    struct qnnp_hip_deconv_s2_args sargs = {
      .input = (const uint8_t*) input,
      .output = (uint8_t*) output,
      .batch = (uint32_t) op->batch_size,
      .input_height = (uint32_t) op->input_height,
      .input_width = (uint32_t) op->input_width,
      .output_height = (uint32_t) op->output_height,
      .output_width = (uint32_t) op->output_width,
      .kernel_height = op->kernel_height,
      .kernel_width = op->kernel_width,
      .pad_top = op->input_padding_top,
      .pad_left = op->input_padding_left,
      .channels = (uint32_t) op->group_input_channels,
      .n = (uint32_t) op->group_output_channels,
      .n_pad = op->n_pad,
      .input_stride = (uint32_t) op->input_pixel_stride,
      .output_stride = (uint32_t) op->output_pixel_stride,
      .row_coeff = 128 - (int32_t) op->kernel_zero_point,
      .input_zero_point = op->input_zero_point,
      .rq = op->requant,
      .bias2_pair = 1,
    };
    for (int ph = 0; ph < 4; ph++) {
      sargs.packed_w[ph] = (const int8_t*) op->phase[ph].d_weights;
      sargs.bias2[ph] = op->phase[ph].d_bias;
      sargs.k_pad[ph] = op->phase[ph].k_pad;
    }
    const int rc_s2 = qnnp_hip_deconv_s2_run(&sargs, &op->kernel_name);
    if (rc_s2 != QNNP_HIP_EINVAL || op->deconv_stream == 2) {
      return rc_s2;
    }
    /* outside the streaming kernel's range (channel multiple, LDS, alignment): the phase GEMMs below */
  } else if (op->deconv_stream == 2) {
    return QNNP_HIP_EINVAL;
  }
  if (op->deconv_phases == 0) {
    /* one table over all taps: the convolution form, with the transposed table (setup) */
    return qnnp_igemm_launch(op, input, input2, output);
  }
  /* strided deconvolution: one dense implicit GEMM per output phase, all in one launch (upload_phase_table) */
  if (op->phase_table_entries == 0) return QNNP_HIP_OK;
  struct qnnp_hip_igemm_args pargs = qnnp_igemm_args(op, input, output);
  pargs.packed_w = (const int8_t*) op->phase[0].d_weights;   /* per-phase fields come from the table */
  pargs.bias2 = op->phase[0].d_bias;
  pargs.offsets = (const int32_t*) op->d_phase_table;          /* non-NULL marks the convolution form */
  pargs.rows = (uint32_t) (op->batch_size * op->phase_max_rows);
  pargs.rows_per_image = (uint32_t) op->phase_max_rows;
  pargs.k_pad = op->phase_max_k_pad;
  pargs.variant = 1;
  pargs.out_image_rows = (uint32_t) (op->output_height * op->output_width);
  pargs.phases = (const struct qnnp_hip_igemm_phase*) op->d_phase_table;
  pargs.nphases = op->phase_table_entries;
  return qnnp_hip_igemm_run(&pargs, &op->kernel_name);
}

static enum qnnp_status qnnp_create_deconvolution2d_nhwc_q8_impl(
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t adjustment_height,
    uint32_t adjustment_width,
    uint32_t kernel_height,
    uint32_t kernel_width,
    uint32_t stride_height,
    uint32_t stride_width,
    uint32_t dilation_height,
    uint32_t dilation_width,
    uint32_t groups,
    size_t group_input_channels,
    size_t group_output_channels,
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
    qnnp_operator_t* deconvolution_out)
{
  (void) flags;
  qnnp_operator_t op = NULL;

  /* reference deconvolution.c:74-116 (:69-72, the initialization, is the entry point's guard) */
  enum qnnp_status status = qnnp_status_invalid_parameter;
  if (kernel_width == 0 || kernel_height == 0) {
    qnnp_log_error("cannot create deconvolution with %" PRIu32 "x%" PRIu32 " kernel: kernel dimensions may not be zero",
        kernel_width, kernel_height);
    goto error;
  }
  if (stride_width == 0 || stride_height == 0) {
    qnnp_log_error("cannot create deconvolution with %" PRIu32 "x%" PRIu32 " stride: stride dimensions may not be zero",
        stride_width, stride_height);
    goto error;
  }
  if (dilation_width == 0 || dilation_height == 0) {
    qnnp_log_error("cannot create deconvolution with %" PRIu32 "x%" PRIu32 " dilation: dilation dimensions may not be zero",
        dilation_width, dilation_height);
    goto error;
  }
  if (!scale_is_valid(input_scale)) {
    qnnp_log_error("cannot create deconvolution with %.7g input scale: a scale has to be a finite number above zero", input_scale);
    goto error;
  }
  if (!scale_is_valid(kernel_scale)) {
    qnnp_log_error("cannot create deconvolution with %.7g kernel scale: a scale has to be a finite number above zero", kernel_scale);
    goto error;
  }
  if (!scale_is_valid(output_scale)) {
    qnnp_log_error("cannot create deconvolution with %.7g output scale: a scale has to be a finite number above zero", output_scale);
    goto error;
  }
  if (groups == 0 || group_input_channels == 0 || group_output_channels == 0 || kernel == NULL || bias == NULL) {
    qnnp_log_error("cannot create deconvolution: groups, channel counts, kernel and bias may not be zero");
    goto error;
  }

  /* reference deconvolution.c:118-128 */
  status = qnnp_status_unsupported_parameter;
  const float deconvolution_scale = input_scale * kernel_scale / output_scale;
  if (deconvolution_scale >= 1.0f) {
    qnnp_log_error(
        "cannot create deconvolution with %.7g input scale, %.7g kernel scale, and %.7g output scale: "
        "deconvolution scale %.7g is greater or equal to 1.0",
        input_scale, kernel_scale, output_scale, deconvolution_scale);
    goto error;
  }
  if (!(deconvolution_scale >= 0x1.0p-32f)) {
    qnnp_log_error("cannot create deconvolution: deconvolution scale %.7g is below 2**-32", deconvolution_scale);
    goto error;
  }
  const size_t kernel_size = (size_t) kernel_height * kernel_width;
  if (kernel_size * group_input_channels > (size_t) UINT32_MAX / 4 ||
      (size_t) groups * group_output_channels > (size_t) UINT32_MAX / 4) {
    qnnp_log_error("cannot create deconvolution: channel / kernel extents exceed the 32-bit index range of the device kernels");
    goto error;
  }

  status = qnnp_status_out_of_memory;
  op = qnnp_allocate_operator(qnnp_ukernel_type_conv, launch_deconvolution);   /* reference deconvolution.c:203 */
  if (op == NULL) {
    goto error;
  }
  op->input_padding_top = input_padding_top;
  op->input_padding_right = input_padding_right;
  op->input_padding_bottom = input_padding_bottom;
  op->input_padding_left = input_padding_left;
  op->adjustment_height = adjustment_height;
  op->adjustment_width = adjustment_width;
  op->kernel_height = kernel_height;
  op->kernel_width = kernel_width;
  op->stride_height = stride_height;
  op->stride_width = stride_width;
  op->dilation_height = dilation_height;
  op->dilation_width = dilation_width;
  op->groups = groups;
  op->group_input_channels = group_input_channels;
  op->group_output_channels = group_output_channels;
  op->input_zero_point = input_zero_point;
  op->kernel_zero_point = kernel_zero_point;
  op->requant = qnnp_compute_requant(deconvolution_scale, output_zero_point, output_min, output_max);
  op->requant.accumulator_bits = qnnp_accumulator_bits(bias, (size_t) groups * group_output_channels,
      kernel_size * group_input_channels);
  op->transposed = 1;

  status = pack_deconvolution(op, kernel, bias);
  if (status != qnnp_status_success) {
    goto error;
  }

  *deconvolution_out = op;
  return qnnp_status_success;

error:
  qnnp_delete_operator(op);
  return status;
}

/* The device-side description of the phase GEMMs of the geometry and batch bound to `op`: all non-empty phases run
 * as ONE launch of the offset-table kernel (blockIdx.y = phase), so that the small per-phase problems fill the chip
 * together and a workgroup's next tile overlaps its current epilogue. */
static enum qnnp_status upload_phase_table(struct qnnp_operator* op)
{
  struct qnnp_hip_igemm_phase table[QNNP_MAX_DECONV_PHASES];
  uint32_t n = 0;
  op->phase_max_rows = 0;
  op->phase_max_k_pad = 0;
  for (uint32_t i = 0; i < op->deconv_phases; i++) {
    const struct qnnp_deconv_phase* ph = &op->phase[i];
    if (ph->rows == 0) continue;
    table[n].packed_w = (const int8_t*) ph->d_weights;
    table[n].bias2 = ph->d_bias;
    table[n].offsets = ph->d_offsets;
    table[n].out_rows = ph->d_out_rows;
    table[n].rows = (uint32_t) (op->batch_size * ph->rows);
    table[n].rows_per_image = (uint32_t) ph->rows;
    table[n].ks = ph->taps;
    table[n].k_total = ph->taps * op->kc_slot;
    table[n].k_pad = ph->k_pad;
    table[n].reserved = 0;
    if (ph->rows > op->phase_max_rows) op->phase_max_rows = ph->rows;
    if (ph->k_pad > op->phase_max_k_pad) op->phase_max_k_pad = ph->k_pad;
    n++;
  }
  op->phase_table_entries = n;
  if (n == 0) return qnnp_status_success;
  if (op->d_phase_table == NULL) {
    op->d_phase_table = qnnp_hip_alloc(sizeof(table));
    if (op->d_phase_table == NULL) {
      qnnp_log_error("out of host memory: %zu bytes for the phase table", sizeof(table));
      return qnnp_status_out_of_memory;
    }
  }
  if (qnnp_hip_h2d(op->d_phase_table, table, sizeof(struct qnnp_hip_igemm_phase) * n, 0) != QNNP_HIP_OK) {
    qnnp_log_error("failed to upload the phase table");
    return qnnp_status_out_of_memory;
  }
  return qnnp_status_success;
}

/* The per-phase offset tables and output-row lists of the geometry bound to `op` (setup). */
static enum qnnp_status build_phase_tables(struct qnnp_operator* op)
{
  const size_t input_height = op->input_height, input_width = op->input_width, input_pixel_stride = op->input_pixel_stride;
  op->offsets_in_h = 0;
  const size_t sh = op->stride_height, sw = op->stride_width;
  for (uint32_t i = 0; i < op->deconv_phases; i++) {
    struct qnnp_deconv_phase* ph = &op->phase[i];
    const size_t py = i / sw, px = i % sw;
    /* first output row / column of the phase: (o + pad) % stride == phase */
    const size_t oy0 = (py + sh - op->input_padding_top % sh) % sh;
    const size_t ox0 = (px + sw - op->input_padding_left % sw) % sw;
    const size_t rows_y = oy0 < op->output_height ? (op->output_height - oy0 + sh - 1) / sh : 0;
    const size_t rows_x = ox0 < op->output_width ? (op->output_width - ox0 + sw - 1) / sw : 0;
    ph->rows = rows_y * rows_x;
    if (ph->rows == 0) continue;
    int32_t* host_offsets = (int32_t*) malloc(sizeof(int32_t) * ph->rows * ph->taps);
    int32_t* host_rows = (int32_t*) malloc(sizeof(int32_t) * ph->rows);
    if (host_offsets == NULL || host_rows == NULL) {
      free(host_offsets);
      free(host_rows);
      qnnp_log_error("out of host memory: %zu bytes for a phase table", sizeof(int32_t) * ph->rows * (ph->taps + 1));
      return qnnp_status_out_of_memory;
    }
    size_t r = 0;
    for (size_t oy = oy0; oy < op->output_height; oy += sh) {
      for (size_t ox = ox0; ox < op->output_width; ox += sw, r++) {
        host_rows[r] = (int32_t) (oy * op->output_width + ox);
        for (uint32_t t = 0; t < ph->taps; t++) {
          int32_t entry = QNNP_OFFSET_PADDING;
          if (ph->tap_ky[t] != 255) {
            /* reference src/indirection.c:171-177; the divisions are exact by construction of the phase */
            const size_t y = oy + op->input_padding_top - (size_t) ph->tap_ky[t] * op->dilation_height;
            const size_t x = ox + op->input_padding_left - (size_t) ph->tap_kx[t] * op->dilation_width;
            const size_t iy = y / sh, ix = x / sw;
            if (iy * sh == y && iy < input_height && ix * sw == x && ix < input_width) {
              entry = (int32_t) ((iy * input_width + ix) * input_pixel_stride);
            }
          }
          host_offsets[r * ph->taps + t] = entry;
        }
      }
    }
    const size_t entries = ph->rows * ph->taps;
    const int ok =
        qnnp_upload_table((void**) &ph->d_offsets, &ph->offsets_capacity, entries, sizeof(int32_t) * entries, host_offsets,
            sizeof(int32_t) * entries) &&
        qnnp_upload_table((void**) &ph->d_out_rows, &ph->rows_capacity, ph->rows, sizeof(int32_t) * ph->rows, host_rows,
            sizeof(int32_t) * ph->rows);
    free(host_offsets);
    free(host_rows);
    if (!ok) {
      qnnp_log_error("failed to place a phase table on the device");
      return qnnp_status_out_of_memory;
    }
  }
  op->offsets_in_h = input_height;
  op->offsets_in_w = input_width;
  op->offsets_in_stride = input_pixel_stride;
  return qnnp_status_success;
}

static enum qnnp_status qnnp_setup_deconvolution2d_nhwc_q8_impl(
    qnnp_operator_t op,
    size_t batch_size,
    size_t input_height,
    size_t input_width,
    const uint8_t* input,
    size_t input_pixel_stride,
    uint8_t* output,
    size_t output_pixel_stride,
    pthreadpool_t threadpool)
{
  (void) threadpool;

  if (!op->transposed) {
    return qnnp_status_invalid_parameter;
  }

  /* reference deconvolution.c:230-233 */
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }

  /* reference deconvolution.c:235-241 */
  if (input_width == 0 || input_height == 0) {
    qnnp_log_error("cannot set up deconvolution with %zux%zu input: input dimensions may not be zero",
        input_width, input_height);
    return qnnp_status_invalid_parameter;
  }
  const size_t in_channels = (size_t) op->groups * op->group_input_channels;
  const size_t out_channels = (size_t) op->groups * op->group_output_channels;
  if (input == NULL || output == NULL || input_pixel_stride < in_channels || output_pixel_stride < out_channels) {
    qnnp_log_error("cannot set up deconvolution: NULL tensor or pixel stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  const size_t pad_h = (size_t) op->input_padding_top + op->input_padding_bottom;
  const size_t pad_w = (size_t) op->input_padding_left + op->input_padding_right;
  const size_t full_h = compute_output_dimension(input_height, 0, op->adjustment_height, op->kernel_height,
      op->dilation_height, op->stride_height);
  const size_t full_w = compute_output_dimension(input_width, 0, op->adjustment_width, op->kernel_width,
      op->dilation_width, op->stride_width);
  if (pad_h >= full_h || pad_w >= full_w) {
    qnnp_log_error("cannot set up deconvolution with %zux%zu input: the padding removes the whole output",
        input_width, input_height);
    return qnnp_status_invalid_parameter;
  }

  /* reference deconvolution.c:243-262 */
  op->setup_valid = 0;   /* until every check, allocation and upload below has succeeded */
  op->batch_size = batch_size;
  op->input_height = input_height;
  op->input_width = input_width;
  op->input = input;
  op->input_pixel_stride = input_pixel_stride;
  op->output_height = full_h - pad_h;
  op->output_width = full_w - pad_w;
  op->output = output;
  op->output_pixel_stride = output_pixel_stride;

  const size_t output_size = op->output_height * op->output_width;
  const size_t input_size = input_height * input_width;
  if (batch_size * output_size > (size_t) UINT32_MAX / 2 || input_size * input_pixel_stride > (size_t) INT32_MAX) {
    qnnp_log_error("cannot set up deconvolution: %zu output pixels / %zu-byte images exceed the device kernels' index range",
        batch_size * output_size, input_size * input_pixel_stride);
    return qnnp_status_unsupported_parameter;
  }

  op->input_span = (batch_size * input_size - 1) * input_pixel_stride + in_channels;
  op->output_span = (batch_size * output_size - 1) * output_pixel_stride + out_channels;
  const enum qnnp_status bound = qnnp_bind_tensors(op, "qnnp_setup_deconvolution2d_nhwc_q8");
  if (bound != qnnp_status_success) {
    return bound;
  }

  op->variant = 1;   /* the offset-table kernel: the table, not the geometry, defines this operator */
  op->deconv_stream = qnnp_state.opt_gemm_kernel == 13 ? 2 : (qnnp_state.opt_gemm_kernel == 1 ? 1 : 0);
  if (op->deconv_phases != 0) {
    /* offset tables are pointer- and batch-invariant; the row counts are not */
    if (op->offsets_in_h != input_height || op->offsets_in_w != input_width ||
        op->offsets_in_stride != input_pixel_stride) {
      const enum qnnp_status status = build_phase_tables(op);
      if (status != qnnp_status_success) {
        return status;
      }
    }
    return upload_phase_table(op);
  }
  const size_t kernel_size = (size_t) op->kernel_height * op->kernel_width;
  const size_t entries = output_size * kernel_size;
  const bool same_geometry = op->d_offsets != NULL &&
      op->offsets_in_h == input_height && op->offsets_in_w == input_width &&
      op->offsets_in_stride == input_pixel_stride;
  if (same_geometry) {
    return qnnp_status_success;  /* the table is pointer- and batch-invariant */
  }
  const size_t bytes = sizeof(int32_t) * entries;
  int32_t* host_table = (int32_t*) malloc(bytes);
  if (host_table == NULL) {
    qnnp_log_error("out of host memory: %zu bytes for the offset table", bytes);
    return qnnp_status_out_of_memory;
  }
  qnnp_indirection_init_deconv2d_offsets(op, host_table);
  const int uploaded = qnnp_upload_table((void**) &op->d_offsets, &op->offsets_capacity, entries, bytes, host_table, bytes);
  free(host_table);
  if (!uploaded) {
    if (op->d_offsets == NULL) {
      qnnp_log_error("out of host memory: %zu bytes for the device offset table", bytes);
    } else {
      op->offsets_in_h = 0;
      qnnp_log_error("failed to upload the offset table");
    }
    return qnnp_status_out_of_memory;
  }
  op->offsets_in_h = input_height;
  op->offsets_in_w = input_width;
  op->offsets_in_stride = input_pixel_stride;
  return qnnp_status_success;
}

/* ---- public entry points: the implementations above inside the device guards of lifecycle.h ---- */

enum qnnp_status qnnp_create_deconvolution2d_nhwc_q8(
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t adjustment_height,
    uint32_t adjustment_width,
    uint32_t kernel_height,
    uint32_t kernel_width,
    uint32_t stride_height,
    uint32_t stride_width,
    uint32_t dilation_height,
    uint32_t dilation_width,
    uint32_t groups,
    size_t group_input_channels,
    size_t group_output_channels,
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
    qnnp_operator_t* deconvolution_out)
{
  int token;
  const enum qnnp_status status = qnnp_enter_create("qnnp_create_deconvolution2d_nhwc_q8", &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token,
      qnnp_create_deconvolution2d_nhwc_q8_impl(input_padding_top, input_padding_right, input_padding_bottom,
          input_padding_left, adjustment_height, adjustment_width, kernel_height, kernel_width, stride_height,
          stride_width, dilation_height, dilation_width, groups, group_input_channels, group_output_channels,
          input_zero_point, input_scale, kernel_zero_point, kernel_scale, kernel, bias, output_zero_point,
          output_scale, output_min, output_max, flags, deconvolution_out));
}

enum qnnp_status qnnp_setup_deconvolution2d_nhwc_q8(
    qnnp_operator_t op,
    size_t batch_size,
    size_t input_height,
    size_t input_width,
    const uint8_t* input,
    size_t input_pixel_stride,
    uint8_t* output,
    size_t output_pixel_stride,
    pthreadpool_t threadpool)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_setup_deconvolution2d_nhwc_q8", op, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(op, token,
      qnnp_setup_deconvolution2d_nhwc_q8_impl(op, batch_size, input_height, input_width, input, input_pixel_stride,
          output, output_pixel_stride, threadpool));
}
