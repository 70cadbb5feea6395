/*
 * convolution.c -- qnnp_create_convolution2d_nhwc_q8 / qnnp_setup_convolution2d_nhwc_q8
 * for the gfx950 build.
 *
 * Replaces reference src/convolution.c:39-378 (create) and :380-492 (setup):
 * same argument validation and status codes, same operator-type selection idea,
 * but the products of create/setup are device-resident:
 *   create: weights re-laid-out as MFMA operand fragments (or a tap-major int16
 *           image for depthwise) with both zero points folded into an int32 bias,
 *           uploaded once; Q31 requantization parameters.
 *   setup : output geometry; for general convolutions a batch-invariant int32
 *           offset table (pixel x tap -> byte offset inside one image, -1 = padding)
 *           instead of the reference's per-image table of absolute host pointers
 *           (src/indirection.c:18-79) -- im2col is never materialised and the
 *           table does not depend on the input pointer or the batch size.
 */
#include <math.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950_perchannel.h>

#include "hip/qnnp_hip.h"
#include "indirection.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "bias-pair.h"
#include "pack.h"
#include "per-channel.h"
#include "requantization.h"
#include "state.h"
#include "upload.h"

/* reference src/convolution.c:29-37 */
static inline size_t compute_output_dimension(
    size_t padded_input, size_t kernel, size_t dilation, size_t subsampling)
{
  const size_t effective_kernel = (kernel - 1) * dilation + 1;
  return (padded_input - effective_kernel) / subsampling + 1;
}

static inline bool scale_is_valid(float scale)
{
  return scale > 0.0f && isnormal(scale);
}

/* ---- depthwise images ------------------------------------------------------------------------------------------------
 * the tap-major int16 image and its bias (required), the int8 dot-product image of 3x3 / 5x5 windows with weights in
 * int8 range (required where it applies) and the matrix-core weight parts (required) */
static enum qnnp_status pack_depthwise(struct qnnp_operator* op, const uint8_t* kernel, const int32_t* bias)
{
  const uint32_t groups = op->groups, kh = op->kernel_height, kw = op->kernel_width;
  const size_t kernel_size = (size_t) kh * kw;
  const uint32_t c_pad = qnnp_round_up_u32(groups, 16);
  const size_t w_bytes = sizeof(int16_t) * kernel_size * c_pad;
  const size_t b_bytes = sizeof(int32_t) * c_pad;
  int16_t* host_weights = (int16_t*) malloc(w_bytes);
  int32_t* host_bias = (int32_t*) malloc(b_bytes);
  enum qnnp_status status = qnnp_status_out_of_memory;
  if (host_weights == NULL || host_bias == NULL) {
    qnnp_log_error("out of host memory: %zu bytes for packed weights", w_bytes + b_bytes);
    goto done;
  }
  qnnp_pack_dwconv_w(groups, c_pad, kh, kw, op->input_zero_point, op->kernel_zero_point, kernel, bias, host_weights, host_bias);
  op->c_pad = c_pad;
  op->dw_wrange = qnnp_dwconv_weight_range(host_weights, kernel_size * c_pad);
  op->d_weights = qnnp_upload(host_weights, w_bytes);
  op->d_bias = (int32_t*) qnnp_upload(host_bias, b_bytes);
  if (op->d_weights == NULL || op->d_bias == NULL) {
    qnnp_log_error("device allocation or upload failed: %zu bytes of packed depthwise weights on the device", w_bytes + b_bytes);
    goto done;
  }
  if (op->per_channel) {
    /* the kernels of hip/q8dwconv_pc.hip read these two images and the table: nothing below has a reader */
    status = qnnp_status_success;
    goto done;
  }
  /* 3x3 with weights in int8 range: the register image of the int8 dot-product walk (pack.h); 5x5 likewise: eight rows
   * (pack.h qnnp_pack_dwconv_dot4_5x5) */
  if (kh == kw && (kh == 3 || kh == 5) && op->dw_wrange != 0) {
    const size_t q_bytes = sizeof(uint32_t) * (kh == 3 ? 4 : 8) * c_pad;
    uint32_t* host_q = (uint32_t*) malloc(q_bytes);
    if (host_q != NULL) {
      if (kh == 3) {
        qnnp_pack_dwconv_dot4(c_pad, op->dw_wrange, host_weights, host_bias, host_q);
      } else {
        qnnp_pack_dwconv_dot4_5x5(c_pad, op->dw_wrange, host_weights, host_bias, host_q);
      }
      op->d_dw_dot4 = qnnp_upload(host_q, q_bytes);
      free(host_q);
    }
    if (op->d_dw_dot4 == NULL) {
      qnnp_log_error("device allocation or upload failed: %zu bytes of depthwise dot-product weights on the device", q_bytes);
      goto done;
    }
  }
  /* second image: int8 weight parts + folded bias for the matrix-core depthwise kernel */
  const uint32_t c_pad32 = qnnp_round_up_u32(groups, 32);
  const size_t x_bytes = (size_t) 3 * kernel_size * c_pad32;
  const size_t bm_bytes = sizeof(int32_t) * c_pad32;
  int8_t* host_x = (int8_t*) malloc(x_bytes);
  int32_t* host_bm = (int32_t*) malloc(bm_bytes);
  if (host_x != NULL && host_bm != NULL) {
    op->dwm_parts = qnnp_pack_dwconv_mfma(groups, c_pad32, kh, kw, op->input_zero_point, op->kernel_zero_point, kernel, bias,
        host_x, host_bm);
    op->c_pad32 = c_pad32;
    op->d_dwm_x = qnnp_upload(host_x, x_bytes);
    op->d_dwm_bias = (int32_t*) qnnp_upload(host_bm, bm_bytes);
  }
  free(host_x);
  free(host_bm);
  if (op->d_dwm_x == NULL || op->d_dwm_bias == NULL) {
    qnnp_log_error("device allocation or upload failed: %zu bytes of depthwise weight parts on the device", x_bytes + bm_bytes);
    goto done;
  }
  status = qnnp_status_success;
done:
  free(host_weights);
  free(host_bias);
  return status;
}

/* ---- GEMM images ---------------------------------------------------------------------------------------------------- */

/* Grouped 1x1 as one dense GEMM (round 6). A group of 12 ... 68 channels fills a fifth ... a half of a 64-byte K step and a
 * 128-channel tile, every group's tile stages its own copy of the rows, and its output pieces are 12 ... 68 bytes; the dense
 * [groups * GOC][groups * GIC] matrix with the groups' blocks on its diagonal and the KERNEL ZERO POINT everywhere else
 * ((w - kzp) = 0: the grouped result bit for bit) reads every input byte once and writes whole pixels, at `groups` times the
 * multiplies -- which these layers do not notice: ShuffleNet v1's 28x28 layers at batch 128 run 15 ... 59 us grouped and 12 ... 27
 * dense (profiles/r06/grouped_1x1_dense_equivalents_r06v.txt); from 14x14 down the two are level or the grouped form leads, so
 * the launch takes this image from 65536 rows up. Built for up to 1024 channels on either side (<= 1 MiB of weights).
 * Optional: without it the operator keeps its grouped image. */
static void pack_dense_optional(struct qnnp_operator* op, const uint8_t* kernel, const int32_t* bias)
{
  const size_t gic = op->group_input_channels, goc = op->group_output_channels;
  const uint32_t cin = (uint32_t) (op->groups * gic), cout = (uint32_t) (op->groups * goc);
  const uint32_t n_pad_d = qnnp_round_up_u32(cout, 32), k_pad_d = qnnp_round_up_u32(cin, 64);
  const size_t wd_bytes = qnnp_igemm_packed_weights_size(1, n_pad_d, k_pad_d);
  uint8_t* dense = (uint8_t*) malloc((size_t) cout * cin);
  int8_t* host_wd = (int8_t*) malloc(wd_bytes);
  int32_t* host_bd = (int32_t*) malloc(sizeof(int32_t) * n_pad_d);
  if (dense != NULL && host_wd != NULL && host_bd != NULL) {
    memset(dense, op->kernel_zero_point, (size_t) cout * cin);
    for (uint32_t g = 0; g < op->groups; g++) {
      for (size_t oc = 0; oc < goc; oc++) {
        memcpy(dense + (g * goc + oc) * cin + g * gic, kernel + (g * goc + oc) * gic, gic);
      }
    }
    qnnp_pack_igemm_w_slots(1, cout, 1, cin, cin, n_pad_d, k_pad_d, op->input_zero_point, op->kernel_zero_point, dense, bias,
        host_wd, host_bd);
    op->d_weights_dense = qnnp_upload(host_wd, wd_bytes);
    op->d_bias_dense = qnnp_upload_bias_pair(host_bd, n_pad_d);
  }
  free(dense);
  free(host_wd);
  free(host_bd);
  if (op->d_weights_dense != NULL && op->d_bias_dense != NULL) {
    op->dense_n_pad = n_pad_d;
    op->dense_k_pad = k_pad_d;
    return;
  }
  qnnp_log_warning("no room for %zu bytes of dense weights on the device: the operator keeps the grouped image", wd_bytes);
  qnnp_hip_free(op->d_weights_dense);
  qnnp_hip_free(op->d_bias_dense);
  op->d_weights_dense = NULL;
  op->d_bias_dense = NULL;
}

/* The second, kernel-zero-point-127 image + bias pair of the zero-point-centred kernels (pack.h
 * qnnp_pack_igemm_w_centred127). Optional: without it the operator runs on the standard image (row term in the
 * kernel). */
static void pack_centred127_optional(struct qnnp_operator* op, const uint8_t* kernel, const int32_t* bias, uint32_t k_total)
{
  const size_t w_bytes = qnnp_igemm_packed_weights_size(1, op->n_pad, op->k_pad);
  const size_t b_bytes = sizeof(int32_t) * op->n_pad;
  int8_t* host_wc = (int8_t*) malloc(w_bytes);
  int32_t* host_bc = (int32_t*) malloc(b_bytes);
  if (host_wc != NULL && host_bc != NULL) {
    qnnp_pack_igemm_w_centred127((uint32_t) op->group_output_channels, k_total, op->k_pad, op->n_pad, op->input_zero_point,
        kernel, bias, host_wc, host_bc);
    op->d_weights_centred = qnnp_upload(host_wc, w_bytes);
    op->d_bias_centred = qnnp_upload_bias_pair(host_bc, op->n_pad);
  }
  free(host_wc);
  free(host_bc);
  if (op->d_weights_centred != NULL && op->d_bias_centred != NULL) {
    op->centre_flip = 0x7F;
    return;
  }
  qnnp_log_warning("no room for %zu bytes of centred weights on the device: the operator keeps the standard image", w_bytes + 2 * b_bytes);
  qnnp_hip_free(op->d_weights_centred);
  qnnp_hip_free(op->d_bias_centred);
  op->d_weights_centred = NULL;
  op->d_bias_centred = NULL;
}

/* First layers (3-channel inputs in 4-byte tap slots): the row-slot image beside the tap-slot one (hip/q8convc3.hip takes
 * it when pixels are dense) -- 16-byte row slots, or 32-byte ones for the larger windows (5x5, ResNet's 7x7 entry layer):
 * same pointer, the window decides which image it is. Centred on kernel zero point 127 it has its own bias pair and no
 * row term in the kernel (pack.h). Required where it applies. */
static enum qnnp_status pack_rows(struct qnnp_operator* op, const uint8_t* kernel, const int32_t* bias)
{
  const uint32_t kh = op->kernel_height, kw = op->kernel_width, n_pad = op->n_pad, goc = (uint32_t) op->group_output_channels;
  const int undilated = op->dilation_height == 1 && op->dilation_width == 1;
  const int rows16 = kh <= 4 && kw * 3 <= 16 && undilated && n_pad <= 64;
  const int rows32 = (kh == 5 || kh == 7) && kw * 3 <= 32 && undilated && n_pad <= (kh == 7 ? 96u : 64u);
  if (op->kc_slot != 4 || !(rows16 || rows32)) {
    return qnnp_status_success;
  }
  const size_t r_bytes = rows16 ? (size_t) n_pad * 64 : qnnp_conv_rows32_size(n_pad, kh);
  int8_t* host_rows = (int8_t*) malloc(r_bytes);
  if (host_rows == NULL) {
    qnnp_log_error("out of host memory: %zu bytes for packed weights", r_bytes);
    return qnnp_status_out_of_memory;
  }
  int placed = 1;
  if (op->kernel_zero_point == 127) {
    int32_t* host_bc = (int32_t*) malloc((size_t) n_pad * sizeof(int32_t));
    placed = host_bc != NULL;
    if (placed) {
      if (rows16) {
        qnnp_pack_conv_rows16_centred127(goc, kh, kw, 3, n_pad, op->input_zero_point, kernel, bias, host_rows, host_bc);
      } else {
        qnnp_pack_conv_rows32_centred127(goc, kh, kw, 3, n_pad, op->input_zero_point, kernel, bias, host_rows, host_bc);
      }
      op->d_bias_rows = qnnp_upload_bias_pair(host_bc, n_pad);
      placed = op->d_bias_rows != NULL;
    }
    free(host_bc);
  } else if (rows16) {
    qnnp_pack_conv_rows16(goc, kh, kw, 3, n_pad, kernel, host_rows);
  } else {
    qnnp_pack_conv_rows32(goc, kh, kw, 3, n_pad, kernel, host_rows);
  }
  if (placed) {
    op->d_weights_rows16 = qnnp_upload(host_rows, r_bytes);
  }
  free(host_rows);
  if (op->d_weights_rows16 == NULL) {
    qnnp_log_error("device allocation or upload failed: %zu bytes of packed weights on the device", r_bytes);
    return qnnp_status_out_of_memory;
  }
  return qnnp_status_success;
}

/* the MFMA fragment image and its bias pair (required), then the optional dense and centred images and the row-slot one */
static enum qnnp_status pack_gemm(struct qnnp_operator* op, const uint8_t* kernel, const int32_t* bias)
{
  const uint32_t groups = op->groups, kh = op->kernel_height, kw = op->kernel_width;
  const size_t gic = op->group_input_channels, goc = op->group_output_channels;
  const size_t kernel_size = (size_t) kh * kw;
  /* 3-channel inputs (first layers): one unaligned 4-byte fetch per tap, see pack.h "channel slots" */
  const uint32_t kc_slot = (op->ukernel_type == qnnp_ukernel_type_conv && groups == 1 && gic == 3) ? 4u : (uint32_t) gic;
  const uint32_t k_total = (uint32_t) (kernel_size * kc_slot);
  const uint32_t n_pad = qnnp_round_up_u32((uint32_t) goc, 32);
  const uint32_t k_pad = qnnp_round_up_u32(k_total, 64);
  const size_t w_bytes = qnnp_igemm_packed_weights_size(groups, n_pad, k_pad);
  const size_t b_bytes = sizeof(int32_t) * (size_t) groups * n_pad;
  int8_t* host_weights = (int8_t*) malloc(w_bytes);
  int32_t* host_bias = (int32_t*) malloc(b_bytes);
  if (host_weights == NULL || host_bias == NULL) {
    free(host_weights);
    free(host_bias);
    qnnp_log_error("out of host memory: %zu bytes for packed weights", w_bytes + b_bytes);
    return qnnp_status_out_of_memory;
  }
  qnnp_pack_igemm_w_slots(groups, (uint32_t) goc, (uint32_t) kernel_size, (uint32_t) gic, kc_slot, n_pad, k_pad,
      op->input_zero_point, op->kernel_zero_point, kernel, bias, host_weights, host_bias);
  op->n_pad = n_pad;
  op->k_pad = k_pad;
  op->kc_slot = kc_slot;
  op->d_weights = qnnp_upload(host_weights, w_bytes);
  op->d_bias = qnnp_upload_bias_pair(host_bias, (size_t) groups * n_pad);   /* bias-pair.h */
  free(host_weights);
  free(host_bias);
  if (op->d_weights == NULL || op->d_bias == NULL) {
    qnnp_log_error("device allocation or upload failed: %zu bytes of packed weights on the device", w_bytes + 2 * b_bytes);
    return qnnp_status_out_of_memory;
  }
  if (op->per_channel) {
    /* the per-channel flavour of the generic kernel reads this image and the table: never the grouped-as-dense image,
     * the centred one or the row slots */
    return qnnp_status_success;
  }
  if (op->ukernel_type == qnnp_ukernel_type_gemm && groups > 1 && groups * gic <= 1024 && groups * goc <= 1024) {
    pack_dense_optional(op, kernel, bias);
  }
  /* Zero-point-centred image (pack.h qnnp_pack_igemm_w_centred127; hip/q8gemm256c.hip, the weight-stationary 3x3
   * kernel of hip/q8convwave.hip): single group, whole 32-deep K blocks, kernel zero point 128 (the standard image IS the centred
   * one) or 127 (a second image + bias pair). The [output channel][kh][kw][input channel] kernel tensor is the GEMM
   * layout the packer takes. */
  /* (round 6: hip/q8convws16s.hip -- 3x3 windows over 16 / 32 / 48 / 64 input channels, SqueezeNet's fire modules -- takes the image
   * WITH K padding: 9 x 16 and 9 x 48 bytes are not whole 32-byte blocks; the padding meets zero weights in either image) */
  const int small_3x3 = kh == 3 && kw == 3 && gic % 16 == 0 && gic <= 64 && goc % 16 == 0 && goc <= 256;
  if (groups == 1 && kc_slot == (uint32_t) gic && (k_total % 32 == 0 || small_3x3)) {
    if (op->kernel_zero_point == 128) {
      op->centre_flip = 0x80;
    } else if (op->kernel_zero_point == 127 &&
               /* (a second image only where a kernel takes it: the 3x3 weight-stationary kernel, the 256x256 GEMM) */
               (small_3x3 ||
                (kernel_size == 1 && k_total == k_pad && k_total >= 512 && n_pad % 256 == 0) ||
                /* ... and the 128-wide tiling of hip/q8gemm128x.hip: any K % 64 == 0 */
                (kernel_size == 1 && k_total == k_pad && k_total % 64 == 0 && goc % 4 == 0))) {
      pack_centred127_optional(op, kernel, bias, k_total);
    }
  }
  return pack_rows(op, kernel, bias);
}

/* ---- launches: one call through the C-ABI HIP shim (hip/qnnp_hip.h) per operator ------------------------------------ */

/* `rc` is what the operator's own kernel answered. An attached residual add (residual.c) that the kernel did not carry
 * follows as the add kernel, in place on the output. */
static int finish_residual_add(struct qnnp_operator* op, void* output, int rc)
{
  if (rc != QNNP_HIP_OK || op->residual == NULL || op->residual_folded) return rc;
  const struct qnnp_hip_vadd_args args = qnnp_vadd_args(op, op->residual, op->residual_pixel_stride,
      output, op->output_pixel_stride, output, op->output_pixel_stride,
      op->batch_size * op->output_height * op->output_width, (size_t) op->groups * op->group_output_channels,
      &op->residual_params);
  const char* add_kernel = NULL;
  return qnnp_hip_vadd_run(&args, &add_kernel);
}

/* Likewise an attached output table (output-table.c) that the kernel did not carry follows as the table kernel, in place
 * on the output: with host endpoints `output` is the staged device output, which the caller copies back afterwards.
 * (hip/x8lut.hip is no part of the seam library, oracle/Makefile: there the symbol is absent, and so is every way to
 * attach a table.) */
extern int qnnp_hip_lut_run(const struct qnnp_hip_lut_args* args, const char** kernel_name) __attribute__((weak));

static int finish_output_table(struct qnnp_operator* op, void* output, int rc)
{
  if (rc != QNNP_HIP_OK || op->d_output_table == NULL || op->table_folded) return rc;
  const size_t pixels = op->batch_size * op->output_height * op->output_width;
  if (qnnp_hip_lut_run == NULL || pixels > (size_t) INT32_MAX) return QNNP_HIP_EINVAL;
  const struct qnnp_hip_lut_args args = {
    .input = (const uint8_t*) output,
    .output = (uint8_t*) output,
    .table = (const uint8_t*) op->d_output_table,
    .pixels = (uint32_t) pixels,
    .channels = (uint32_t) ((size_t) op->groups * op->group_output_channels),
    .input_stride = op->output_pixel_stride,
    .output_stride = op->output_pixel_stride,
  };
  const char* table_kernel = NULL;   /* qnnp_gfx950_operator_kernel keeps the convolution kernel's name */
  return qnnp_hip_lut_run(&args, &table_kernel);
}

static int launch_dwconv(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  /* reference operator-run.c:647-710 (context) + :238-284 (trampolines) */
  const struct qnnp_hip_dwconv_args args = {
    .input = (const uint8_t*) input,
    .output = (uint8_t*) output,
    .streaming_mode = op->streaming_mode,
    .wadj = (const int16_t*) op->d_weights,
    .bias1 = op->d_bias,
    .dwm_x = (const int8_t*) op->d_dwm_x,
    .dwm_bias = op->d_dwm_bias,
    .dwm_parts = op->dwm_parts,
    .w_range = op->dw_wrange,
    .dot4 = (const uint32_t*) op->d_dw_dot4,
    .c_pad32 = op->c_pad32,
    .batch = (uint32_t) op->batch_size,
    .input_height = (uint32_t) op->input_height,
    .input_width = (uint32_t) op->input_width,
    .output_height = (uint32_t) op->output_height,
    .output_width = (uint32_t) op->output_width,
    .channels = op->groups,
    .c_pad = op->c_pad,
    .kernel_height = op->kernel_height,
    .kernel_width = op->kernel_width,
    .stride_height = op->stride_height,
    .stride_width = op->stride_width,
    .dilation_height = op->dilation_height,
    .dilation_width = op->dilation_width,
    .pad_top = op->input_padding_top,
    .pad_left = op->input_padding_left,
    .input_stride = (uint32_t) op->input_pixel_stride,
    .output_stride = (uint32_t) op->output_pixel_stride,
    .input_zero_point = op->input_zero_point,
    .rq = op->requant,
    .variant = op->variant,
    .plan = &op->dw_plan,
    .rq_pc = (const struct qnnp_requant_pc_entry*) op->d_requant_pc,
    .table = (const uint8_t*) op->d_output_table,
    .table_folded = &op->table_folded,
  };
  op->residual_folded = 0;
  op->table_folded = 0;
  return finish_output_table(op, output, finish_residual_add(op, output, qnnp_hip_dwconv_run(&args, &op->kernel_name)));
}

/* reference operator-run.c:770-804 (gemm) and :805-844 (conv) */
static int launch_igemm_kernel(struct qnnp_operator* op, const void* input, void* output)
{
  const int is_conv = op->ukernel_type == qnnp_ukernel_type_conv;
  const uint32_t output_size = (uint32_t) (op->output_height * op->output_width);
  const uint32_t taps = is_conv ? op->kernel_height * op->kernel_width : 1;
  struct qnnp_hip_igemm_args args = qnnp_igemm_args(op, input, output);
  args.packed_w = (const int8_t*) op->d_weights;
  args.packed_w_rows16 = is_conv ? (const int8_t*) op->d_weights_rows16 : NULL;
  args.bias2_rows = is_conv ? op->d_bias_rows : NULL;
  args.bias2 = op->d_bias;
  args.bias2_pair = 1;
  args.offsets = is_conv ? op->d_offsets : NULL;
  args.rows = (uint32_t) op->batch_size * output_size;
  args.rows_per_image = output_size;
  args.ks = taps;
  args.k_total = taps * op->kc_slot;
  args.k_pad = op->k_pad;
  args.variant = op->variant;
  args.input_height = (uint32_t) op->input_height;
  args.input_width = (uint32_t) op->input_width;
  args.output_height = (uint32_t) op->output_height;
  args.output_width = (uint32_t) op->output_width;
  args.kernel_height = op->kernel_height;
  args.kernel_width = op->kernel_width;
  args.stride_height = op->stride_height;
  args.stride_width = op->stride_width;
  args.dilation_height = op->dilation_height;
  args.dilation_width = op->dilation_width;
  args.pad_top = op->input_padding_top;
  args.pad_left = op->input_padding_left;
  args.residual = (const uint8_t*) op->residual;
  args.residual_stride = (uint32_t) op->residual_pixel_stride;
  args.residual_add = &op->residual_params;
  args.residual_folded = &op->residual_folded;
  /* zero-point-centred image (fully-connected.c): its own, or the standard one when that is centred already */
  args.packed_w_centred = (const int8_t*) (op->d_weights_centred != NULL ? op->d_weights_centred : op->d_weights);
  args.bias2_centred = op->d_bias_centred != NULL ? op->d_bias_centred : op->d_bias;
  args.centre_flip = op->centre_flip;
  args.rq_pc = (const struct qnnp_requant_pc_entry*) op->d_requant_pc;
  args.table = (const uint8_t*) op->d_output_table;
  args.table_folded = &op->table_folded;
  /* grouped 1x1 with a dense image (pack_dense_optional): many rows -> the dense GEMM; "gemm_kernel" 31 forces it (and is
   * refused where the operator keeps the grouped image), any other forced kernel keeps the grouped image */
  op->ran_dense = 0;
  if (op->d_weights_dense != NULL && op->residual == NULL &&
      (op->variant == 31 || (op->variant == 0 && (uint64_t) op->batch_size * output_size >= 65536u))) {
    args.packed_w = (const int8_t*) op->d_weights_dense;
    args.bias2 = op->d_bias_dense;
    args.groups = 1;
    args.n = (uint32_t) (op->groups * op->group_output_channels);
    args.n_pad = op->dense_n_pad;
    args.kc = (uint32_t) (op->groups * op->group_input_channels);
    args.kc_slot = args.k_total = args.kc;
    args.k_pad = op->dense_k_pad;
    args.variant = 0;
    args.packed_w_centred = args.packed_w;
    args.bias2_centred = args.bias2;
    args.centre_flip = 0;
    op->ran_dense = 1;
  }
  if (op->variant == 31 && !op->ran_dense) return QNNP_HIP_EINVAL;
  return qnnp_hip_igemm_run(&args, &op->kernel_name);
}

int qnnp_igemm_launch(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  op->residual_folded = 0;
  op->table_folded = 0;
  return finish_output_table(op, output, finish_residual_add(op, output, launch_igemm_kernel(op, input, output)));
}

/* kernel_scales == NULL: the per-tensor create with `kernel_scale`. Else the per-channel one: `per_channel` is set,
 * `kernel_scale` is unused and kernel_scales holds groups * group_output_channels floats. (per_channel with a NULL array
 * is the refusal the per-channel entry point owes its caller.) */
static enum qnnp_status qnnp_create_convolution2d_nhwc_q8_impl(
    int per_channel,
    const float* kernel_scales,
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t kernel_height,
    uint32_t kernel_width,
    uint32_t subsampling_height,
    uint32_t subsampling_width,
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
    qnnp_operator_t* convolution_out)
{
  (void) flags; /* accepted and ignored, as in the reference (convolution.c:63) */
  qnnp_operator_t op = NULL;

  /* 1. validate. reference convolution.c:74-115 (:69-72, the initialization, is the entry point's guard) */
  enum qnnp_status status = qnnp_status_invalid_parameter;
  if (kernel_width == 0 || kernel_height == 0) {
    qnnp_log_error("cannot create convolution with %" PRIu32 "x%" PRIu32 " kernel: kernel dimensions may not be zero",
        kernel_width, kernel_height);
    goto error;
  }
  if (subsampling_width == 0 || subsampling_height == 0) {
    qnnp_log_error("cannot create convolution with %" PRIu32 "x%" PRIu32 " subsampling: subsampling dimensions may not be zero",
        subsampling_width, subsampling_height);
    goto error;
  }
  if (dilation_width == 0 || dilation_height == 0) {
    qnnp_log_error("cannot create convolution with %" PRIu32 "x%" PRIu32 " dilation: dilation dimensions may not be zero",
        dilation_width, dilation_height);
    goto error;
  }
  if (!scale_is_valid(input_scale)) {
    qnnp_log_error("cannot create convolution with %.7g input scale: a scale has to be a finite number above zero", input_scale);
    goto error;
  }
  if (per_channel ? kernel_scales == NULL : !scale_is_valid(kernel_scale)) {
    if (per_channel) {
      qnnp_log_error("cannot create convolution: the array of kernel scales may not be NULL");
    } else {
      qnnp_log_error("cannot create convolution with %.7g kernel scale: a scale has to be a finite number above zero", kernel_scale);
    }
    goto error;
  }
  if (!scale_is_valid(output_scale)) {
    qnnp_log_error("cannot create convolution with %.7g output scale: a scale has to be a finite number above zero", output_scale);
    goto error;
  }
  if (groups == 0 || group_input_channels == 0 || group_output_channels == 0 || kernel == NULL || bias == NULL) {
    qnnp_log_error("cannot create convolution: groups, channel counts, kernel and bias may not be zero");
    goto error;
  }
  const size_t output_channels = (size_t) groups * group_output_channels;
  if (per_channel) {
    const size_t bad = qnnp_per_channel_first_invalid(kernel_scales, output_channels);
    if (bad != output_channels) {
      qnnp_log_error("cannot create convolution with %.7g kernel scale of channel %zu: a scale has to be a finite number above zero",
          kernel_scales[bad], bad);
      goto error;
    }
  }

  /* reference convolution.c:117-168 (the "inefficiency" notes are informational there) */
  status = qnnp_status_unsupported_parameter;
  float convolution_scale = 0.0f;
  if (per_channel) {
    const size_t bad = qnnp_per_channel_first_unsupported(input_scale, kernel_scales, output_scale, output_channels);
    if (bad != output_channels) {
      qnnp_log_error(
          "cannot create convolution with %.7g input scale, %.7g kernel scale of channel %zu, and %.7g output scale: "
          "convolution scale %.7g is outside [2**-32, 1.0)",
          input_scale, kernel_scales[bad], bad, output_scale,
          qnnp_per_channel_scale(input_scale, kernel_scales[bad], output_scale));
      goto error;
    }
    /* (what op->requant carries beside the zero point and the clamp: the largest channel scale) */
    for (size_t c = 0; c < output_channels; c++) {
      const float scale = qnnp_per_channel_scale(input_scale, kernel_scales[c], output_scale);
      if (scale > convolution_scale) convolution_scale = scale;
    }
  } else {
    convolution_scale = input_scale * kernel_scale / output_scale;
  }
  if (convolution_scale >= 1.0f) {
    qnnp_log_error(
        "cannot create convolution with %.7g input scale, %.7g kernel scale, and %.7g output scale: "
        "convolution scale %.7g is greater or equal to 1.0",
        input_scale, kernel_scale, output_scale, convolution_scale);
    goto error;
  }
  if (!(convolution_scale >= 0x1.0p-32f)) {
    /* the reference's parameter builder asserts this range (requantization.h:28, :139) */
    qnnp_log_error("cannot create convolution: convolution scale %.7g is below 2**-32", convolution_scale);
    goto error;
  }
  const size_t kernel_size = (size_t) kernel_height * kernel_width;
  if (kernel_size * group_input_channels > (size_t) UINT32_MAX / 4 ||
      (size_t) groups * group_output_channels > (size_t) UINT32_MAX / 4) {
    qnnp_log_error("cannot create convolution: channel / kernel extents exceed the 32-bit index range of the device kernels");
    goto error;
  }

  /*
   * 2. Operator-type selection. Reference convolution.c:180-189 sends 3x3 / 5x5
   * depthwise to dwconv, unpadded stride-1 1x1 to gemm and the rest to conv.
   * The device depthwise kernel is not limited to 9 or 25 taps, so every
   * depthwise convolution (one input and one output channel per group) takes
   * it; results are identical, only the kernel differs.
   */
  const bool any_padding =
      (input_padding_left | input_padding_top | input_padding_right | input_padding_bottom) != 0;
  enum qnnp_ukernel_type ukernel_type = qnnp_ukernel_type_conv;
  if (group_input_channels == 1 && group_output_channels == 1 && groups > 1) {
    ukernel_type = qnnp_ukernel_type_dwconv;
  } else if (kernel_size == 1 && subsampling_height == 1 && subsampling_width == 1 && !any_padding) {
    ukernel_type = qnnp_ukernel_type_gemm;
  }

  status = qnnp_status_out_of_memory;
  op = qnnp_allocate_operator(ukernel_type, ukernel_type == qnnp_ukernel_type_dwconv ? launch_dwconv : qnnp_igemm_launch);
  if (op == NULL) {
    goto error;
  }
  op->input_padding_top = input_padding_top;
  op->input_padding_right = input_padding_right;
  op->input_padding_bottom = input_padding_bottom;
  op->input_padding_left = input_padding_left;
  op->kernel_height = kernel_height;
  op->kernel_width = kernel_width;
  op->stride_height = subsampling_height;
  op->stride_width = subsampling_width;
  op->dilation_height = dilation_height;
  op->dilation_width = dilation_width;
  op->groups = groups;
  op->group_input_channels = group_input_channels;
  op->group_output_channels = group_output_channels;
  op->input_zero_point = input_zero_point;
  op->kernel_zero_point = kernel_zero_point;
  op->per_channel = per_channel;
  op->requant = qnnp_compute_requant(convolution_scale, output_zero_point, output_min, output_max);
  op->requant.accumulator_bits = qnnp_accumulator_bits(bias, (size_t) groups * group_output_channels,
      kernel_size * group_input_channels);

  /* 3. / 4. the device images */
  status = ukernel_type == qnnp_ukernel_type_dwconv ? pack_depthwise(op, kernel, bias) : pack_gemm(op, kernel, bias);
  if (status != qnnp_status_success) {
    goto error;
  }
  if (per_channel) {
    /* one entry per output channel, padded to the kernels' channel pad: c_pad for depthwise (its "groups" are channels of
     * one run), n_pad per group for the GEMM image */
    op->d_requant_pc = ukernel_type == qnnp_ukernel_type_dwconv
        ? qnnp_per_channel_upload_table(1, groups, op->c_pad, input_scale, kernel_scales, output_scale)
        : qnnp_per_channel_upload_table(groups, group_output_channels, op->n_pad, input_scale, kernel_scales, output_scale);
    if (op->d_requant_pc == NULL) {
      status = qnnp_status_out_of_memory;
      goto error;
    }
  }

  /* reference convolution.c:372: the handle is written only on success */
  *convolution_out = op;
  return qnnp_status_success;

error:
  qnnp_delete_operator(op);
  return status;
}

static enum qnnp_status qnnp_setup_convolution2d_nhwc_q8_impl(
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
  (void) threadpool; /* unused by the reference's setup too (convolution.c:389) */

  if (op->transposed || op->kernel_height == 0 ||
      (op->ukernel_type != qnnp_ukernel_type_conv && op->ukernel_type != qnnp_ukernel_type_dwconv &&
       op->ukernel_type != qnnp_ukernel_type_gemm)) {
    return qnnp_status_invalid_parameter;   /* not a handle from qnnp_create_convolution2d_nhwc_q8 */
  }

  /* reference convolution.c:396-399 */
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }

  /* reference convolution.c:401-407 */
  if (input_width == 0 || input_height == 0) {
    qnnp_log_error("cannot set up convolution with %zux%zu input: input dimensions may not be zero",
        input_width, input_height);
    return qnnp_status_invalid_parameter;
  }
  const size_t in_channels = (size_t) op->groups * op->group_input_channels;
  const size_t out_channels = (size_t) op->groups * op->group_output_channels;
  if (input == NULL || output == NULL || input_pixel_stride < in_channels || output_pixel_stride < out_channels) {
    qnnp_log_error("cannot set up convolution: NULL tensor or pixel stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  const size_t eff_kh = (size_t) (op->kernel_height - 1) * op->dilation_height + 1;
  const size_t eff_kw = (size_t) (op->kernel_width - 1) * op->dilation_width + 1;
  if (op->input_padding_top + input_height + op->input_padding_bottom < eff_kh ||
      op->input_padding_left + input_width + op->input_padding_right < eff_kw) {
    qnnp_log_error("cannot set up convolution with %zux%zu input: padded input is smaller than the dilated kernel",
        input_width, input_height);
    return qnnp_status_invalid_parameter;
  }

  /* reference convolution.c:409-426 */
  op->setup_valid = 0;   /* until every check, allocation and upload below has succeeded */
  op->residual = NULL;   /* an attached residual add belongs to the previous binding (residual.c) */
  op->dw_plan.key = 0;   /* depthwise launch plan: recomputed at the next run */
  op->batch_size = batch_size;
  op->input_height = input_height;
  op->input_width = input_width;
  op->input = input;
  op->input_pixel_stride = input_pixel_stride;
  op->output_height = compute_output_dimension(
      op->input_padding_top + input_height + op->input_padding_bottom,
      op->kernel_height, op->dilation_height, op->stride_height);
  op->output_width = compute_output_dimension(
      op->input_padding_left + input_width + op->input_padding_right,
      op->kernel_width, op->dilation_width, op->stride_width);
  op->output = output;
  op->output_pixel_stride = output_pixel_stride;

  const size_t output_size = op->output_height * op->output_width;
  const size_t input_size = input_height * input_width;
  if (batch_size * output_size > (size_t) UINT32_MAX / 2 || input_size * input_pixel_stride > (size_t) INT32_MAX) {
    qnnp_log_error("cannot set up convolution: %zu output pixels / %zu-byte images exceed the device kernels' index range",
        batch_size * output_size, input_size * input_pixel_stride);
    return qnnp_status_unsupported_parameter;
  }

  op->input_span = (batch_size * input_size - 1) * input_pixel_stride + in_channels;
  op->output_span = (batch_size * output_size - 1) * output_pixel_stride + out_channels;
  const enum qnnp_status bound = qnnp_bind_tensors(op, "qnnp_setup_convolution2d_nhwc_q8");
  if (bound != qnnp_status_success) {
    return bound;
  }

  switch (op->ukernel_type) {
    case qnnp_ukernel_type_gemm:
      /* maps directly to GEMM, no table (reference convolution.c:429-431) */
      op->variant = qnnp_state.opt_gemm_kernel;
      return qnnp_status_success;
    case qnnp_ukernel_type_dwconv:
      /* the depthwise kernels derive tap coordinates arithmetically */
      op->variant = qnnp_state.opt_dwconv_kernel;
      return qnnp_status_success;
    case qnnp_ukernel_type_conv:
    {
      op->variant = qnnp_state.opt_gemm_kernel;
      const size_t kernel_size = (size_t) op->kernel_height * op->kernel_width;
      const size_t entries = output_size * kernel_size;
      const bool same_geometry = op->d_offsets != NULL &&
          op->offsets_in_h == input_height && op->offsets_in_w == input_width &&
          op->offsets_in_stride == input_pixel_stride;
      if (same_geometry) {
        return qnnp_status_success;  /* table is pointer- and batch-invariant */
      }
      const size_t bytes = sizeof(int32_t) * entries;
      int32_t* host_table = (int32_t*) malloc(bytes);
      if (host_table == NULL) {
        qnnp_log_error("out of host memory: %zu bytes for the offset table", bytes);
        return qnnp_status_out_of_memory;
      }
      qnnp_indirection_init_conv2d_offsets(op, host_table);
      /* (+ 16 bytes: the 3-channel streaming kernel reads a lane's four consecutive entries with one 16-byte
       *  load, which for the last pixel's second K block starts on its 9th entry and runs past the table) */
      const int uploaded = qnnp_upload_table((void**) &op->d_offsets, &op->offsets_capacity, entries, bytes + 16, host_table, bytes);
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
    default:
      return qnnp_status_invalid_parameter;
  }
}

/* ---- public entry points: the implementations above inside the device guards of lifecycle.h ---- */

enum qnnp_status qnnp_create_convolution2d_nhwc_q8(
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t kernel_height,
    uint32_t kernel_width,
    uint32_t subsampling_height,
    uint32_t subsampling_width,
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
    qnnp_operator_t* convolution_out)
{
  int token;
  const enum qnnp_status status = qnnp_enter_create("qnnp_create_convolution2d_nhwc_q8", &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token,
      qnnp_create_convolution2d_nhwc_q8_impl(0, NULL, input_padding_top, input_padding_right, input_padding_bottom,
          input_padding_left, kernel_height, kernel_width, subsampling_height, subsampling_width, dilation_height,
          dilation_width, groups, group_input_channels, group_output_channels, input_zero_point, input_scale,
          kernel_zero_point, kernel_scale, kernel, bias, output_zero_point, output_scale, output_min, output_max,
          flags, convolution_out));
}

enum qnnp_status qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t kernel_height,
    uint32_t kernel_width,
    uint32_t subsampling_height,
    uint32_t subsampling_width,
    uint32_t dilation_height,
    uint32_t dilation_width,
    uint32_t groups,
    size_t group_input_channels,
    size_t group_output_channels,
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
    qnnp_operator_t* convolution_out)
{
  int token;
  const enum qnnp_status status = qnnp_enter_create("qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel", &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token,
      qnnp_create_convolution2d_nhwc_q8_impl(1, kernel_scales, input_padding_top, input_padding_right,
          input_padding_bottom, input_padding_left, kernel_height, kernel_width, subsampling_height, subsampling_width,
          dilation_height, dilation_width, groups, group_input_channels, group_output_channels, input_zero_point,
          input_scale, kernel_zero_point, 0.0f, kernel, bias, output_zero_point, output_scale, output_min, output_max,
          flags, convolution_out));
}

enum qnnp_status qnnp_setup_convolution2d_nhwc_q8(
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
  const enum qnnp_status status = qnnp_enter_setup("qnnp_setup_convolution2d_nhwc_q8", op, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(op, token,
      qnnp_setup_convolution2d_nhwc_q8_impl(op, batch_size, input_height, input_width, input, input_pixel_stride,
          output, output_pixel_stride, threadpool));
}
