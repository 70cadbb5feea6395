/*
 * dynamic-fully-connected.c -- qnnp_gfx950_create_fully_connected_nc_f32_qd8[_qc4w, _qb4w, _qb4w_zp, _qb4w_b32, _mxfp4w] / qnnp_gfx950_setup_fully_connected_nc_f32_qd8 and their GROUPED forms
 * (include/qnnpack_gfx950_dynamic.h has the arithmetic and the statuses): float32 rows in, float32 rows out, each input row
 * quantized to its own range on the device and multiplied with int8 or 4-bit weights on the matrix cores.
 *
 * No reference counterpart. Create packs the weights into the fragment image of hip/qd8f32gemm.hip (4-bit weights: the
 * pair-fragment image of hip/qd8f32gemm4.hip; the operator remembers the width, nothing else differs) and uploads one table
 * entry per output channel -- for block-wise 4-bit scales also one per channel and block, the block table of hip/qd8f32gemm4b.hip, and with
 * per-block zero points the block table and the zero-point pair table of hip/qd8f32gemm4z.hip, for blocks of 32 the image and the two pair-indexed tables of hip/qd8f32gemm4s.hip, for MXFP4 weights that image with the raw codes and the one table of hip/qd8f32gemm4m.hip -- (as per-channel.h does for the per-channel operators); setup follows quantize.c -- validation
 * in the documented order, every check before the operator changes -- and grows the one device scratch the operator owns
 * (as squeeze-excite.c owns its gate rows; freed by qnnp_delete_operator). The run is two launches, reached through
 * op->launch: the rows kernel of hip/f32qd8rows.hip into the scratch, then the GEMM or GEMV kernel out of it. The scratch
 * needs no clearing when it grows: the rows kernel writes every byte the second launch reads, the K pad included.
 *
 * The GROUPED create (qnnp_gfx950_create_grouped_fully_connected_nc_f32_qd8_mxfp4w) keeps `groups` MXFP4 weight sets in one
 * operator: that many images and tables, one behind the other, written by the packers of the _mxfp4w create. Its setup takes a
 * device array of group ids, one per output row, which the launches read when they run; the scratch then also holds the
 * permutation, the tile list and the tile count of hip/qd8f32gemm4g.hip, and the run is three launches: the rows kernel over
 * the INPUT rows, that unit's plan kernel, and its product kernel on a grid fixed here, before any id is known.
 *
 * The two _gated setups (qnnp_gfx950_setup_[grouped_]fully_connected_nc_f32_qd8_gated) take any of these handles with input
 * rows of K PAIRS {gate, up}: they share their bodies with the plain setups (the floats per input row are a parameter), the
 * operator remembers the gate, and launch_rows sends the first launch to hip/f32qd8gatedrows.hip, which quantizes
 * act(gate) * up without writing it as floats. Nothing behind the first launch knows.
 *
 * The two _rmsnorm setups (qnnp_gfx950_setup_[grouped_]fully_connected_nc_f32_qd8_rmsnorm) are the first layer's counterpart:
 * the same bodies again with a struct qd8_norm, the operator remembers gamma, epsilon and the residual pair, and launch_rows
 * sends the first launch to hip/f32qd8rmsnormrows.hip, which quantizes rmsnorm(input + residual) * gamma without writing it
 * as floats and writes the sum back as the residual stream. K is at most 16384 there, and every tensor is device memory.
 *
 * Not part of the seam library (oracle/Makefile).
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <qnnpack.h>
#include <qnnpack_gfx950_dynamic.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "state.h"
#include "upload.h"

#define QNNP_QD8_MAX_INPUT_CHANNELS ((size_t) 32768)          /* K * 255 * 128 stays below 2^31 */
#define QNNP_QD8_MAX_NORM_CHANNELS ((size_t) 16384)           /* the rmsnorm setups: a row stays in a workgroup's registers */
#define QNNP_QD8_MAX_OUTPUT_CHANNELS ((size_t) 1 << 24)       /* exclusive */
#define QNNP_QD8_MAX_GROUPS ((size_t) 1024)                   /* the plan kernel has one thread per group */
#define QNNP_QD8_MAX_ASSIGNMENTS ((size_t) 8)
#define QNNP_QD8_MAX_GROUPED_ROWS ((size_t) 1 << 20)          /* exclusive: output rows of the grouped operator */
#define QNNP_QD8_MAX_GATHER_BYTES ((size_t) 1 << 31)          /* the grouped kernels' 32-bit offset of a gathered row */

/* the first launch of either form: op->batch_size input rows into the scratch, by the plain, the gated or the rmsnorm row
 * kernels as the current setup says */
static int launch_rows(struct qnnp_operator* op, const void* input, int8_t* quantized, struct qnnp_hip_qd8_row_entry* row_table)
{
  if (op->qd8_gated) {
    const struct qnnp_hip_qd8_gated_rows_args gated_args = {
      .input = (const float*) input,
      .quantized = quantized,
      .row_table = row_table,
      .rows = (uint32_t) op->batch_size,
      .k = (uint32_t) op->group_input_channels,
      .k_pad = op->k_pad,
      .input_stride = op->input_pixel_stride,
      .alpha = op->qd8_gate_alpha,
      .limit = op->qd8_gate_limit,
      .up_shift = op->qd8_gate_up_shift,
    };
    return qnnp_hip_qd8_gated_rows_run(&gated_args, &op->qd8_rows_kernel);
  }
  if (op->qd8_rmsnorm) {
    const struct qnnp_hip_qd8_rmsnorm_rows_args norm_args = {
      .input = (const float*) input,
      .quantized = quantized,
      .row_table = row_table,
      .rows = (uint32_t) op->batch_size,
      .k = (uint32_t) op->group_input_channels,
      .k_pad = op->k_pad,
      .input_stride = op->input_pixel_stride,
      .gamma = op->qd8_norm_gamma,
      .residual = op->qd8_norm_residual,
      .residual_out = op->qd8_norm_residual_out,
      .residual_stride = op->qd8_norm_residual_stride,
      .epsilon = op->qd8_norm_epsilon,
    };
    return qnnp_hip_qd8_rmsnorm_rows_run(&norm_args, &op->qd8_rows_kernel);
  }
  const struct qnnp_hip_qd8_rows_args rows_args = {
    .input = (const float*) input,
    .quantized = quantized,
    .row_table = row_table,
    .rows = (uint32_t) op->batch_size,
    .k = (uint32_t) op->group_input_channels,
    .k_pad = op->k_pad,
    .input_stride = op->input_pixel_stride,
  };
  return qnnp_hip_qd8_rows_run(&rows_args, &op->qd8_rows_kernel);
}

static int launch_dynamic_fully_connected(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  int8_t* quantized = (int8_t*) op->d_qd8_scratch;
  struct qnnp_hip_qd8_row_entry* row_table =
      (struct qnnp_hip_qd8_row_entry*) ((uint8_t*) op->d_qd8_scratch + op->qd8_row_table_offset);
  const int rc = launch_rows(op, input, quantized, row_table);
  if (rc != QNNP_HIP_OK) {
    return rc;
  }
  const struct qnnp_hip_qd8_gemm_args gemm_args = {
    .quantized = quantized,
    .row_table = row_table,
    .packed_w = (const int8_t*) op->d_weights,
    .channel_table = (const struct qnnp_hip_qd8_channel_entry*) op->d_qd8_channels,
    .output = (float*) output,
    .rows = (uint32_t) op->batch_size,
    .n = (uint32_t) op->channels,
    .n_pad = op->n_pad,
    .k_pad = op->k_pad,
    .output_stride = op->output_pixel_stride,
    .output_min = op->f32_output_min,
    .output_max = op->f32_output_max,
  };
  if (op->qd8_mxfp4 != 0) {
    const struct qnnp_hip_qd8_mxfp4w_gemm_args mx_args = {
      .gemm = gemm_args,
      .block_table = (const int32_t*) op->d_qd8_blocks,
    };
    return qnnp_hip_qd8_mxfp4w_gemm_run(&mx_args, &op->kernel_name);
  }
  if (op->qd8_block_size == 32) {
    const size_t scale_bytes = (size_t) op->n_pad * ((op->k_pad + 127u) / 128u) * 4 * sizeof(float);
    const struct qnnp_hip_qd8_qb4w_b32_gemm_args b32_args = {
      .gemm = gemm_args,
      .block_scales = (const float*) op->d_qd8_blocks,
      .block_sums = (const int16_t*) ((const uint8_t*) op->d_qd8_blocks + scale_bytes),
    };
    return qnnp_hip_qd8_qb4w_b32_gemm_run(&b32_args, &op->kernel_name);
  }
  if (op->qd8_zero_points != 0) {
    const size_t table_bytes =
        (size_t) op->n_pad * (op->k_pad / op->qd8_block_size) * sizeof(struct qnnp_hip_qd8_zp_block_entry);
    const struct qnnp_hip_qd8_qb4w_zp_gemm_args zp_args = {
      .gemm = gemm_args,
      .block_table = (const struct qnnp_hip_qd8_zp_block_entry*) op->d_qd8_blocks,
      .zero_point_pairs = (const uint16_t*) ((const uint8_t*) op->d_qd8_blocks + table_bytes),
      .block_size = op->qd8_block_size,
    };
    return qnnp_hip_qd8_qb4w_zp_gemm_run(&zp_args, &op->kernel_name);
  }
  if (op->qd8_block_size != 0) {
    const struct qnnp_hip_qd8_qb4w_gemm_args block_args = {
      .gemm = gemm_args,
      .block_table = (const struct qnnp_hip_qd8_block_entry*) op->d_qd8_blocks,
      .block_size = op->qd8_block_size,
    };
    return qnnp_hip_qd8_qb4w_gemm_run(&block_args, &op->kernel_name);
  }
  return op->qd8_weight_bits == 4 ? qnnp_hip_qd8_qc4w_gemm_run(&gemm_args, &op->kernel_name)
                                  : qnnp_hip_qd8_gemm_run(&gemm_args, &op->kernel_name);
}

/* the grouped operator: op->batch_size INPUT rows, qd8_assignments output rows each */
static int launch_grouped_fully_connected(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  uint8_t* scratch = (uint8_t*) op->d_qd8_scratch;
  struct qnnp_hip_qd8_row_entry* row_table = (struct qnnp_hip_qd8_row_entry*) (scratch + op->qd8_row_table_offset);
  const int rc = launch_rows(op, input, (int8_t*) scratch, row_table);
  if (rc != QNNP_HIP_OK) {
    return rc;
  }
  const struct qnnp_hip_qd8_mxfp4w_grouped_args args = {
    .quantized = (const int8_t*) scratch,
    .row_table = row_table,
    .packed_w = (const int8_t*) op->d_weights,
    .block_table = (const int32_t*) op->d_qd8_blocks,
    .bias = (const float*) op->d_qd8_channels,
    .group_ids = op->qd8_group_ids,
    .perm = (uint32_t*) (scratch + op->qd8_perm_offset),
    .tiles = (struct qnnp_hip_qd8_grouped_tile*) (scratch + op->qd8_tiles_offset),
    .tile_count = (uint32_t*) (scratch + op->qd8_tile_count_offset),
    .output = (float*) output,
    .rows = (uint32_t) (op->batch_size * op->qd8_assignments),
    .assignments = op->qd8_assignments,
    .groups = op->qd8_groups,
    .tile_rows = op->qd8_tile_rows,
    .max_tiles = op->qd8_max_tiles,
    .n = (uint32_t) op->channels,
    .n_pad = op->n_pad,
    .k_pad = op->k_pad,
    .output_stride = op->output_pixel_stride,
    .output_min = op->f32_output_min,
    .output_max = op->f32_output_max,
  };
  return qnnp_hip_qd8_mxfp4w_grouped_run(&args, &op->kernel_name);
}

/* weight (c, k) of either kernel layout: int8 [n][k], or nibbles [n][(k + 1) / 2] with position k in bits
 * 4 (k % 2) .. 4 (k % 2) + 3 of byte k / 2, two's complement */
static inline int32_t weight_at(const void* kernel, uint32_t bits, size_t k_total, size_t c, size_t k)
{
  if (bits == 8) {
    return ((const int8_t*) kernel)[c * k_total + k];
  }
  const uint32_t nibble = (((const uint8_t*) kernel)[c * ((k_total + 1) / 2) + k / 2] >> (4 * (k % 2))) & 15u;
  return (int32_t) (nibble ^ 8u) - 8;
}

/* The fragment image (hip/qnnp_hip.h): for channel block nb and K tile kt, lane l of fragment nb * ktiles + kt holds the
 * sixteen weights of channel nb * 16 + l % 16 at K positions kt * 64 + (l / 16) * 16 .. + 15; padding is zero. */
static void pack_weights(size_t k, size_t n, uint32_t k_pad, uint32_t n_pad, const int8_t* kernel, int8_t* packed)
{
  const size_t ktiles = k_pad / 64;
  for (size_t nb = 0; nb < n_pad / 16; nb++) {
    for (size_t kt = 0; kt < ktiles; kt++) {
      int8_t* fragment = packed + (nb * ktiles + kt) * 1024;
      for (size_t l = 0; l < 64; l++) {
        const size_t c = nb * 16 + l % 16;
        const size_t k0 = kt * 64 + (l / 16) * 16;
        for (size_t j = 0; j < 16; j++) {
          fragment[l * 16 + j] = c < n && k0 + j < k ? kernel[c * k + k0 + j] : 0;
        }
      }
    }
  }
}

/* The pair-fragment image (hip/qnnp_hip.h): for channel block nb and K-tile pair kp, byte j of lane l of fragment
 * nb * kpairs + kp holds two weights of channel nb * 16 + l % 16: K position kp * 128 + (l / 16) * 16 + j in its low
 * nibble and that position plus 64 in its high nibble; padding is zero. */
static void pack_weights_qc4w(size_t k, size_t n, uint32_t k_pad4, uint32_t n_pad, const uint8_t* kernel, uint8_t* packed)
{
  const size_t kpairs = k_pad4 / 128;
  for (size_t nb = 0; nb < n_pad / 16; nb++) {
    for (size_t kp = 0; kp < kpairs; kp++) {
      uint8_t* fragment = packed + (nb * kpairs + kp) * 1024;
      for (size_t l = 0; l < 64; l++) {
        const size_t c = nb * 16 + l % 16;
        const size_t k0 = kp * 128 + (l / 16) * 16;
        for (size_t j = 0; j < 16; j++) {
          const uint32_t low = c < n && k0 + j < k ? (uint32_t) weight_at(kernel, 4, k, c, k0 + j) & 15u : 0u;
          const uint32_t high = c < n && k0 + 64 + j < k ? (uint32_t) weight_at(kernel, 4, k, c, k0 + 64 + j) & 15u : 0u;
          fragment[l * 16 + j] = (uint8_t) (low | (high << 4));
        }
      }
    }
  }
}

/* The block table (hip/qnnp_hip.h): entry ((c / 16) * nblk + b) * 16 + c % 16 = {kernel_scales[c][b] / 16 -- exact, the
 * scale is at least 2^-16 --, 16 * the sum of the block's weights, at most 16 * 8 * 256 in magnitude}; padding channels
 * {1 / 16, 0}. */
static void fill_block_table(size_t k, size_t n, uint32_t n_pad, size_t block_size, const uint8_t* kernel,
                             const float* kernel_scales, struct qnnp_hip_qd8_block_entry* table)
{
  const size_t nblk = k / block_size;
  for (size_t c = 0; c < n_pad; c++) {
    for (size_t b = 0; b < nblk; b++) {
      struct qnnp_hip_qd8_block_entry* entry = &table[((c / 16) * nblk + b) * 16 + c % 16];
      *entry = (struct qnnp_hip_qd8_block_entry) { .s16 = 0.0625f, .wsum16 = 0 };
      if (c < n) {
        int32_t wsum = 0;
        for (size_t i = b * block_size; i < (b + 1) * block_size; i++) {
          wsum += weight_at(kernel, 4, k, c, i);
        }
        entry->s16 = kernel_scales[c * nblk + b] * 0.0625f;
        entry->wsum16 = 16 * wsum;
      }
    }
  }
}

/* The two tables of the _qb4w_zp create (hip/qnnp_hip.h), in one allocation. `kernel` holds UNSIGNED nibbles u. The block
 * table: entry ((c / 16) * nblk + b) * 16 + c % 16 = {kernel_scales[c][b], the sum of u - z over the block, at most 15 * 256
 * in magnitude}; padding channels {1, 0}. Behind it the zero-point pair table: uint16 ((c / 16) * kpairs + kp) * 16 + c % 16 =
 * the zero point of the block of K tile 2 kp in the low byte and of K tile 2 kp + 1 in the high byte; zero for padding
 * channels and for a tile past K. */
static void fill_block_table_zp(size_t k, size_t n, uint32_t n_pad, uint32_t k_pad4, size_t block_size, const uint8_t* kernel,
                                const float* kernel_scales, const uint8_t* kernel_zero_points,
                                struct qnnp_hip_qd8_zp_block_entry* table)
{
  const size_t nblk = k / block_size, kpairs = k_pad4 / 128;
  uint16_t* pairs = (uint16_t*) (table + (size_t) n_pad * nblk);
  for (size_t c = 0; c < n_pad; c++) {
    for (size_t b = 0; b < nblk; b++) {
      struct qnnp_hip_qd8_zp_block_entry* entry = &table[((c / 16) * nblk + b) * 16 + c % 16];
      *entry = (struct qnnp_hip_qd8_zp_block_entry) { .scale = 1.0f, .wsum = 0 };
      if (c < n) {
        int32_t usum = 0;
        for (size_t i = b * block_size; i < (b + 1) * block_size; i++) {
          usum += (kernel[c * (k / 2) + i / 2] >> (4 * (i % 2))) & 15;
        }
        entry->scale = kernel_scales[c * nblk + b];
        entry->wsum = usum - (int32_t) block_size * kernel_zero_points[c * nblk + b];
      }
    }
    for (size_t kp = 0; kp < kpairs; kp++) {
      const size_t k_even = kp * 128, k_odd = kp * 128 + 64;
      const uint32_t low = c < n ? kernel_zero_points[c * nblk + k_even / block_size] : 0u;
      const uint32_t high = c < n && k_odd < k ? kernel_zero_points[c * nblk + k_odd / block_size] : 0u;
      pairs[((c / 16) * kpairs + kp) * 16 + c % 16] = (uint16_t) (low | (high << 8));
    }
  }
}

/* The _qb4w_b32 create's image and tables (hip/qnnp_hip.h). `flip` is 0 for unsigned nibbles with `kernel_zero_points`, and 8
 * for signed nibbles w (kernel_zero_points == NULL): u = w ^ 8 with every zero point 8 has the same u - z. */
static inline uint32_t nibble_b32(const uint8_t* kernel, uint32_t flip, size_t k_total, size_t c, size_t k)
{
  return ((kernel[c * (k_total / 2) + k / 2] >> (4 * (k % 2))) & 15u) ^ flip;
}

/* The block-32 pair-fragment image: byte j of lane l of fragment nb * kpairs + kp holds two weights of channel
 * nb * 16 + l % 16: K position kp * 128 + (j / 8) * 32 + (l / 16) * 8 + j % 8 in its low nibble and that position plus 64 in
 * its high nibble; padding is zero. Bytes 0 .. 7 of a lane lie in the first 32-block of either K tile, bytes 8 .. 15 in the
 * second. */
static void pack_weights_qb4w_b32(size_t k, size_t n, uint32_t k_pad4, uint32_t n_pad, const uint8_t* kernel, uint32_t flip,
                                  uint8_t* packed)
{
  const size_t kpairs = k_pad4 / 128;
  for (size_t nb = 0; nb < n_pad / 16; nb++) {
    for (size_t kp = 0; kp < kpairs; kp++) {
      uint8_t* fragment = packed + (nb * kpairs + kp) * 1024;
      for (size_t l = 0; l < 64; l++) {
        const size_t c = nb * 16 + l % 16;
        for (size_t j = 0; j < 16; j++) {
          const size_t k0 = kp * 128 + (j / 8) * 32 + (l / 16) * 8 + j % 8;
          const uint32_t low = c < n && k0 < k ? nibble_b32(kernel, flip, k, c, k0) : 0u;
          const uint32_t high = c < n && k0 + 64 < k ? nibble_b32(kernel, flip, k, c, k0 + 64) : 0u;
          fragment[l * 16 + j] = (uint8_t) (low | (high << 4));
        }
      }
    }
  }
}

/* The two tables of the _qb4w_b32 create (hip/qnnp_hip.h), in one allocation, entry ((c / 16) * kpairs + kp) * 16 + c % 16 of
 * either: four scales (1 for padding channels and blocks past K), and behind all of them four int16 of 16 * wsum + z with
 * wsum the block's sum of u - z, at most 15 * 32 in magnitude (0 for padding channels and blocks past K). */
static void fill_tables_b32(size_t k, size_t n, uint32_t n_pad, uint32_t k_pad4, const uint8_t* kernel, uint32_t flip,
                            const float* kernel_scales, const uint8_t* kernel_zero_points, float* scales)
{
  const size_t nblk = k / 32, kpairs = k_pad4 / 128;
  int16_t* sums = (int16_t*) (scales + (size_t) n_pad * kpairs * 4);
  for (size_t c = 0; c < n_pad; c++) {
    for (size_t b = 0; b < kpairs * 4; b++) {
      const size_t at = (((c / 16) * kpairs + b / 4) * 16 + c % 16) * 4 + b % 4;
      scales[at] = 1.0f;
      sums[at] = 0;
      if (c < n && b < nblk) {
        const int32_t z = kernel_zero_points != NULL ? kernel_zero_points[c * nblk + b] : 8;
        int32_t wsum = 0;
        for (size_t i = b * 32; i < (b + 1) * 32; i++) {
          wsum += (int32_t) nibble_b32(kernel, flip, k, c, i) - z;
        }
        scales[at] = kernel_scales[c * nblk + b];
        sums[at] = (int16_t) (16 * wsum + z);
      }
    }
  }
}

/* Twice the value of an E2M1 code: sign in bit 3, magnitude index in bits 0 .. 2 into {0, 0.5, 1, 1.5, 2, 3, 4, 6} */
static const int8_t mxfp4_w2[16] = { 0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12 };

/* The one table of the _mxfp4w create (hip/qnnp_hip.h), entry ((c / 16) * kpairs + kp) * 16 + c % 16: four int32 of
 * 256 * wsum2 + e, wsum2 the block's sum of w2 (at most 12 * 32 in magnitude) and e its E8M0 byte; 128 (wsum2 0, the term's
 * exponent 0) for padding channels and blocks past K. */
static void fill_table_mxfp4w(size_t k, size_t n, uint32_t n_pad, uint32_t k_pad4, const uint8_t* kernel,
                              const uint8_t* kernel_scales, int32_t* table)
{
  const size_t nblk = k / 32, kpairs = k_pad4 / 128;
  for (size_t c = 0; c < n_pad; c++) {
    for (size_t b = 0; b < kpairs * 4; b++) {
      const size_t at = (((c / 16) * kpairs + b / 4) * 16 + c % 16) * 4 + b % 4;
      table[at] = 128;
      if (c < n && b < nblk) {
        int32_t wsum2 = 0;
        for (size_t i = b * 32; i < (b + 1) * 32; i++) {
          wsum2 += mxfp4_w2[nibble_b32(kernel, 0, k, c, i)];
        }
        table[at] = 256 * wsum2 + (int32_t) kernel_scales[c * nblk + b];
      }
    }
  }
}

/* `mxfp4`: the _mxfp4w create -- block_size is 32, `kernel` holds E2M1 codes, `kernel_scales` E8M0 bytes and there are no zero
 * points; otherwise `kernel_scales` are floats */
static enum qnnp_status create_dynamic_fully_connected(
    size_t input_channels, size_t output_channels, size_t block_size, const void* kernel, uint32_t weight_bits, int mxfp4,
    const void* kernel_scales_any, const uint8_t* kernel_zero_points, const float* bias, float output_min, float output_max, qnnp_operator_t* fully_connected)
{
  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_dynamic_fully_connected, launch_dynamic_fully_connected);
  if (op == NULL) {
    return qnnp_status_out_of_memory;
  }
  const float* kernel_scales = mxfp4 ? NULL : (const float*) kernel_scales_any;
  const uint32_t k_pad = ((uint32_t) input_channels + 63u) & ~63u;
  const uint32_t n_pad = ((uint32_t) output_channels + 15u) & ~15u;
  const uint32_t k_pad4 = ((uint32_t) input_channels + 127u) & ~127u;       /* whole K-tile pairs */
  const size_t w_bytes = weight_bits == 4 ? (size_t) n_pad * (k_pad4 / 2) : (size_t) n_pad * k_pad;
  const size_t t_bytes = (size_t) n_pad * sizeof(struct qnnp_hip_qd8_channel_entry);
  /* block-wise scales: one more table (with zero points: eight bytes per entry as well, and the pair table behind it);
   * without them a token byte, so that one test serves every allocation */
  const size_t b_bytes = block_size == 0 ? 1
      : mxfp4 ? (size_t) n_pad * (k_pad4 / 128) * (4 * sizeof(int32_t))
      : block_size == 32 ? (size_t) n_pad * (k_pad4 / 128) * (4 * sizeof(float) + 4 * sizeof(int16_t))
      : (size_t) n_pad * (input_channels / block_size) * sizeof(struct qnnp_hip_qd8_block_entry)
          + (kernel_zero_points != NULL ? (size_t) n_pad * (k_pad4 / 128) * sizeof(uint16_t) : 0);
  int8_t* packed = (int8_t*) malloc(w_bytes);
  struct qnnp_hip_qd8_channel_entry* table = (struct qnnp_hip_qd8_channel_entry*) malloc(t_bytes);
  struct qnnp_hip_qd8_block_entry* blocks = (struct qnnp_hip_qd8_block_entry*) malloc(b_bytes);
  if (packed != NULL && table != NULL && blocks != NULL) {
    /* block size 32 alone: signed nibbles become unsigned; E2M1 codes travel as they are */
    const uint32_t flip = kernel_zero_points == NULL && !mxfp4 ? 8u : 0u;
    if (block_size == 32) {
      pack_weights_qb4w_b32(input_channels, output_channels, k_pad4, n_pad, (const uint8_t*) kernel, flip, (uint8_t*) packed);
    } else if (weight_bits == 4) {
      pack_weights_qc4w(input_channels, output_channels, k_pad4, n_pad, (const uint8_t*) kernel, (uint8_t*) packed);
    } else {
      pack_weights(input_channels, output_channels, k_pad, n_pad, (const int8_t*) kernel, packed);
    }
    for (size_t c = 0; c < n_pad; c++) {
      /* the padding channels: valid entries whose results are never stored */
      table[c] = (struct qnnp_hip_qd8_channel_entry) { .kernel_scale = 1.0f, .bias = 0.0f, .wsum = 0 };
      if (c < output_channels && block_size != 0) {
        table[c].bias = bias != NULL ? bias[c] : 0.0f;       /* the scales and weight sums are the block table's */
      } else if (c < output_channels) {
        int32_t wsum = 0;
        for (size_t k = 0; k < input_channels; k++) {
          wsum += weight_at(kernel, weight_bits, input_channels, c, k);        /* at most 128 * 32768 in magnitude */
        }
        table[c].kernel_scale = kernel_scales[c];
        table[c].bias = bias != NULL ? bias[c] : 0.0f;
        table[c].wsum = wsum;
      }
    }
    op->d_weights = qnnp_upload(packed, w_bytes);
    op->d_qd8_channels = qnnp_upload(table, t_bytes);
    if (mxfp4) {
      fill_table_mxfp4w(input_channels, output_channels, n_pad, k_pad4, (const uint8_t*) kernel,
          (const uint8_t*) kernel_scales_any, (int32_t*) blocks);
      op->d_qd8_blocks = qnnp_upload(blocks, b_bytes);
    } else if (block_size == 32) {
      fill_tables_b32(input_channels, output_channels, n_pad, k_pad4, (const uint8_t*) kernel, flip, kernel_scales,
          kernel_zero_points, (float*) blocks);
      op->d_qd8_blocks = qnnp_upload(blocks, b_bytes);
    } else if (kernel_zero_points != NULL) {
      fill_block_table_zp(input_channels, output_channels, n_pad, k_pad4, block_size, (const uint8_t*) kernel, kernel_scales,
          kernel_zero_points, (struct qnnp_hip_qd8_zp_block_entry*) blocks);
      op->d_qd8_blocks = qnnp_upload(blocks, b_bytes);
    } else if (block_size != 0) {
      fill_block_table(input_channels, output_channels, n_pad, block_size, (const uint8_t*) kernel, kernel_scales, blocks);
      op->d_qd8_blocks = qnnp_upload(blocks, b_bytes);
    }
  } else {
    qnnp_log_error("out of host memory: %zu bytes for packed weights", w_bytes + t_bytes + b_bytes);
  }
  free(packed);
  free(table);
  free(blocks);
  if (op->d_weights == NULL || op->d_qd8_channels == NULL || (block_size != 0 && op->d_qd8_blocks == NULL)) {
    qnnp_log_error("cannot create dynamic fully connected operator: %zu bytes of packed weights could not be placed on the "
        "device", w_bytes + t_bytes);
    qnnp_delete_operator(op);
    return qnnp_status_out_of_memory;
  }
  op->group_input_channels = input_channels;
  op->channels = output_channels;          /* of the output: what operator-run.c compares the output stride with */
  op->k_pad = k_pad;
  op->n_pad = n_pad;
  op->qd8_weight_bits = weight_bits;
  op->qd8_block_size = (uint32_t) block_size;
  op->qd8_zero_points = kernel_zero_points != NULL || (block_size == 32 && !mxfp4);
  op->qd8_mxfp4 = mxfp4 ? 1 : 0;
  op->f32_output_min = output_min;
  op->f32_output_max = output_max;
  *fully_connected = op;
  return qnnp_status_success;
}

/* The grouped create's device side: per group the image of pack_weights_qb4w_b32 and the table of fill_table_mxfp4w, group
 * after group in ONE allocation each (64-bit offsets; the host holds one group's at a time), and the bias floats
 * [groups][n_pad], zero in the padding. */
static enum qnnp_status create_grouped_fully_connected(
    size_t groups, size_t input_channels, size_t output_channels, const uint8_t* kernel, const uint8_t* kernel_scales,
    const float* bias, float output_min, float output_max, qnnp_operator_t* fully_connected)
{
  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_dynamic_fully_connected, launch_grouped_fully_connected);
  if (op == NULL) {
    return qnnp_status_out_of_memory;
  }
  const uint32_t k_pad = ((uint32_t) input_channels + 63u) & ~63u;
  const uint32_t n_pad = ((uint32_t) output_channels + 15u) & ~15u;
  const uint32_t k_pad4 = ((uint32_t) input_channels + 127u) & ~127u;
  const size_t w_bytes = (size_t) n_pad * (k_pad4 / 2);
  const size_t b_bytes = (size_t) n_pad * (k_pad4 / 128) * (4 * sizeof(int32_t));
  const size_t bias_bytes = groups * n_pad * sizeof(float);
  uint8_t* packed = (uint8_t*) malloc(w_bytes);
  int32_t* blocks = (int32_t*) malloc(b_bytes);
  float* biases = (float*) calloc(groups * n_pad, sizeof(float));
  int uploaded = 0;
  if (packed != NULL && blocks != NULL && biases != NULL) {
    op->d_weights = qnnp_hip_alloc(groups * w_bytes);
    op->d_qd8_blocks = qnnp_hip_alloc(groups * b_bytes);
    uploaded = op->d_weights != NULL && op->d_qd8_blocks != NULL;
    for (size_t g = 0; uploaded && g < groups; g++) {
      const uint8_t* group_kernel = kernel + g * output_channels * (input_channels / 2);
      pack_weights_qb4w_b32(input_channels, output_channels, k_pad4, n_pad, group_kernel, 0, packed);
      fill_table_mxfp4w(input_channels, output_channels, n_pad, k_pad4, group_kernel,
          kernel_scales + g * output_channels * (input_channels / 32), blocks);
      for (size_t c = 0; bias != NULL && c < output_channels; c++) {
        biases[g * n_pad + c] = bias[g * output_channels + c];
      }
      uploaded = qnnp_hip_h2d((uint8_t*) op->d_weights + g * w_bytes, packed, w_bytes, 0) == QNNP_HIP_OK &&
          qnnp_hip_h2d((uint8_t*) op->d_qd8_blocks + g * b_bytes, blocks, b_bytes, 0) == QNNP_HIP_OK;
    }
    if (uploaded) {
      op->d_qd8_channels = qnnp_upload(biases, bias_bytes);
    }
  } else {
    qnnp_log_error("out of host memory: %zu bytes for packed weights", w_bytes + b_bytes + bias_bytes);
  }
  free(packed);
  free(blocks);
  free(biases);
  if (!uploaded || op->d_qd8_channels == NULL) {
    qnnp_log_error("cannot create grouped dynamic fully connected operator: %zu bytes of packed weights could not be placed "
        "on the device", groups * (w_bytes + b_bytes) + bias_bytes);
    qnnp_delete_operator(op);
    return qnnp_status_out_of_memory;
  }
  op->group_input_channels = input_channels;
  op->channels = output_channels;
  op->k_pad = k_pad;
  op->n_pad = n_pad;
  op->qd8_weight_bits = 4;
  op->qd8_block_size = 32;
  op->qd8_mxfp4 = 1;
  op->qd8_groups = (uint32_t) groups;
  op->f32_output_min = output_min;
  op->f32_output_max = output_max;
  *fully_connected = op;
  return qnnp_status_success;
}

/* every create: the checks in the header's order, then the packing under the device. `blockwise`: 1 for the _qb4w and
 * _qb4w_zp creates and 2 for the _qb4w_b32 create (whose block_size is 32, the one value the other two refuse), with input_channels / block_size (rounded down, where the create is going to be refused) scales per channel, each
 * in [2^-16, 2^16], and 3 for the _mxfp4w create (block_size 32 as well; `kernel_scales` are then E8M0 BYTES e, scale 2^(e - 127): 255, the format's NaN, is invalid where a float scale is when it is no normal number above zero, and a byte outside [111, 143] = [2^-16, 2^16] is unsupported); otherwise block_size is 0 and there is one scale per channel in [2^-20, 2^20]. `zero_points`: the
 * _qb4w_zp create, with as many kernel_zero_points as scales, each at most 15; otherwise kernel_zero_points is NULL.
 * `grouped`: the grouped _mxfp4w create, whose arrays hold `groups` weight sets one behind the other: every count below is
 * taken `groups` times; otherwise groups is 1. */
static enum qnnp_status create_checked(
    const char* function, int grouped, size_t groups, size_t input_channels, size_t output_channels, int blockwise, size_t block_size, const void* kernel,
    uint32_t weight_bits, const void* kernel_scales_any, int zero_points, const uint8_t* kernel_zero_points, const float* bias, float output_min, float output_max,
    qnnp_operator_t* fully_connected)
{
  const int mxfp4 = blockwise == 3;
  const float* kernel_scales = mxfp4 ? NULL : (const float*) kernel_scales_any;
  const uint8_t* e8m0 = mxfp4 ? (const uint8_t*) kernel_scales_any : NULL;
  enum qnnp_status status = qnnp_check_initialized(function);
  if (status != qnnp_status_success) {
    return status;
  }
  if (groups == 0 || input_channels == 0 || output_channels == 0 || kernel == NULL || kernel_scales_any == NULL || (blockwise && block_size == 0) ||
      (zero_points && kernel_zero_points == NULL)) {
    qnnp_log_error("cannot create dynamic fully connected operator with %zu input and %zu output channels: channel counts, "
        "block size, kernel, kernel scales and kernel zero points may not be zero", input_channels, output_channels);
    return qnnp_status_invalid_parameter;
  }
  const size_t scale_count = groups * output_channels * (blockwise ? input_channels / block_size : 1);
  const float scale_min = blockwise ? 0x1.0p-16f : 0x1.0p-20f, scale_max = blockwise ? 0x1.0p+16f : 0x1.0p+20f;
  for (size_t c = 0; mxfp4 && c < scale_count; c++) {
    if (e8m0[c] == 255) {
      qnnp_log_error("cannot create dynamic fully connected operator with E8M0 kernel scale %zu = 255: not a number", c);
      return qnnp_status_invalid_parameter;
    }
  }
  for (size_t c = 0; !mxfp4 && c < scale_count; c++) {
    if (!(kernel_scales[c] > 0.0f && isnormal(kernel_scales[c]))) {
      qnnp_log_error("cannot create dynamic fully connected operator with %.7g kernel scale %zu: a scale has to "
          "be a finite number above zero", kernel_scales[c], c);
      return qnnp_status_invalid_parameter;
    }
  }
  for (size_t c = 0; zero_points && c < scale_count; c++) {
    if (kernel_zero_points[c] > 15) {
      qnnp_log_error("cannot create dynamic fully connected operator with kernel zero point %zu = %u: a zero point of 4-bit "
          "weights is at most 15", c, (unsigned) kernel_zero_points[c]);
      return qnnp_status_invalid_parameter;
    }
  }
  for (size_t c = 0; bias != NULL && c < groups * output_channels; c++) {
    if (bias[c] != 0.0f && !isnormal(bias[c])) {
      qnnp_log_error("cannot create dynamic fully connected operator with %.7g bias of channel %zu: a bias has to be zero "
          "or a normal number", bias[c], c);
      return qnnp_status_invalid_parameter;
    }
  }
  if (isnan(output_min) || isnan(output_max) || output_min > output_max) {
    qnnp_log_error("cannot create dynamic fully connected operator with [%.7g, %.7g] output range: the bounds may not be "
        "NaN and min may not exceed max", output_min, output_max);
    return qnnp_status_invalid_parameter;
  }
  if (blockwise && ((blockwise >= 2 ? block_size != 32 : (block_size != 64 && block_size != 128 && block_size != 256)) ||
      input_channels % block_size != 0)) {
    qnnp_log_error("cannot create dynamic fully connected operator with %zu input channels in blocks of %zu: a block is 64, "
        "128 or 256 wide (32 through the _qb4w_b32 create) and divides the input channels", input_channels, block_size);
    return qnnp_status_unsupported_parameter;
  }
  for (size_t c = 0; mxfp4 && c < scale_count; c++) {
    if (e8m0[c] < 111 || e8m0[c] > 143) {
      qnnp_log_error("cannot create dynamic fully connected operator with E8M0 kernel scale %zu = %u: scale must be in "
          "[111, 143] = [2^-16, 2^16] range", c, (unsigned) e8m0[c]);
      return qnnp_status_unsupported_parameter;
    }
  }
  for (size_t c = 0; !mxfp4 && c < scale_count; c++) {
    if (!(kernel_scales[c] >= scale_min && kernel_scales[c] <= scale_max)) {
      qnnp_log_error("cannot create dynamic fully connected operator with %.7g kernel scale %zu: scale must be "
          "in [%g, %g] range", kernel_scales[c], c, scale_min, scale_max);
      return qnnp_status_unsupported_parameter;
    }
  }
  if (input_channels > QNNP_QD8_MAX_INPUT_CHANNELS || output_channels >= QNNP_QD8_MAX_OUTPUT_CHANNELS ||
      groups > QNNP_QD8_MAX_GROUPS) {
    qnnp_log_error("cannot create dynamic fully connected operator with %zu input and %zu output channels in %zu groups: at "
        "most %zu input channels (the int32 accumulator), fewer than %zu output channels and at most %zu groups",
        input_channels, output_channels, groups, QNNP_QD8_MAX_INPUT_CHANNELS, QNNP_QD8_MAX_OUTPUT_CHANNELS,
        QNNP_QD8_MAX_GROUPS);
    return qnnp_status_unsupported_parameter;
  }

  int token;
  status = qnnp_enter_for_update(qnnp_hip_device(), qnnp_status_unsupported_hardware, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  if (grouped) {
    return qnnp_leave_create(token, create_grouped_fully_connected(groups, input_channels, output_channels,
        (const uint8_t*) kernel, e8m0, bias, output_min, output_max, fully_connected));
  }
  return qnnp_leave_create(token, create_dynamic_fully_connected(
      input_channels, output_channels, block_size, kernel, weight_bits, mxfp4, kernel_scales_any, kernel_zero_points, bias,
      output_min, output_max, fully_connected));
}

enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8(
    size_t input_channels,
    size_t output_channels,
    const int8_t* kernel,
    const float* kernel_scales,
    const float* bias,
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected)
{
  (void) flags;
  return create_checked("qnnp_gfx950_create_fully_connected_nc_f32_qd8", 0, 1, input_channels, output_channels, 0, 0, kernel, 8,
      kernel_scales, 0, NULL, bias, output_min, output_max, fully_connected);
}

enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8_qc4w(
    size_t input_channels,
    size_t output_channels,
    const uint8_t* kernel,
    const float* kernel_scales,
    const float* bias,
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected)
{
  (void) flags;
  return create_checked("qnnp_gfx950_create_fully_connected_nc_f32_qd8_qc4w", 0, 1, input_channels, output_channels, 0, 0, kernel, 4,
      kernel_scales, 0, NULL, bias, output_min, output_max, fully_connected);
}

enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w(
    size_t input_channels,
    size_t output_channels,
    size_t block_size,
    const uint8_t* kernel,
    const float* kernel_scales,
    const float* bias,
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected)
{
  (void) flags;
  return create_checked("qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w", 0, 1, input_channels, output_channels, 1, block_size,
      kernel, 4, kernel_scales, 0, NULL, bias, output_min, output_max, fully_connected);
}

enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_zp(
    size_t input_channels,
    size_t output_channels,
    size_t block_size,
    const uint8_t* kernel,
    const float* kernel_scales,
    const uint8_t* kernel_zero_points,
    const float* bias,
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected)
{
  (void) flags;
  return create_checked("qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_zp", 0, 1, input_channels, output_channels, 1, block_size,
      kernel, 4, kernel_scales, 1, kernel_zero_points, bias, output_min, output_max, fully_connected);
}

enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_b32(
    size_t input_channels,
    size_t output_channels,
    const uint8_t* kernel,
    const float* kernel_scales,
    const uint8_t* kernel_zero_points,
    const float* bias,
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected)
{
  (void) flags;
  return create_checked("qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_b32", 0, 1, input_channels, output_channels, 2, 32,
      kernel, 4, kernel_scales, kernel_zero_points != NULL, kernel_zero_points, bias, output_min, output_max, fully_connected);
}

enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8_mxfp4w(
    size_t input_channels,
    size_t output_channels,
    const uint8_t* kernel,
    const uint8_t* kernel_scales,
    const float* bias,
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected)
{
  (void) flags;
  return create_checked("qnnp_gfx950_create_fully_connected_nc_f32_qd8_mxfp4w", 0, 1, input_channels, output_channels, 3, 32,
      kernel, 4, kernel_scales, 0, NULL, bias, output_min, output_max, fully_connected);
}

enum qnnp_status qnnp_gfx950_create_grouped_fully_connected_nc_f32_qd8_mxfp4w(
    size_t groups,
    size_t input_channels,
    size_t output_channels,
    const uint8_t* kernel,
    const uint8_t* kernel_scales,
    const float* bias,
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected)
{
  (void) flags;
  return create_checked("qnnp_gfx950_create_grouped_fully_connected_nc_f32_qd8_mxfp4w", 1, groups, input_channels,
      output_channels, 3, 32, kernel, 4, kernel_scales, 0, NULL, bias, output_min, output_max, fully_connected);
}

/* what a _gated setup adds to its plain one: NULL for the plain setups, whose input rows hold input_channels floats; with a
 * gate they hold twice that many, the pairs {gate, up} */
struct qd8_gate {
  float alpha, limit, up_shift;
};

static int gate_is_valid(const struct qd8_gate* gate)
{
  const int alpha_ok = isnormal(gate->alpha) && gate->alpha >= 0x1.0p-6f && gate->alpha <= 0x1.0p+6f;
  const int limit_ok = (gate->limit >= 0x1.0p-6f && gate->limit <= 0x1.0p+6f) || gate->limit == INFINITY;      /* NaN: neither */
  const int shift_ok = gate->up_shift == 0.0f || (isnormal(gate->up_shift) && fabsf(gate->up_shift) <= 0x1.0p+6f);
  return alpha_ok && limit_ok && shift_ok;
}

/* what an _rmsnorm setup adds to its plain one: NULL for the others. The input rows hold input_channels floats as in the plain
 * setups; gamma has that many, and so has every row of the two residual tensors, which share residual_stride. */
struct qd8_norm {
  const float* gamma;
  float epsilon;
  const float* residual;       /* or NULL */
  float* residual_out;         /* NULL, or (with a residual) where input + residual goes: the residual itself, or disjoint */
  size_t residual_stride;
};

static int norm_pointers_are_given(const struct qd8_norm* norm)
{
  return norm->gamma != NULL && (norm->residual_out == NULL || norm->residual != NULL);
}

static int norm_pointers_are_aligned(const struct qd8_norm* norm)
{
  return ((uintptr_t) norm->gamma | (uintptr_t) norm->residual | (uintptr_t) norm->residual_out) % sizeof(float) == 0;
}

static int norm_epsilon_is_valid(const struct qd8_norm* norm)
{
  return isnormal(norm->epsilon) && norm->epsilon >= 0x1.0p-40f && norm->epsilon <= 1.0f;
}

/* the overlap rules of the header: the output shares no byte with gamma or a residual tensor (the setup has compared it with
 * the input and the group ids); residual_out shares none with the input, gamma or the group ids, and is the residual itself
 * or disjoint from it. group_ids is NULL in the plain form. */
static int norm_tensors_overlap(
    const struct qd8_norm* norm, size_t batch_size, size_t k, const void* input, size_t input_span, const void* output,
    size_t output_span, const void* group_ids, size_t ids_span)
{
  const size_t gamma_span = k * sizeof(float);
  const size_t residual_span = ((batch_size - 1) * norm->residual_stride + k) * sizeof(float);
  if (qnnp_spans_overlap(norm->gamma, gamma_span, output, output_span)) {
    return 1;
  }
  if (norm->residual != NULL && qnnp_spans_overlap(norm->residual, residual_span, output, output_span)) {
    return 1;
  }
  if (norm->residual_out == NULL) {
    return 0;
  }
  return qnnp_spans_overlap(norm->residual_out, residual_span, output, output_span) ||
      qnnp_spans_overlap(norm->residual_out, residual_span, input, input_span) ||
      qnnp_spans_overlap(norm->residual_out, residual_span, norm->gamma, gamma_span) ||
      (group_ids != NULL && qnnp_spans_overlap(norm->residual_out, residual_span, group_ids, ids_span)) ||
      ((const float*) norm->residual_out != norm->residual &&
          qnnp_spans_overlap(norm->residual_out, residual_span, norm->residual, residual_span));
}

static int norm_tensors_are_on_device(const struct qd8_norm* norm)
{
  return qnnp_hip_is_device_pointer(norm->gamma) == 1 &&
      (norm->residual == NULL || qnnp_hip_is_device_pointer(norm->residual) == 1) &&
      (norm->residual_out == NULL || qnnp_hip_is_device_pointer(norm->residual_out) == 1);
}

/* the input form of the setup that is being made: a gate, a norm, or neither (never both) */
static void remember_input_form(qnnp_operator_t op, const struct qd8_gate* gate, const struct qd8_norm* norm)
{
  op->qd8_gated = gate != NULL;
  if (gate != NULL) {
    op->qd8_gate_alpha = gate->alpha;
    op->qd8_gate_limit = gate->limit;
    op->qd8_gate_up_shift = gate->up_shift;
  }
  op->qd8_rmsnorm = norm != NULL;
  if (norm != NULL) {
    op->qd8_norm_gamma = norm->gamma;
    op->qd8_norm_epsilon = norm->epsilon;
    op->qd8_norm_residual = norm->residual;
    op->qd8_norm_residual_out = norm->residual_out;
    op->qd8_norm_residual_stride = norm->residual_stride;
  }
}

static enum qnnp_status setup_dynamic_fully_connected(
    const char* function, qnnp_operator_t op, size_t batch_size, const float* input, size_t input_stride,
    const struct qd8_gate* gate, const struct qd8_norm* norm, float* output, size_t output_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_dynamic_fully_connected || op->qd8_groups != 0) {
    return qnnp_status_invalid_parameter;
  }
  if (norm != NULL && op->group_input_channels > QNNP_QD8_MAX_NORM_CHANNELS) {
    qnnp_log_error("cannot set up dynamic fully connected operator with %zu input channels on normalized rows: at most %zu",
        op->group_input_channels, QNNP_QD8_MAX_NORM_CHANNELS);
    return qnnp_status_unsupported_parameter;
  }
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  /* the floats of an input row; the quantized row has group_input_channels elements either way */
  const size_t input_channels = (gate != NULL ? 2 : 1) * op->group_input_channels, output_channels = op->channels;
  if (input == NULL || output == NULL || (norm != NULL && !norm_pointers_are_given(norm))) {
    qnnp_log_error("cannot set up dynamic fully connected operator: NULL tensor, or a residual output without a residual");
    return qnnp_status_invalid_parameter;
  }
  if ((uintptr_t) input % sizeof(float) != 0 || (uintptr_t) output % sizeof(float) != 0 ||
      (norm != NULL && !norm_pointers_are_aligned(norm))) {
    qnnp_log_error("cannot set up dynamic fully connected operator: a tensor is not 4-byte aligned");
    return qnnp_status_invalid_parameter;
  }
  if (gate != NULL && !gate_is_valid(gate)) {
    qnnp_log_error("cannot set up dynamic fully connected operator with gate parameters alpha %.7g, limit %.7g, up_shift "
        "%.7g: alpha a normal number in [2^-6, 2^6], limit in [2^-6, 2^6] or +infinity, up_shift zero or a normal number of "
        "at most 2^6 in magnitude", gate->alpha, gate->limit, gate->up_shift);
    return qnnp_status_invalid_parameter;
  }
  if (norm != NULL && !norm_epsilon_is_valid(norm)) {
    qnnp_log_error("cannot set up dynamic fully connected operator with epsilon %.7g: not a normal number in [2^-40, 1]",
        norm->epsilon);
    return qnnp_status_invalid_parameter;
  }
  if (input_stride < input_channels || output_stride < output_channels ||
      (norm != NULL && norm->residual != NULL && norm->residual_stride < input_channels)) {
    qnnp_log_error("cannot set up dynamic fully connected operator: row stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  if (batch_size > (size_t) INT32_MAX) {
    qnnp_log_error("cannot set up dynamic fully connected operator with batch %zu: outside the device kernels' index range",
        batch_size);
    return qnnp_status_unsupported_parameter;
  }
  const size_t input_span = ((batch_size - 1) * input_stride + input_channels) * sizeof(float);
  const size_t output_span = ((batch_size - 1) * output_stride + output_channels) * sizeof(float);
  if (qnnp_spans_overlap(input, input_span, output, output_span) ||
      (norm != NULL && norm_tensors_overlap(norm, batch_size, input_channels, input, input_span, output, output_span, NULL, 0))) {
    qnnp_log_error("cannot set up dynamic fully connected operator: the input and output tensors overlap, or the tensors of "
        "the normalization overlap them or each other");
    return qnnp_status_invalid_parameter;
  }
  if (qnnp_hip_is_device_pointer(input) < 0 || qnnp_hip_is_device_pointer(output) < 0) {
    qnnp_log_error("cannot set up dynamic fully connected operator: a tensor lives on a different device than the operator");
    return qnnp_status_invalid_parameter;
  }
  /* the device reads gamma when the operator runs, and a staged output next to a device residual_out is not built */
  if (norm != NULL && (qnnp_hip_is_device_pointer(input) != 1 || qnnp_hip_is_device_pointer(output) != 1 ||
      !norm_tensors_are_on_device(norm))) {
    qnnp_log_error("cannot set up dynamic fully connected operator on normalized rows: every tensor has to be memory of the "
        "operator's device");
    return qnnp_status_invalid_parameter;
  }
  /* the quantized rows (k_pad is a multiple of 64: the table behind them is 8-byte aligned), then the row table */
  const size_t row_table_offset = batch_size * op->k_pad;
  const size_t scratch_bytes = row_table_offset + batch_size * sizeof(struct qnnp_hip_qd8_row_entry);

  op->setup_valid = 0;   /* from here on the operator changes: until every allocation below has succeeded */
  if (op->qd8_scratch_capacity < scratch_bytes) {
    qnnp_hip_free(op->d_qd8_scratch);
    op->qd8_scratch_capacity = 0;
    op->d_qd8_scratch = qnnp_hip_alloc(scratch_bytes);
    if (op->d_qd8_scratch == NULL) {
      qnnp_log_error("failed to allocate %zu bytes of device scratch for the quantized rows", scratch_bytes);
      return qnnp_status_out_of_memory;
    }
    op->qd8_scratch_capacity = scratch_bytes;
  }
  op->qd8_row_table_offset = row_table_offset;
  remember_input_form(op, gate, norm);
  op->batch_size = batch_size;
  op->input = input;
  op->input_pixel_stride = input_stride;
  op->output = output;
  op->output_pixel_stride = output_stride;
  op->input_span = input_span;
  op->output_span = output_span;
  return qnnp_bind_tensors(op, function);
}

/* the three plain setups: the lifecycle around the one body */
static enum qnnp_status setup_dynamic_fully_connected_entered(
    const char* function, qnnp_operator_t fully_connected, size_t batch_size, const float* input, size_t input_stride,
    const struct qd8_gate* gate, const struct qd8_norm* norm, float* output, size_t output_stride)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup(function, fully_connected, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(fully_connected, token, setup_dynamic_fully_connected(
      function, fully_connected, batch_size, input, input_stride, gate, norm, output, output_stride));
}

enum qnnp_status qnnp_gfx950_setup_fully_connected_nc_f32_qd8(
    qnnp_operator_t fully_connected,
    size_t batch_size,
    const float* input,
    size_t input_stride,
    float* output,
    size_t output_stride)
{
  return setup_dynamic_fully_connected_entered("qnnp_gfx950_setup_fully_connected_nc_f32_qd8", fully_connected, batch_size,
      input, input_stride, NULL, NULL, output, output_stride);
}

enum qnnp_status qnnp_gfx950_setup_fully_connected_nc_f32_qd8_gated(
    qnnp_operator_t fully_connected,
    size_t batch_size,
    const float* input,
    size_t input_stride,
    float alpha,
    float limit,
    float up_shift,
    float* output,
    size_t output_stride)
{
  const struct qd8_gate gate = { .alpha = alpha, .limit = limit, .up_shift = up_shift };
  return setup_dynamic_fully_connected_entered("qnnp_gfx950_setup_fully_connected_nc_f32_qd8_gated", fully_connected,
      batch_size, input, input_stride, &gate, NULL, output, output_stride);
}

enum qnnp_status qnnp_gfx950_setup_fully_connected_nc_f32_qd8_rmsnorm(
    qnnp_operator_t fully_connected,
    size_t batch_size,
    const float* input,
    size_t input_stride,
    const float* gamma,
    float epsilon,
    const float* residual,
    float* residual_out,
    size_t residual_stride,
    float* output,
    size_t output_stride)
{
  const struct qd8_norm norm = { .gamma = gamma, .epsilon = epsilon, .residual = residual, .residual_out = residual_out,
                                 .residual_stride = residual_stride };
  return setup_dynamic_fully_connected_entered("qnnp_gfx950_setup_fully_connected_nc_f32_qd8_rmsnorm", fully_connected,
      batch_size, input, input_stride, NULL, &norm, output, output_stride);
}

static inline size_t round_up_16(size_t bytes)
{
  return (bytes + 15) & ~(size_t) 15;
}

static enum qnnp_status setup_grouped_fully_connected(
    const char* function, qnnp_operator_t op, size_t batch_size, size_t assignments, const float* input, size_t input_stride,
    const struct qd8_gate* gate, const struct qd8_norm* norm, const int32_t* group_ids, float* output, size_t output_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_dynamic_fully_connected || op->qd8_groups == 0) {
    return qnnp_status_invalid_parameter;
  }
  if (norm != NULL && op->group_input_channels > QNNP_QD8_MAX_NORM_CHANNELS) {
    qnnp_log_error("cannot set up grouped dynamic fully connected operator with %zu input channels on normalized rows: at "
        "most %zu", op->group_input_channels, QNNP_QD8_MAX_NORM_CHANNELS);
    return qnnp_status_unsupported_parameter;
  }
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t input_channels = (gate != NULL ? 2 : 1) * op->group_input_channels, output_channels = op->channels;
  if (input == NULL || output == NULL || group_ids == NULL || assignments == 0 ||
      (norm != NULL && !norm_pointers_are_given(norm))) {
    qnnp_log_error("cannot set up grouped dynamic fully connected operator: NULL tensor or group ids, or no assignments");
    return qnnp_status_invalid_parameter;
  }
  if ((uintptr_t) input % sizeof(float) != 0 || (uintptr_t) output % sizeof(float) != 0 ||
      (uintptr_t) group_ids % sizeof(int32_t) != 0 || (norm != NULL && !norm_pointers_are_aligned(norm))) {
    qnnp_log_error("cannot set up grouped dynamic fully connected operator: a tensor or the group ids are not 4-byte aligned");
    return qnnp_status_invalid_parameter;
  }
  if (gate != NULL && !gate_is_valid(gate)) {
    qnnp_log_error("cannot set up grouped dynamic fully connected operator with gate parameters alpha %.7g, limit %.7g, "
        "up_shift %.7g: alpha a normal number in [2^-6, 2^6], limit in [2^-6, 2^6] or +infinity, up_shift zero or a normal "
        "number of at most 2^6 in magnitude", gate->alpha, gate->limit, gate->up_shift);
    return qnnp_status_invalid_parameter;
  }
  if (norm != NULL && !norm_epsilon_is_valid(norm)) {
    qnnp_log_error("cannot set up grouped dynamic fully connected operator with epsilon %.7g: not a normal number in "
        "[2^-40, 1]", norm->epsilon);
    return qnnp_status_invalid_parameter;
  }
  if (input_stride < input_channels || output_stride < output_channels ||
      (norm != NULL && norm->residual != NULL && norm->residual_stride < input_channels)) {
    qnnp_log_error("cannot set up grouped dynamic fully connected operator: row stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  /* the limits, before any product of the sizes is formed and before anything is looked at */
  if (assignments > QNNP_QD8_MAX_ASSIGNMENTS || batch_size >= QNNP_QD8_MAX_GROUPED_ROWS ||
      batch_size * assignments >= QNNP_QD8_MAX_GROUPED_ROWS || batch_size * op->k_pad > QNNP_QD8_MAX_GATHER_BYTES) {
    qnnp_log_error("cannot set up grouped dynamic fully connected operator with batch %zu and %zu assignments: at most %zu "
        "assignments, fewer than %zu output rows and at most %zu bytes of quantized input rows", batch_size, assignments,
        QNNP_QD8_MAX_ASSIGNMENTS, QNNP_QD8_MAX_GROUPED_ROWS, QNNP_QD8_MAX_GATHER_BYTES);
    return qnnp_status_unsupported_parameter;
  }
  const size_t rows = batch_size * assignments;
  /* H and the grid: by the sizes alone. At a mean of 16 rows per group or fewer a 128-row tile is at least 7 / 8 padding and
   * the groups' weights are streamed once each, the 16-row kernel's regime. */
  const int forced = qnnp_state.opt_qd8_grouped_kernel;
  const uint32_t tile_rows = forced == 1 || (forced == 0 && rows <= 16 * (size_t) op->qd8_groups) ? 16 : 128;
  const size_t max_tiles = rows / tile_rows + (op->qd8_groups < rows ? op->qd8_groups : rows);
  const size_t tiles_n = tile_rows == 16 ? op->n_pad / 16 : (output_channels + 127) / 128;
  if (max_tiles * tiles_n > (size_t) INT32_MAX) {
    qnnp_log_error("cannot set up grouped dynamic fully connected operator: %zu x %zu tiles are outside the launch range",
        max_tiles, tiles_n);
    return qnnp_status_unsupported_parameter;
  }
  const size_t input_span = ((batch_size - 1) * input_stride + input_channels) * sizeof(float);
  const size_t output_span = ((rows - 1) * output_stride + output_channels) * sizeof(float);
  const size_t ids_span = rows * sizeof(int32_t);
  if (qnnp_spans_overlap(input, input_span, output, output_span) || qnnp_spans_overlap(group_ids, ids_span, output, output_span) ||
      (norm != NULL &&
          norm_tensors_overlap(norm, batch_size, input_channels, input, input_span, output, output_span, group_ids, ids_span))) {
    qnnp_log_error("cannot set up grouped dynamic fully connected operator: the output overlaps the input or the group ids, or "
        "the tensors of the normalization overlap them or each other");
    return qnnp_status_invalid_parameter;
  }
  /* all three in device memory: the ids are read by the launches, and an output staged through the device would bring
   * back bytes for the rows that were skipped */
  if (qnnp_hip_is_device_pointer(input) != 1 || qnnp_hip_is_device_pointer(output) != 1 ||
      qnnp_hip_is_device_pointer(group_ids) != 1 || (norm != NULL && !norm_tensors_are_on_device(norm))) {
    qnnp_log_error("cannot set up grouped dynamic fully connected operator: the tensors and the group ids have to be memory "
        "of the operator's device");
    return qnnp_status_invalid_parameter;
  }
  /* the quantized rows, the row table, the permutation, the tile list (16-byte entries), the tile count */
  const size_t row_table_offset = batch_size * op->k_pad;
  const size_t perm_offset = row_table_offset + batch_size * sizeof(struct qnnp_hip_qd8_row_entry);
  const size_t tiles_offset = round_up_16(perm_offset + rows * sizeof(uint32_t));
  const size_t tile_count_offset = tiles_offset + max_tiles * sizeof(struct qnnp_hip_qd8_grouped_tile);
  const size_t scratch_bytes = tile_count_offset + sizeof(uint32_t);

  op->setup_valid = 0;   /* from here on the operator changes: until every allocation below has succeeded */
  if (op->qd8_scratch_capacity < scratch_bytes) {
    qnnp_hip_free(op->d_qd8_scratch);
    op->qd8_scratch_capacity = 0;
    op->d_qd8_scratch = qnnp_hip_alloc(scratch_bytes);
    if (op->d_qd8_scratch == NULL) {
      qnnp_log_error("failed to allocate %zu bytes of device scratch for the quantized rows and the plan", scratch_bytes);
      return qnnp_status_out_of_memory;
    }
    op->qd8_scratch_capacity = scratch_bytes;
  }
  op->qd8_row_table_offset = row_table_offset;
  op->qd8_perm_offset = perm_offset;
  op->qd8_tiles_offset = tiles_offset;
  op->qd8_tile_count_offset = tile_count_offset;
  op->qd8_assignments = (uint32_t) assignments;
  op->qd8_tile_rows = tile_rows;
  op->qd8_max_tiles = (uint32_t) max_tiles;
  op->qd8_group_ids = group_ids;
  remember_input_form(op, gate, norm);
  op->batch_size = batch_size;
  op->input = input;
  op->input_pixel_stride = input_stride;
  op->output = output;
  op->output_pixel_stride = output_stride;
  op->input_span = input_span;
  op->output_span = output_span;
  return qnnp_bind_tensors(op, function);
}

/* the three grouped setups: the lifecycle around the one body */
static enum qnnp_status setup_grouped_fully_connected_entered(
    const char* function, qnnp_operator_t fully_connected, size_t batch_size, size_t assignments, const float* input,
    size_t input_stride, const struct qd8_gate* gate, const struct qd8_norm* norm, const int32_t* group_ids, float* output,
    size_t output_stride)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup(function, fully_connected, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(fully_connected, token, setup_grouped_fully_connected(
      function, fully_connected, batch_size, assignments, input, input_stride, gate, norm, group_ids, output, output_stride));
}

enum qnnp_status qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8(
    qnnp_operator_t fully_connected,
    size_t batch_size,
    size_t assignments,
    const float* input,
    size_t input_stride,
    const int32_t* group_ids,
    float* output,
    size_t output_stride)
{
  return setup_grouped_fully_connected_entered("qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8", fully_connected,
      batch_size, assignments, input, input_stride, NULL, NULL, group_ids, output, output_stride);
}

enum qnnp_status qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8_gated(
    qnnp_operator_t fully_connected,
    size_t batch_size,
    size_t assignments,
    const float* input,
    size_t input_stride,
    float alpha,
    float limit,
    float up_shift,
    const int32_t* group_ids,
    float* output,
    size_t output_stride)
{
  const struct qd8_gate gate = { .alpha = alpha, .limit = limit, .up_shift = up_shift };
  return setup_grouped_fully_connected_entered("qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8_gated", fully_connected,
      batch_size, assignments, input, input_stride, &gate, NULL, group_ids, output, output_stride);
}

enum qnnp_status qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8_rmsnorm(
    qnnp_operator_t fully_connected,
    size_t batch_size,
    size_t assignments,
    const float* input,
    size_t input_stride,
    const float* gamma,
    float epsilon,
    const float* residual,
    float* residual_out,
    size_t residual_stride,
    const int32_t* group_ids,
    float* output,
    size_t output_stride)
{
  const struct qd8_norm norm = { .gamma = gamma, .epsilon = epsilon, .residual = residual, .residual_out = residual_out,
                                 .residual_stride = residual_stride };
  return setup_grouped_fully_connected_entered("qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8_rmsnorm", fully_connected,
      batch_size, assignments, input, input_stride, NULL, &norm, group_ids, output, output_stride);
}

const char* qnnp_gfx950_dynamic_rows_kernel(qnnp_operator_t fully_connected)
{
  return fully_connected != NULL && fully_connected->ukernel_type == qnnp_ukernel_type_dynamic_fully_connected
      ? fully_connected->qd8_rows_kernel : NULL;
}
