/*
 * qd8_epilogue.hip.h -- what the product kernels of the dynamically quantized fully connected operator share
 * (qd8f32gemm.hip: int8 weights; qd8f32gemm4.hip: 4-bit weights): the kernel argument block and the float epilogue of
 * include/qnnpack_gfx950_dynamic.h. Per output, in this order, every float operation rounded once:
 *   acc += (128 - zp_r) * wsum[c]            the rows are centred on 128, the definition on zp_r
 *   s = scale_r * kernel_scale[c];  y = (float) acc * s;  y = y + bias[c];  y = min(max(y, output_min), output_max)
 * A unit that includes this is compiled with contraction off (the pragma below holds for the rest of the unit):
 * y * s + bias must not become one fused operation.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"
#include "qnnp_hip.h"

#pragma clang fp contract(off)

namespace qnnp {

namespace {

struct Qd8Params {
  const uint8_t* a;                          // [rows][k_pad] int8
  const qnnp_hip_qd8_row_entry* rows_tab;    // [rows]
  const uint8_t* w;                          // fragments [n_pad / 16][k_pad / 64][1024]
  const qnnp_hip_qd8_channel_entry* chan_tab;   // [n_pad]
  float* out;
  uint64_t out_stride;                       // elements
  uint32_t rows, n, n_pad, k_pad;
  uint32_t tiles_n;                          // gemm: 128-channel tiles
  float out_min, out_max;
};

/* one output from its accumulator: the definition's float sequence, in its order */
__device__ __forceinline__ float qd8_finish(int32_t acc, const qnnp_hip_qd8_row_entry& row, const qnnp_hip_qd8_channel_entry& ch,
                                            float out_min, float out_max)
{
  acc += row.zero_offset * ch.wsum;          // |.| <= 128 * 128 * 32768 = 2^29 on either side: no wrap
  const float s = row.scale * ch.kernel_scale;
  float y = static_cast<float>(acc) * s;
  y = y + ch.bias;
  return fminf(fmaxf(y, out_min), out_max);
}

/* block-wise scales (qd8f32gemm4b.hip): one output from the ordered float sum of its blocks' terms */
__device__ __forceinline__ float qb4w_finish(float ysum, const qnnp_hip_qd8_row_entry& row, float bias, float out_min, float out_max)
{
  float y = ysum * row.scale;
  y = y + bias;
  return fminf(fmaxf(y, out_min), out_max);
}

/* One 16 x 16 accumulator tile: lane l holds rows row0 + 4 (l / 16) + r (r = 0 .. 3) of channel c0 + l % 16. The four row
 * entries are one 32-byte run of the table, loaded once per tile row (rows past the batch re-read the last entry). */
struct RowQuad {
  qnnp_hip_qd8_row_entry e[4];
};
__device__ __forceinline__ RowQuad qd8_load_rows(uint32_t row0, const Qd8Params& p)
{
  const uint32_t first = row0 + 4u * ((threadIdx.x & 63u) >> 4);
  RowQuad q;
#pragma unroll
  for (uint32_t r = 0; r < 4; r++) q.e[r] = p.rows_tab[first + r < p.rows ? first + r : p.rows - 1u];
  return q;
}
__device__ __forceinline__ void qd8_store_tile(const v4i& acc, uint32_t row0, const RowQuad& rows, uint32_t c,
                                               const qnnp_hip_qd8_channel_entry& ch, const Qd8Params& p)
{
  const uint32_t first = row0 + 4u * ((threadIdx.x & 63u) >> 4);
#pragma unroll
  for (uint32_t r = 0; r < 4; r++) {
    const float y = qd8_finish(acc[r], rows.e[r], ch, p.out_min, p.out_max);
    if (first + r < p.rows && c < p.n) p.out[static_cast<uint64_t>(first + r) * p.out_stride + c] = y;
  }
}

}  // namespace

}  // namespace qnnp
