/*
 * f32qd8rows.hip -- the first launch of the dynamically quantized fully connected operator (dynamic-fully-connected.c;
 * include/qnnpack_gfx950_dynamic.h has the definition): per input row, ONE launch finds the range, derives the row's
 * scale and zero point and writes the quantized row. No reference counterpart. Float32, every operation rounded once:
 * no multiply is followed by an add anywhere in this file, so nothing can fuse.
 *
 *   lo = min(0, min_k x), hi = max(0, max_k x)                  NaN elements drop out of fminf / fmaxf
 *   scale = (hi - lo) / 255;  outside [2^-60, 2^60] (or NaN): 1
 *   inv = 1 / scale;  zp = (int) rintf(min(-lo * inv, 255))
 *   t = x * inv;  NaN -> 0;  clamp to [-zp, 255 - zp];  q = (int) rintf(t) + zp
 * The row goes out as int8 q - 128 (q ^ 0x80), k_pad bytes, the bytes from K on zero, and {scale, 128 - zp} into the row
 * table: what qd8f32gemm.hip reads.
 *
 * A lane's piece is SIXTEEN consecutive elements of one row: four 16-byte float loads in, one 16-byte store out, so the
 * int8 row is written in whole 16-byte pieces and the pad up to k_pad (a multiple of 64) by the same stores. Three
 * kernels by K, so that a row is read from HBM once wherever it fits in registers:
 *   f32_qd8_rows_wave     K <= 1024: one wave per row, one piece per lane, four rows per workgroup; nothing but lane
 *                         exchanges between the loads and the stores
 *   f32_qd8_rows_block    K <= 16384: one 256-thread workgroup per row, up to four pieces (64 floats) per lane in registers
 *   f32_qd8_rows_twopass  beyond: the workgroup walks the row for the range, then again to quantize (the second walk
 *                         finds a row of up to 128 KiB in L2)
 * The range is reduced inside a wave by ds_swizzle butterflies over 32 lanes and one v_permlane32_swap across the halves,
 * across the four waves of a workgroup through LDS. Every lane ends up with the SAME lo and hi and computes scale, inv and
 * zp from those two floats itself: no lane can disagree, and nothing is broadcast.
 * The _x4 flavours (input base, or with more than one row the row stride, no multiple of 16 bytes) load the sixteen
 * elements as dwords; so does the one piece of a row that K cuts, in both flavours.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"
#include "f32qd8rows.hip.h"
#include "per_device.h"
#include "qnnp_hip.h"

#pragma clang fp contract(off)

namespace qnnp {

namespace {

struct RowsParams {
  const float* x;
  int8_t* q;
  qnnp_hip_qd8_row_entry* table;
  uint64_t x_stride;     // elements
  uint32_t rows, k, k_pad;
};

template <bool VEC>
__global__ __launch_bounds__(kRowsThreads)
void f32_qd8_rows_wave_kernel(const RowsParams p)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t row = static_cast<uint64_t>(blockIdx.x) * (kRowsThreads / 64) + (threadIdx.x >> 6);
  if (row >= p.rows) return;                                  // (wave-uniform; no barrier in this kernel)
  const float* x_row = p.x + row * p.x_stride;
  const uint32_t e0 = lane * kPiece;
  const Piece piece = load_piece<VEC>(x_row, e0, p.k);        // lanes past K hold zeros
  float lo = 0.0f, hi = 0.0f;
  piece_range(piece, lo, hi);
  wave_range(lo, hi);
  const RowQuant r = row_quant(lo, hi);
  if (e0 < p.k_pad) store_piece(piece, p.q + row * p.k_pad, e0, p.k, r);
  if (lane == 0) store_entry(p.table + row, r);
}

template <bool VEC>
__global__ __launch_bounds__(kRowsThreads)
void f32_qd8_rows_block_kernel(const RowsParams p)
{
  __shared__ float range[4][2];
  const uint64_t row = blockIdx.x;
  const float* x_row = p.x + row * p.x_stride;
  Piece piece[kBlockPieces];
  float lo = 0.0f, hi = 0.0f;
#pragma unroll
  for (int i = 0; i < kBlockPieces; i++) {
    const uint32_t e0 = (i * kRowsThreads + threadIdx.x) * kPiece;
    piece[i] = load_piece<VEC>(x_row, e0, p.k);
    piece_range(piece[i], lo, hi);
  }
  wave_range(lo, hi);
  block_range(lo, hi, range);
  const RowQuant r = row_quant(lo, hi);
  int8_t* q_row = p.q + row * p.k_pad;
#pragma unroll
  for (int i = 0; i < kBlockPieces; i++) {
    const uint32_t e0 = (i * kRowsThreads + threadIdx.x) * kPiece;
    if (e0 < p.k_pad) store_piece(piece[i], q_row, e0, p.k, r);
  }
  if (threadIdx.x == 0) store_entry(p.table + row, r);
}

template <bool VEC>
__global__ __launch_bounds__(kRowsThreads)
void f32_qd8_rows_twopass_kernel(const RowsParams p)
{
  __shared__ float range[4][2];
  const uint64_t row = blockIdx.x;
  const float* x_row = p.x + row * p.x_stride;
  float lo = 0.0f, hi = 0.0f;
  for (uint32_t e0 = threadIdx.x * kPiece; e0 < p.k; e0 += kRowsThreads * kPiece) {
    const Piece piece = load_piece<VEC>(x_row, e0, p.k);
    piece_range(piece, lo, hi);
  }
  wave_range(lo, hi);
  block_range(lo, hi, range);
  const RowQuant r = row_quant(lo, hi);
  int8_t* q_row = p.q + row * p.k_pad;
  for (uint32_t e0 = threadIdx.x * kPiece; e0 < p.k_pad; e0 += kRowsThreads * kPiece) {
    const Piece piece = load_piece<VEC>(x_row, e0, p.k);
    store_piece(piece, q_row, e0, p.k, r);
  }
  if (threadIdx.x == 0) store_entry(p.table + row, r);
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_qd8_rows_run(const struct qnnp_hip_qd8_rows_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->input == nullptr || a->quantized == nullptr || a->row_table == nullptr ||
      (reinterpret_cast<uintptr_t>(a->input) & 3u) != 0 || (reinterpret_cast<uintptr_t>(a->quantized) & 15u) != 0 ||
      a->k == 0 || a->k > 32768u || a->k_pad != ((a->k + 63u) & ~63u) || a->rows > 0x7FFFFFFFu || a->input_stride < a->k) {
    return QNNP_HIP_EINVAL;
  }
  if (a->rows == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  RowsParams p;
  p.x = a->input;
  p.q = a->quantized;
  p.table = a->row_table;
  p.x_stride = a->input_stride;
  p.rows = a->rows;
  p.k = a->k;
  p.k_pad = a->k_pad;
  const bool vec = (reinterpret_cast<uintptr_t>(a->input) & 15u) == 0 && (a->rows == 1 || a->input_stride % 4 == 0);
  const char* name;
  if (a->k <= kWaveMaxK) {
    const dim3 grid((a->rows + 3u) / 4u);
    if (vec) hipLaunchKernelGGL((f32_qd8_rows_wave_kernel<true>), grid, dim3(kRowsThreads), 0, stream, p);
    else hipLaunchKernelGGL((f32_qd8_rows_wave_kernel<false>), grid, dim3(kRowsThreads), 0, stream, p);
    name = vec ? "f32_qd8_rows_wave" : "f32_qd8_rows_wave_x4";
  } else if (a->k <= kBlockMaxK) {
    if (vec) hipLaunchKernelGGL((f32_qd8_rows_block_kernel<true>), dim3(a->rows), dim3(kRowsThreads), 0, stream, p);
    else hipLaunchKernelGGL((f32_qd8_rows_block_kernel<false>), dim3(a->rows), dim3(kRowsThreads), 0, stream, p);
    name = vec ? "f32_qd8_rows_block" : "f32_qd8_rows_block_x4";
  } else {
    if (vec) hipLaunchKernelGGL((f32_qd8_rows_twopass_kernel<true>), dim3(a->rows), dim3(kRowsThreads), 0, stream, p);
    else hipLaunchKernelGGL((f32_qd8_rows_twopass_kernel<false>), dim3(a->rows), dim3(kRowsThreads), 0, stream, p);
    name = vec ? "f32_qd8_rows_twopass" : "f32_qd8_rows_twopass_x4";
  }
  if (kernel_name != nullptr) *kernel_name = name;
  return launch_status();
}
