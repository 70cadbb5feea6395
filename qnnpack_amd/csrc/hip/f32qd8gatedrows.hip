/*
 * f32qd8gatedrows.hip -- the first launch of the dynamically quantized fully connected operator after a GATED setup
 * (dynamic-fully-connected.c; include/qnnpack_gfx950_dynamic.h has the definition): the input row holds K pairs
 * {gate, up}, interleaved, and the row that is quantized is h[k] = act(gate[k]) * (up[k] + up_shift), act(g) =
 * g * sigmoid(alpha * g) with both values clamped at `limit` first (SwiGLU and its clamped form). h exists in registers
 * only: it is never written as floats. No reference counterpart. Float32, every operation rounded once: no multiply is
 * followed by an add that could fuse (contraction is off for the file), and the division is the IEEE one.
 *
 *   gc = g > limit ? limit : g;   uc = u > limit ? limit : (u < -limit ? -limit : u);   z = alpha * gc
 *   y = max(-|z|, -80);  n = rintf(y * log2(e));  r = (y - n * ln2_hi) - n * ln2_lo;  p = a degree-6 polynomial in r
 *   e = p * 2^n  (= exp(-|z|), never above 1);  q = e / (1 + e);  sigmoid(z) = z > 0 ? 1 - q : q
 *   a = gc * sigmoid(z), a signed zero if |a| <= 2^-126;  b = uc + up_shift, a signed zero if |b| < 2^-126;  h = a * b
 * and from h on everything is f32qd8rows.hip's, through the helpers of f32qd8rows.hip.h: range, scale, zero point, the
 * int8 row q - 128 in whole 16-byte stores with the pad up to k_pad zeroed, {scale, 128 - zp} into the row table.
 *
 * A lane's piece is SIXTEEN positions = thirty-two input floats = one contiguous 128-byte read, eight 16-byte loads. Three
 * kernels with the regime bounds of the plain ones, on K = the number of POSITIONS:
 *   f32_qd8_gated_rows_wave     K <= 1024: one wave per row, one piece per lane, four rows per workgroup
 *   f32_qd8_gated_rows_block    K <= 16384: one workgroup per row; a lane turns each piece into its sixteen h as it
 *                               arrives and keeps up to 64 h in registers -- not the 128 inputs
 *   f32_qd8_gated_rows_twopass  beyond: the row is walked twice and h computed twice (same code, same bits); the second
 *                               walk finds the row, 256 KiB at most, in L2
 * How a piece overlaps the next: the block and twopass kernels hold TWO raw pieces. The eight loads of piece i + 1 are
 * issued before the first instruction that needs piece i, so the polynomial and the division of piece i (sixteen times
 * about sixty instructions) run while piece i + 1 is in flight. A lane skips the arithmetic of a piece that begins at or
 * past K: at K = 2880, 180 of 256 lanes have one piece and nobody has a second.
 * The _x4 flavours (input base, or with more than one row the row stride, no multiple of 16 bytes) load dwords; so does the
 * one piece of a row that K cuts, in both flavours. Positions from K on are h = 0, which neither end of the range sees.
 * The wave kernel gives a lane sixteen positions at every K: fewer would spread the arithmetic over more lanes, but a
 * lane's sixteen output bytes are one store, and the pad is zeroed by those same stores.
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

struct GatedRowsParams {
  const float* x;
  int8_t* q;
  qnnp_hip_qd8_row_entry* table;
  uint64_t x_stride;     // elements (floats), at least 2 k
  uint32_t rows, k, k_pad;
  float alpha, limit, up_shift;
};

/* the thirty-two input floats of a piece: v[2 i] the gate and v[2 i + 1] the up value of position e0 + i */
struct RawPiece {
  float v[2 * kPiece];
};

/* positions from K on read as {0, 0}; a piece that begins at or past K touches no memory */
template <bool VEC>
__device__ __forceinline__ RawPiece load_raw(const float* row, uint32_t e0, uint32_t k)
{
  RawPiece p;
  if (VEC && e0 + kPiece <= k) {
    const f32x4* src = reinterpret_cast<const f32x4*>(row + 2 * e0);
    f32x4 t[8];
#pragma unroll
    for (int j = 0; j < 8; j++) t[j] = src[j];
#pragma unroll
    for (int j = 0; j < 8; j++) {
#pragma unroll
      for (int i = 0; i < 4; i++) p.v[4 * j + i] = t[j][i];
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kPiece; i++) {
      const bool in = e0 + i < k;
      p.v[2 * i] = in ? row[2 * (e0 + i)] : 0.0f;
      p.v[2 * i + 1] = in ? row[2 * (e0 + i) + 1] : 0.0f;
    }
  }
  return p;
}

/* h of one position, the header's lines in their order. A NaN gate reaches no float-to-integer conversion: the exponent
 * path runs on y = 0 for it, and a = gc * s is NaN whatever s is. */
__device__ __forceinline__ float gated_h(float g, float u, float alpha, float limit, float up_shift)
{
  const float gc = g > limit ? limit : g;
  const float uc = u > limit ? limit : (u < -limit ? -limit : u);
  const float z = alpha * gc;
  float y = -fabsf(z);
  y = y < -80.0f ? -80.0f : y;
  y = y != y ? 0.0f : y;
  const float n = rintf(y * 0x1.715476p+0f);
  const float r1 = y - n * 0x1.62E400p-1f;               // the product is exact
  const float r2 = r1 - n * 0x1.7F7D1Cp-20f;
  float p = 0x1.0F9F9Cp-7f;
  p = p * r2;  p = p + 0x1.573A1Ap-5f;
  p = p * r2;  p = p + 0x1.555A80p-3f;
  p = p * r2;  p = p + 0x1.FFFDC6p-2f;
  p = p * r2;  p = p + 0x1.FFFFF6p-1f;
  p = p * r2;  p = p + 1.0f;
  const float e = p * __int_as_float((static_cast<int>(n) + 127) << 23);     // n in [-116, 0]: a normal power of two
  const float d = 1.0f + e;
  const float q = e / d;
  const float s = z > 0.0f ? 1.0f - q : q;
  float a = gc * s;
  a = fabsf(a) <= 0x1.0p-126f ? copysignf(0.0f, a) : a;      // <=: a product that ROUNDS to 2^-126 is a zero in either denormal mode
  float b = uc + up_shift;
  b = fabsf(b) < 0x1.0p-126f ? copysignf(0.0f, b) : b;
  return a * b;
}

/* the sixteen h of a raw piece; positions from K on are 0 */
__device__ __forceinline__ Piece gate_piece(const RawPiece& raw, uint32_t e0, const GatedRowsParams& p)
{
  Piece h;
  if (e0 < p.k) {
#pragma unroll
    for (uint32_t i = 0; i < kPiece; i++) {
      const float v = gated_h(raw.v[2 * i], raw.v[2 * i + 1], p.alpha, p.limit, p.up_shift);
      h.v[i] = e0 + i < p.k ? v : 0.0f;
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kPiece; i++) h.v[i] = 0.0f;
  }
  return h;
}

template <bool VEC>
__global__ __launch_bounds__(kRowsThreads)
void f32_qd8_gated_rows_wave_kernel(const GatedRowsParams p)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t row = static_cast<uint64_t>(blockIdx.x) * (kRowsThreads / 64) + (threadIdx.x >> 6);
  if (row >= p.rows) return;                                  // (wave-uniform; no barrier in this kernel)
  const float* x_row = p.x + row * p.x_stride;
  const uint32_t e0 = lane * kPiece;
  const Piece piece = gate_piece(load_raw<VEC>(x_row, e0, p.k), e0, p);   // lanes past K hold zeros
  float lo = 0.0f, hi = 0.0f;
  piece_range(piece, lo, hi);
  wave_range(lo, hi);
  const RowQuant r = row_quant(lo, hi);
  if (e0 < p.k_pad) store_piece(piece, p.q + row * p.k_pad, e0, p.k, r);
  if (lane == 0) store_entry(p.table + row, r);
}

template <bool VEC>
__global__ __launch_bounds__(kRowsThreads)
void f32_qd8_gated_rows_block_kernel(const GatedRowsParams p)
{
  __shared__ float range[4][2];
  const uint64_t row = blockIdx.x;
  const float* x_row = p.x + row * p.x_stride;
  Piece piece[kBlockPieces];
  float lo = 0.0f, hi = 0.0f;
  RawPiece raw = load_raw<VEC>(x_row, threadIdx.x * kPiece, p.k);
#pragma unroll
  for (int i = 0; i < kBlockPieces; i++) {
    const uint32_t e0 = (i * kRowsThreads + threadIdx.x) * kPiece;
    RawPiece next = raw;                       // (only so that the last trip's `raw = next` has a value: no register is copied)
    if (i + 1 < kBlockPieces) next = load_raw<VEC>(x_row, e0 + kRowsThreads * kPiece, p.k);   // in flight under piece i
    piece[i] = gate_piece(raw, e0, p);
    piece_range(piece[i], lo, hi);
    raw = next;
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
void f32_qd8_gated_rows_twopass_kernel(const GatedRowsParams p)
{
  __shared__ float range[4][2];
  constexpr uint32_t kStep = kRowsThreads * kPiece;
  const uint64_t row = blockIdx.x;
  const float* x_row = p.x + row * p.x_stride;
  float lo = 0.0f, hi = 0.0f;
  RawPiece raw = load_raw<VEC>(x_row, threadIdx.x * kPiece, p.k);
  for (uint32_t e0 = threadIdx.x * kPiece; e0 < p.k; e0 += kStep) {
    const RawPiece next = load_raw<VEC>(x_row, e0 + kStep, p.k);       // (nothing is read at or past K)
    const Piece piece = gate_piece(raw, e0, p);
    piece_range(piece, lo, hi);
    raw = next;
  }
  wave_range(lo, hi);
  block_range(lo, hi, range);
  const RowQuant r = row_quant(lo, hi);
  int8_t* q_row = p.q + row * p.k_pad;
  raw = load_raw<VEC>(x_row, threadIdx.x * kPiece, p.k);
  for (uint32_t e0 = threadIdx.x * kPiece; e0 < p.k_pad; e0 += kStep) {
    const RawPiece next = load_raw<VEC>(x_row, e0 + kStep, p.k);
    const Piece piece = gate_piece(raw, e0, p);                        // the first walk's bits again
    store_piece(piece, q_row, e0, p.k, r);
    raw = next;
  }
  if (threadIdx.x == 0) store_entry(p.table + row, r);
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_qd8_gated_rows_run(const struct qnnp_hip_qd8_gated_rows_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->input == nullptr || a->quantized == nullptr || a->row_table == nullptr ||
      (reinterpret_cast<uintptr_t>(a->input) & 3u) != 0 || (reinterpret_cast<uintptr_t>(a->quantized) & 15u) != 0 ||
      a->k == 0 || a->k > 32768u || a->k_pad != ((a->k + 63u) & ~63u) || a->rows > 0x7FFFFFFFu ||
      a->input_stride < 2 * static_cast<uint64_t>(a->k)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->rows == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  GatedRowsParams p;
  p.x = a->input;
  p.q = a->quantized;
  p.table = a->row_table;
  p.x_stride = a->input_stride;
  p.rows = a->rows;
  p.k = a->k;
  p.k_pad = a->k_pad;
  p.alpha = a->alpha;
  p.limit = a->limit;
  p.up_shift = a->up_shift;
  const bool vec = (reinterpret_cast<uintptr_t>(a->input) & 15u) == 0 && (a->rows == 1 || a->input_stride % 4 == 0);
  const char* name;
  if (a->k <= kWaveMaxK) {
    const dim3 grid((a->rows + 3u) / 4u);
    if (vec) hipLaunchKernelGGL((f32_qd8_gated_rows_wave_kernel<true>), grid, dim3(kRowsThreads), 0, stream, p);
    else hipLaunchKernelGGL((f32_qd8_gated_rows_wave_kernel<false>), grid, dim3(kRowsThreads), 0, stream, p);
    name = vec ? "f32_qd8_gated_rows_wave" : "f32_qd8_gated_rows_wave_x4";
  } else if (a->k <= kBlockMaxK) {
    if (vec) hipLaunchKernelGGL((f32_qd8_gated_rows_block_kernel<true>), dim3(a->rows), dim3(kRowsThreads), 0, stream, p);
    else hipLaunchKernelGGL((f32_qd8_gated_rows_block_kernel<false>), dim3(a->rows), dim3(kRowsThreads), 0, stream, p);
    name = vec ? "f32_qd8_gated_rows_block" : "f32_qd8_gated_rows_block_x4";
  } else {
    if (vec) hipLaunchKernelGGL((f32_qd8_gated_rows_twopass_kernel<true>), dim3(a->rows), dim3(kRowsThreads), 0, stream, p);
    else hipLaunchKernelGGL((f32_qd8_gated_rows_twopass_kernel<false>), dim3(a->rows), dim3(kRowsThreads), 0, stream, p);
    name = vec ? "f32_qd8_gated_rows_twopass" : "f32_qd8_gated_rows_twopass_x4";
  }
  if (kernel_name != nullptr) *kernel_name = name;
  return launch_status();
}
